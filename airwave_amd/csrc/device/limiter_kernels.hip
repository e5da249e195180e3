// limiter_kernels.hip — gfx950 kernel of the look-ahead true-peak limiter (device code in limiter_tile.hpp).
#include "limiter_kernels.hpp"

namespace awk {

namespace {

struct LimGpuCtx {
    unsigned char *lds_;
    __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
    __device__ __forceinline__ unsigned char *lds() const { return lds_; }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
    __device__ __forceinline__ void ld16(const float *g, float (&x)[4]) const {
        const float4 v = *reinterpret_cast<const float4 *>(g);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    }
    __device__ __forceinline__ void st16(float *g, const float (&x)[4]) const { *reinterpret_cast<float4 *>(g) = make_float4(x[0], x[1], x[2], x[3]); }
    __device__ __forceinline__ void ld_lds16(const float *l, float *x) const {
        const float4 v = *reinterpret_cast<const float4 *>(l);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    }
    __device__ __forceinline__ void ld_lds8(const float *l, float *x) const {
        const float2 v = *reinterpret_cast<const float2 *>(l);
        x[0] = v.x; x[1] = v.y;
    }
    // every wave is launched whole and keeps its lanes together at these calls, so the shuffles see all 64 lanes
    __device__ __forceinline__ uint32_t wave_min(uint32_t v) const {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(v, m); v = o < v ? o : v; }
        return v;
    }
    __device__ __forceinline__ unsigned wave_sum(unsigned v) const {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        return v;
    }
    // the sum of v over the lanes below this one
    __device__ __forceinline__ unsigned long long wave_exclusive_sum(unsigned long long v) const {
        const int lane = (int)(threadIdx.x & 63u);
        unsigned long long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        return incl - v;
    }
    __device__ __forceinline__ void atomic_min(uint32_t *a, uint32_t v) const { atomicMin(a, v); }
    __device__ __forceinline__ void atomic_add(unsigned long long *a, unsigned long long v) const { atomicAdd(a, v); }
};

}  // namespace

// grid: (tiles of a stream, streams)
__global__ void __launch_bounds__(kLimThreads) aw_limiter_kernel(LimiterParams p) {
    __shared__ __align__(16) unsigned char lim_lds[kLimLdsBytes];
    LimGpuCtx ctx{lim_lds};
    limiter_tile<LimGpuCtx>(ctx, p, (long long)blockIdx.y, (long long)blockIdx.x);
}

hipError_t prepare_limiter_kernels() { return hipSuccess; }       // static LDS under 64 KB: nothing to set

hipError_t launch_limiter(const LimiterParams &p, hipStream_t stream) {
    if (p.n_streams <= 0 || p.frames <= 0) return hipSuccess;
    if (!p.in || !p.out || p.in == p.out || !p.hist_in || !p.hist_out || p.hist_in == p.hist_out || !p.min_gain || !p.limited || !p.nonfinite ||
        ((reinterpret_cast<uintptr_t>(p.in) | reinterpret_cast<uintptr_t>(p.out)) & 3u) || !awlim::config_ok(p.L, p.H, p.ceiling))
        return hipErrorInvalidValue;
    const long long tiles = (p.frames + kLimTile - 1) / kLimTile;
    if (tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const size_t hist = 2 * (size_t)awlim::halo(p.L, p.H);
    // the y dimension of a grid holds 65,535 workgroups: more streams go in slices
    for (int s0 = 0; s0 < p.n_streams; s0 += 65535) {
        LimiterParams q = p;
        const int ns = p.n_streams - s0 < 65535 ? p.n_streams - s0 : 65535;
        q.in = p.in + (long long)s0 * p.frames * 2; q.out = p.out + (long long)s0 * p.frames * 2; q.n_streams = ns;
        if (p.gain) q.gain = p.gain + s0;
        q.hist_in = p.hist_in + (size_t)s0 * hist; q.hist_out = p.hist_out + (size_t)s0 * hist;
        q.min_gain = p.min_gain + s0; q.limited = p.limited + s0; q.nonfinite = p.nonfinite + s0;
        hipLaunchKernelGGL(aw_limiter_kernel, dim3((unsigned)tiles, (unsigned)ns), dim3(kLimThreads), 0, stream, q);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace awk
