// loudness_kernels.hip — gfx950 kernels of the per-stream integrated loudness (device code in loudness_scan.hpp).
#include "loudness_kernels.hpp"

namespace awk {

namespace {

// The execution context of the scan (the EQ kernel's: eq_kernels.hip): DPP moves of doubles, two v_mov_b32 each.  Lanes without a
// source receive zero (row_shr: bound_ctrl; row_bcast: the rows outside the row mask keep the zero `old`).
struct LdGpuCtx {
    cf *lds_;
    __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int wave() const { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
    __device__ __forceinline__ cf *lds() const { return lds_; }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
    template <int CTRL, int ROW_MASK, bool BOUND>
    static __device__ __forceinline__ double dpp(double old, double v) {
        const unsigned long long o = __builtin_bit_cast(unsigned long long, old), u = __builtin_bit_cast(unsigned long long, v);
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)u, CTRL, ROW_MASK, 0xf, BOUND);
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(u >> 32), CTRL, ROW_MASK, 0xf, BOUND);
        return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
    }
    // x = a x + c in x's own register: the filter loop carries the 2 x 32 samples in fixed registers (eq_kernels.hip)
    __device__ __forceinline__ void fma_in_place(double &x, double a, double c, double after0, double after1) const {
        asm("v_fma_f64 %0, %1, %0, %2" : "+v"(x) : "s"(a), "v"(c), "v"(after0), "v"(after1));
    }
    template <int D> __device__ __forceinline__ double row_shr(double v) const { return dpp<0x110 + D, 0xf, true>(0.0, v); }
    __device__ __forceinline__ double row_bcast15(double v) const { return dpp<0x142, 0xa, false>(0.0, v); }
    __device__ __forceinline__ double row_bcast31(double v) const { return dpp<0x143, 0xc, false>(0.0, v); }
    __device__ __forceinline__ double wave_shr1(double v, double fill) const { return dpp<0x138, 0xf, false>(fill, v); }
};

}  // namespace

// The tables come in as `const __restrict__` kernel arguments: with a wave-uniform index hipcc reads them with scalar loads.
__global__ void __launch_bounds__(kEqThreads, 2) aw_loudness_kernel(LoudnessParams p, const double *__restrict__ tab, const double *__restrict__ plane) {
    extern __shared__ __align__(16) unsigned char ld_lds[];
    LdGpuCtx ctx{reinterpret_cast<cf *>(ld_lds)};
    p.tab = tab;
    p.plane = plane;
    loudness_stream<LdGpuCtx>(ctx, p, (long long)blockIdx.x);
}

__global__ void aw_loudness_sequential_kernel(LoudnessParams p, int n_streams) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_streams) loudness_sequential(p, i);
}

hipError_t prepare_loudness_kernels() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&aw_loudness_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdLdsBytes);
}

hipError_t launch_loudness(const LoudnessParams &p, int n_streams, hipStream_t stream) {
    if (n_streams <= 0 || p.frames <= 0) return hipSuccess;
    const long long body = p.hop >= kEqChunk ? p.frames - p.frames % kEqChunk : 0;
    if (body > 0) {
        LoudnessParams q = p;
        q.frames = body;
        hipLaunchKernelGGL(aw_loudness_kernel, dim3((unsigned)n_streams), dim3(kEqThreads), kLdLdsBytes, stream, q, q.tab, q.plane);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (p.frames > body) {
        LoudnessParams q = p;
        q.in = p.in + body * 2; q.frames = p.frames - body; q.frame0 = p.frame0 + body;
        hipLaunchKernelGGL(aw_loudness_sequential_kernel, dim3((unsigned)((n_streams + 63) / 64)), dim3(64), 0, stream, q, n_streams);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace awk
