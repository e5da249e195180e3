// stage_gpu_ctx.hpp — DEVICE-ONLY: the GPU's execution context of the output-stage tile kernels (truepeak_tile.hpp over StageGpuCtx<float>,
// limiter_tile.hpp over StageGpuCtx<unsigned char>; T is the element type of the kernel's LDS image).  Its CPU counterpart is
// tests/emu/emu_stage_ctx.hpp; no host or emulation code includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace awk {

template <class T> struct StageGpuCtx {
    T *lds_;
    __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
    __device__ __forceinline__ T *lds() const { return lds_; }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
    __device__ __forceinline__ void ld16(const float *g, float (&x)[4]) const {
        const float4 v = *reinterpret_cast<const float4 *>(g);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    }
    __device__ __forceinline__ void st16(float *p, const float (&x)[4]) const { *reinterpret_cast<float4 *>(p) = make_float4(x[0], x[1], x[2], x[3]); }
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
    __device__ __forceinline__ uint32_t wave_max(uint32_t v) const {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(v, m); v = o > v ? o : v; }
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
    __device__ __forceinline__ void atomic_max(uint32_t *a, uint32_t v) const { atomicMax(a, v); }
    __device__ __forceinline__ void atomic_add(unsigned long long *a, unsigned long long v) const { atomicAdd(a, v); }
};

}  // namespace awk
