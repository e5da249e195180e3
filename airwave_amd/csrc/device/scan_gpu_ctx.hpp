// scan_gpu_ctx.hpp — DEVICE-ONLY: the GPU's execution context of the chunk-parallel scan kernels (eq_cascade.hpp in eq_kernels.hip,
// loudness_scan.hpp in loudness_kernels.hip).  Its CPU counterpart is EmuCtx (tests/emu/emu_ctx.hpp); no host or emulation code includes
// this header.
#pragma once
#include <hip/hip_runtime.h>

#include "cplx.hpp"

namespace awk {

struct ScanGpuCtx {
    cf *lds_;
    __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int wave() const { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
    __device__ __forceinline__ cf *lds() const { return lds_; }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
    // Cross-lane moves of the in-register scan (two DPP v_mov_b32 per double).  Lanes without a source receive zero
    // (row_shr: bound_ctrl; row_bcast: the rows outside the row mask keep the zero `old`).
    template <int CTRL, int ROW_MASK, bool BOUND>
    static __device__ __forceinline__ double dpp(double old, double v) {
        const unsigned long long o = __builtin_bit_cast(unsigned long long, old), u = __builtin_bit_cast(unsigned long long, v);
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)u, CTRL, ROW_MASK, 0xf, BOUND);
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(u >> 32), CTRL, ROW_MASK, 0xf, BOUND);
        return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
    }
    // x = a x + c in x's own register (a tied operand): the filter loop carries the chunk's samples of both ears in fixed registers,
    // without it hipcc renames them in every filter and copies them all back at the loop's back edge.  `after0/1` only order the
    // statement behind the other readers of the old x.
    __device__ __forceinline__ void fma_in_place(double &x, double a, double c, double after0, double after1) const {
        asm("v_fma_f64 %0, %1, %0, %2" : "+v"(x) : "s"(a), "v"(c), "v"(after0), "v"(after1));
    }
    template <int D> __device__ __forceinline__ double row_shr(double v) const { return dpp<0x110 + D, 0xf, true>(0.0, v); }   // lane - D of the same 16-lane row
    __device__ __forceinline__ double row_bcast15(double v) const { return dpp<0x142, 0xa, false>(0.0, v); }   // rows 1, 3 <- lane 15 of the row below
    __device__ __forceinline__ double row_bcast31(double v) const { return dpp<0x143, 0xc, false>(0.0, v); }   // rows 2, 3 <- lane 31
    __device__ __forceinline__ double wave_shr1(double v, double fill) const { return dpp<0x138, 0xf, false>(fill, v); }   // lane - 1; lane 0 <- fill
};

}  // namespace awk
