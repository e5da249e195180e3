// limiter_kernels.hip — gfx950 kernel of the look-ahead true-peak limiter (device code in limiter_tile.hpp).
#include "limiter_kernels.hpp"
#include "stage_gpu_ctx.hpp"

namespace awk {

// grid: (tiles of a stream, streams)
__global__ void __launch_bounds__(kLimThreads) aw_limiter_kernel(LimiterParams p) {
    __shared__ __align__(16) unsigned char lim_lds[kLimLdsBytes];
    StageGpuCtx<unsigned char> ctx{lim_lds};
    limiter_tile<StageGpuCtx<unsigned char>>(ctx, p, (long long)blockIdx.y, (long long)blockIdx.x);
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
