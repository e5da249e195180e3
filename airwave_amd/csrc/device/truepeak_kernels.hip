// truepeak_kernels.hip — gfx950 kernel of the per-stream true peak (device code in truepeak_tile.hpp).
#include "truepeak_kernels.hpp"
#include "stage_gpu_ctx.hpp"

namespace awk {

// grid: (tiles of a stream, streams)
__global__ void __launch_bounds__(kTpThreads) aw_true_peak_kernel(TruePeakParams p) {
    __shared__ __align__(16) float tp_lds[kTpLdsFloats];
    StageGpuCtx<float> ctx{tp_lds};
    truepeak_tile<StageGpuCtx<float>>(ctx, p, (long long)blockIdx.y, (long long)blockIdx.x);
}

hipError_t prepare_truepeak_kernels() { return hipSuccess; }      // static LDS under 64 KB: nothing to set

hipError_t launch_truepeak(const TruePeakParams &p, hipStream_t stream) {
    if (p.n_streams <= 0 || p.frames <= 0) return hipSuccess;
    if (!p.in || !p.hist_in || !p.hist_out || p.hist_in == p.hist_out || !p.call_tp || (p.tp_bits && !p.nonfinite) ||
        (reinterpret_cast<uintptr_t>(p.in) & 3u))
        return hipErrorInvalidValue;
    const long long tiles = (p.frames + kTpTile - 1) / kTpTile;
    if (tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    // the y dimension of a grid holds 65,535 workgroups: more streams go in slices
    for (int s0 = 0; s0 < p.n_streams; s0 += 65535) {
        TruePeakParams q = p;
        const int ns = p.n_streams - s0 < 65535 ? p.n_streams - s0 : 65535;
        q.in = p.in + (long long)s0 * p.frames * 2; q.n_streams = ns;
        q.hist_in = p.hist_in + (size_t)s0 * 2 * awtp::kHistory; q.hist_out = p.hist_out + (size_t)s0 * 2 * awtp::kHistory;
        if (p.tp_bits) { q.tp_bits = p.tp_bits + 2 * (size_t)s0; q.nonfinite = p.nonfinite + s0; }
        q.call_tp = p.call_tp + s0;
        hipLaunchKernelGGL(aw_true_peak_kernel, dim3((unsigned)tiles, (unsigned)ns), dim3(kTpThreads), 0, stream, q);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace awk
