// rateconv_kernels.hip — gfx950 kernels of the sample-rate converter (device code in rateconv_tile.hpp): the float32 form, the PCM form and the
// two measuring forms of the PCM form.
#include "rateconv_kernels.hpp"
#include "stage_gpu_ctx.hpp"

namespace awk {

// grid: (tiles of a stream, streams)
__global__ void __launch_bounds__(kRcThreads) aw_rateconv_kernel(RateconvParams p) {
    __shared__ __align__(16) float rc_lds[kRcLdsFloats];
    StageGpuCtx<float> ctx{rc_lds};
    rateconv_tile<StageGpuCtx<float>>(ctx, p, (long long)blockIdx.y, (long long)blockIdx.x);
}

__global__ void __launch_bounds__(kRcThreads) aw_rateconv_pcm_kernel(RateconvParams p) {
    __shared__ __align__(16) float rc_lds[kRcLdsFloats];
    StageGpuCtx<float> ctx{rc_lds};
    rateconv_tile_pcm<StageGpuCtx<float>>(ctx, p, (long long)blockIdx.y, (long long)blockIdx.x);
}

__global__ void __launch_bounds__(kRcThreads) aw_rateconv_pcm_tp_kernel(RateconvParams p, RateconvTp tp) {
    __shared__ __align__(16) float rc_lds[kRcLdsFloats];
    StageGpuCtx<float> ctx{rc_lds};
    rateconv_tile_pcm_tp<StageGpuCtx<float>>(ctx, p, tp, (long long)blockIdx.y, (long long)blockIdx.x);
}

__global__ void __launch_bounds__(kRcThreads) aw_rateconv_tp_measure_kernel(RateconvParams p, RateconvTp tp) {
    __shared__ __align__(16) float rc_lds[kRcLdsFloats];
    StageGpuCtx<float> ctx{rc_lds};
    rateconv_tile_tp_measure<StageGpuCtx<float>>(ctx, p, tp, (long long)blockIdx.y, (long long)blockIdx.x);
}

namespace {

// pcm: p.in and p.out are byte buffers of p.in_format / p.out_format at any alignment
// tp: a measuring form of the PCM form, tiles of tp->tile; measure_only: the one that writes no output
hipError_t launch_form(const RateconvParams &p, bool pcm, hipStream_t stream, const RateconvTp *tp = nullptr, bool measure_only = false) {
    if (p.n_streams <= 0 || p.in_frames <= 0) return hipSuccess;
    if (p.channels < 1 || p.channels > awrc::kMaxChannels || p.L < 1 || p.M < 1 || p.L > awrc::kMaxTerm || p.M > awrc::kMaxTerm ||
        p.taps < 4 || p.taps != 2 * p.latency || p.row_stride != rc_row_stride(p.taps) || p.out_frames < 0 || p.consumed < 0 || p.produced < 0 ||
        p.tile < 1 || p.tile != rc_tile(p.L, p.M, p.taps, p.channels))
        return hipErrorInvalidValue;
    if (p.out_frames != awrc::outputs_after(p.consumed + p.in_frames, p.L, p.M, p.latency) - p.produced) return hipErrorInvalidValue;
    if (!p.c || !p.hist_in || !p.hist_out || p.hist_in == p.hist_out || !p.counts || (p.out_frames > 0 && !p.out && !measure_only) ||
        (reinterpret_cast<uintptr_t>(p.c) & 15u))
        return hipErrorInvalidValue;
    if (pcm) {
        if (!awp::format_bytes(p.in_format) || !awp::format_bytes(p.out_format) || p.dither < awp::kDitherNone || p.dither > awp::kDitherTpdfHp)
            return hipErrorInvalidValue;
    } else if ((reinterpret_cast<uintptr_t>(p.in) & 3u) || (reinterpret_cast<uintptr_t>(p.out) & 3u)) {
        return hipErrorInvalidValue;
    }
    if (tp && (!pcm || tp->tile < 1 || tp->tile != rc_tp_tile(p.L, p.M, p.taps, p.channels) || !tp->hist_in || !tp->hist_out ||
               tp->hist_in == tp->hist_out || !tp->records))
        return hipErrorInvalidValue;
    const int step = tp ? tp->tile : p.tile;
    const long long tiles = (p.out_frames + step - 1) / step;
    if (tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const size_t hist = (size_t)(p.taps - 1) * p.channels;
    const long long bi = pcm ? awp::format_bytes(p.in_format) : 4, bo = pcm ? awp::format_bytes(p.out_format) : 4;
    // the y dimension of a grid holds 65,535 workgroups: more streams go in slices
    for (int s0 = 0; s0 < p.n_streams; s0 += 65535) {
        RateconvParams q = p;
        q.n_streams = p.n_streams - s0 < 65535 ? p.n_streams - s0 : 65535;
        if (p.in) q.in = reinterpret_cast<const float *>(reinterpret_cast<const unsigned char *>(p.in) + (long long)s0 * p.in_frames * p.channels * bi);
        if (p.out) q.out = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(p.out) + (long long)s0 * p.out_frames * p.channels * bo);
        q.hist_in = p.hist_in + s0 * hist; q.hist_out = p.hist_out + s0 * hist;
        q.counts = p.counts + 2 * (size_t)s0;
        q.first_stream = p.first_stream + (unsigned long long)s0;
        if (p.gains) q.gains = p.gains + s0;
        if (p.levels) q.levels = p.levels + s0;
        const dim3 grid((unsigned)(tiles > 0 ? tiles : 1), (unsigned)q.n_streams);
        if (tp) {
            RateconvTp r = *tp;
            r.hist_in = tp->hist_in + (size_t)s0 * awtp::kHistory * p.channels; r.hist_out = tp->hist_out + (size_t)s0 * awtp::kHistory * p.channels;
            r.records = tp->records + s0;
            if (measure_only) hipLaunchKernelGGL(aw_rateconv_tp_measure_kernel, grid, dim3(kRcThreads), 0, stream, q, r);
            else hipLaunchKernelGGL(aw_rateconv_pcm_tp_kernel, grid, dim3(kRcThreads), 0, stream, q, r);
        } else if (pcm) hipLaunchKernelGGL(aw_rateconv_pcm_kernel, grid, dim3(kRcThreads), 0, stream, q);
        else hipLaunchKernelGGL(aw_rateconv_kernel, grid, dim3(kRcThreads), 0, stream, q);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_rateconv(const RateconvParams &p, hipStream_t stream) { return launch_form(p, false, stream); }
hipError_t launch_rateconv_pcm(const RateconvParams &p, hipStream_t stream) { return launch_form(p, true, stream); }
hipError_t launch_rateconv_pcm_tp(const RateconvParams &p, const RateconvTp &tp, hipStream_t stream) { return launch_form(p, true, stream, &tp); }
hipError_t launch_rateconv_tp_measure(const RateconvParams &p, const RateconvTp &tp, hipStream_t stream) { return launch_form(p, true, stream, &tp, true); }

}  // namespace awk
