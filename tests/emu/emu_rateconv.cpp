// emu_rateconv.cpp — TEST-ONLY: the sample-rate converter's kernel (airwave_amd/csrc/device/rateconv_tile.hpp, the code hipcc compiles) on
// the CPU over emu_stage_ctx.hpp's context: one emulated workgroup of kRcThreads threads per tile and stream, the grid launch_rateconv
// makes (one workgroup per stream when a call produces nothing).  Beside it the header's sequential rule, the plan and the table.
#include "emu_stage_ctx.hpp"

#include "../../airwave_amd/csrc/device/rateconv_tile.hpp"

namespace {

bool planned(double in_rate, double out_rate, awrc::Plan &p) { return awrc::plan(in_rate, out_rate, p) == awrc::kPlanOk; }

}  // namespace

extern "C" {

// o: L, M, taps, latency; returns awrc::PlanError
int emu_rateconv_plan(double in_rate, double out_rate, int *o) {
    awrc::Plan p;
    const int e = awrc::plan(in_rate, out_rate, p);
    if (e == awrc::kPlanOk) { o[0] = p.L; o[1] = p.M; o[2] = p.taps; o[3] = p.latency; }
    return e;
}

// c [L][taps]
int emu_rateconv_filter(double in_rate, double out_rate, float *c) {
    awrc::Plan p;
    if (!planned(in_rate, out_rate, p)) return -1;
    awrc::filter(p, c);
    return 0;
}

int emu_rateconv_tile(double in_rate, double out_rate, int channels) {
    awrc::Plan p;
    return planned(in_rate, out_rate, p) ? awk::rc_tile(p.L, p.M, p.taps, channels) : -1;
}

int emu_rateconv_lds_floats() { return awk::kRcLdsFloats; }

// One call of the kernel.  in: [n_streams][in_frames][channels] at any float, or NULL for zeros; hist_in / hist_out: [n_streams][taps - 1][channels];
// counts: [2] consumed and produced before the call, carried on; dev_counts: [n_streams][2] as the kernel writes them; out: dense in the
// count returned.  -1: the rates have no plan.
long long emu_rateconv(double in_rate, double out_rate, int channels, const float *in, int n_streams, long long in_frames, const float *hist_in,
                       float *hist_out, long long *counts, long long *dev_counts, float *out) {
    awrc::Plan pl;
    if (!planned(in_rate, out_rate, pl) || in_frames <= 0) return -1;
    awk::RateconvParams p{};
    p.in = in; p.in_frames = in_frames; p.out = out;
    p.out_frames = awrc::outputs_after(counts[0] + in_frames, pl.L, pl.M, pl.latency) - counts[1];
    p.n_streams = n_streams; p.channels = channels;
    p.L = pl.L; p.M = pl.M; p.taps = pl.taps; p.latency = pl.latency;
    p.tile = awk::rc_tile(pl.L, pl.M, pl.taps, channels);
    p.row_stride = awk::rc_row_stride(pl.taps);
    // the table as the handle uploads it: rows padded to 16-byte words, on a 16-byte boundary; the pad poisoned, for no tap reads it
    std::vector<float> dense((size_t)pl.L * pl.taps), rows((size_t)pl.L * p.row_stride + 4, std::nanf(""));
    awrc::filter(pl, dense.data());
    float *c = rows.data() + ((16 - (reinterpret_cast<uintptr_t>(rows.data()) & 15u)) & 15u) / 4;
    for (int ph = 0; ph < pl.L; ++ph)
        for (int k = 0; k < pl.taps; ++k) c[(size_t)ph * p.row_stride + k] = dense[(size_t)ph * pl.taps + k];
    p.c = c;
    p.hist_in = hist_in; p.hist_out = hist_out;
    p.consumed = counts[0]; p.produced = counts[1]; p.counts = dev_counts;
    const long long tiles = (p.out_frames + p.tile - 1) / p.tile;
    StageEmuShared sh(awk::kRcThreads, sizeof(float) * awk::kRcLdsFloats);
    for (int s = 0; s < n_streams; ++s)
        for (long long tile = 0; tile < (tiles > 0 ? tiles : 1); ++tile)
            emu_workgroup(awk::kRcThreads, [&](int t) { awk::rateconv_tile(StageEmuCtx<float>{t, &sh}, p, s, tile); });
    counts[0] += in_frames; counts[1] += p.out_frames;
    return p.out_frames;
}

// the header's rule over the same buffers, stream by stream (hist carried in place); in NULL: zeros
long long emu_rateconv_sequential(double in_rate, double out_rate, int channels, const float *in, int n_streams, long long in_frames, float *hist,
                                  long long *counts, float *out) {
    awrc::Plan pl;
    if (!planned(in_rate, out_rate, pl) || in_frames <= 0) return -1;
    std::vector<float> c((size_t)pl.L * pl.taps), zeros(in ? 0 : (size_t)in_frames * channels, 0.0f);
    awrc::filter(pl, c.data());
    const long long n_out = awrc::outputs_after(counts[0] + in_frames, pl.L, pl.M, pl.latency) - counts[1];
    awrc::Counts after{counts[0], counts[1]};
    for (int s = 0; s < n_streams; ++s) {
        awrc::Counts n{counts[0], counts[1]};
        const long long made = awrc::sequential(pl, c.data(), in ? in + (size_t)s * in_frames * channels : zeros.data(), in_frames, channels,
                                                hist + (size_t)s * (pl.taps - 1) * channels, n, out + (size_t)s * n_out * channels);
        if (made != n_out) return -2;
        after = n;
    }
    counts[0] = after.consumed; counts[1] = after.produced;
    return n_out;
}

}
