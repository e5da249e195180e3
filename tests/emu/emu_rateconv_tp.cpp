// emu_rateconv_tp.cpp — TEST-ONLY: the measuring forms of the sample-rate converter's kernel (airwave_amd/csrc/device/rateconv_tile.hpp,
// rateconv_tile_pcm_tp and rateconv_tile_tp_measure: the code hipcc compiles) on the CPU over emu_stage_ctx.hpp's context, on the grid
// launch_rateconv_pcm_tp makes.  Beside it the true-peak rule alone (awrc::true_peak_sequential over awtp::filter), which the tests
// compose with emu_rateconv_pcm.cpp's composition, and the two tile-length functions.
#include "emu_stage_ctx.hpp"

#include "../../airwave_amd/csrc/device/rateconv_tile.hpp"

namespace {

// emu_rateconv_pcm.cpp's Settings (ctypes mirrors this layout)
struct Settings {
    int in_format, out_format, dither, reserved;
    unsigned long long seed, first_stream;
    const float *gains;
    awk::RateconvLevels *levels;
    unsigned long long *clipped;
};

}  // namespace

extern "C" {

int emu_rateconv_tp_tiles(int L, int M, int taps, int channels, int *tile, int *tp_tile) {
    *tile = awk::rc_tile(L, M, taps, channels);
    *tp_tile = awk::rc_tp_tile(L, M, taps, channels);
    return 0;
}

void emu_rateconv_tp_filter(float *c36) {
    float c[awtp::kCoefficients];
    awtp::filter(c);
    std::memcpy(c36, c, sizeof c);
}

float emu_rateconv_tp_ceiling_gain(float tp, float c) { return awrc::ceiling_gain(tp, c); }

// One call of a measuring form; the arguments of emu_rateconv_pcm (emu_rateconv_pcm.cpp), then the carried v slots [n_streams][11][channels],
// the records and the form: measure_only != 0 is rateconv_tile_tp_measure, which gets no output buffer.
long long emu_rateconv_tp(double in_rate, double out_rate, int channels, const void *in, int n_streams, long long in_frames, const float *hist_in,
                          float *hist_out, long long *counts, long long *dev_counts, void *out, const Settings *st, const float *tp_hist_in,
                          float *tp_hist_out, awk::RateconvTruePeak *records, int measure_only) {
    awrc::Plan pl;
    if (awrc::plan(in_rate, out_rate, pl) != awrc::kPlanOk || in_frames <= 0) return -1;
    awk::RateconvParams p{};
    p.in = static_cast<const float *>(in); p.in_frames = in_frames; p.out = measure_only ? nullptr : static_cast<float *>(out);
    p.out_frames = awrc::outputs_after(counts[0] + in_frames, pl.L, pl.M, pl.latency) - counts[1];
    p.n_streams = n_streams; p.channels = channels;
    p.L = pl.L; p.M = pl.M; p.taps = pl.taps; p.latency = pl.latency;
    p.tile = awk::rc_tile(pl.L, pl.M, pl.taps, channels);
    p.row_stride = awk::rc_row_stride(pl.taps);
    std::vector<float> dense((size_t)pl.L * pl.taps), rows((size_t)pl.L * p.row_stride + 4, std::nanf(""));
    awrc::filter(pl, dense.data());
    float *c = rows.data() + ((16 - (reinterpret_cast<uintptr_t>(rows.data()) & 15u)) & 15u) / 4;
    for (int ph = 0; ph < pl.L; ++ph)
        for (int k = 0; k < pl.taps; ++k) c[(size_t)ph * p.row_stride + k] = dense[(size_t)ph * pl.taps + k];
    p.c = c;
    p.hist_in = hist_in; p.hist_out = hist_out;
    p.consumed = counts[0]; p.produced = counts[1]; p.counts = dev_counts;
    p.in_format = st->in_format; p.out_format = st->out_format; p.dither = st->dither;
    p.dither_seed = st->seed; p.first_stream = st->first_stream;
    p.gains = st->gains; p.levels = st->levels; p.clipped = st->clipped;
    awk::RateconvTp tp{};
    tp.hist_in = tp_hist_in; tp.hist_out = tp_hist_out; tp.records = records;
    tp.tile = awk::rc_tp_tile(pl.L, pl.M, pl.taps, channels);
    if (tp.tile < 1) return -4;
    awtp::filter(tp.c);
    const long long tiles = (p.out_frames + tp.tile - 1) / tp.tile;
    StageEmuShared sh(awk::kRcThreads, sizeof(float) * awk::kRcLdsFloats);
    for (int s = 0; s < n_streams; ++s)
        for (long long tile = 0; tile < (tiles > 0 ? tiles : 1); ++tile)
            emu_workgroup(awk::kRcThreads, [&](int t) {
                if (measure_only) awk::rateconv_tile_tp_measure(StageEmuCtx<float>{t, &sh}, p, tp, s, tile);
                else awk::rateconv_tile_pcm_tp(StageEmuCtx<float>{t, &sh}, p, tp, s, tile);
            });
    counts[0] += in_frames; counts[1] += p.out_frames;
    return p.out_frames;
}

// The rule alone: y [n_streams][frames][channels] float32 are the streams' next outputs; hist [n_streams][11][channels] is carried in place.
void emu_rateconv_tp_rule(const float *y, int n_streams, long long frames, int channels, float *hist, awrc::TruePeakRecord *records) {
    float c[awtp::kCoefficients];
    awtp::filter(c);
    for (int s = 0; s < n_streams; ++s)
        awrc::true_peak_sequential(c, y + (size_t)s * frames * channels, frames, channels, hist + (size_t)s * awtp::kHistory * channels, records[s]);
}

}
