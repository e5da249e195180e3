// emu_true_peak.cpp — TEST-ONLY: the true-peak kernel (airwave_amd/csrc/device/truepeak_tile.hpp, the code hipcc compiles) on the CPU over
// emu_stage_ctx.hpp's context: one emulated workgroup of kTpThreads threads per tile and stream, the grid launch_truepeak makes.  Beside
// it the header's sequential rule.
#include "emu_stage_ctx.hpp"

#include "../../airwave_amd/csrc/device/truepeak_tile.hpp"

extern "C" {

int emu_true_peak_tile() { return awk::kTpTile; }

void emu_true_peak_filter(float *c) { float f[awtp::kCoefficients]; awtp::filter(f); std::memcpy(c, f, sizeof(f)); }

// in: [n_streams][frames][2] at any float (the test shifts it to try every alignment); hist_in / hist_out: [n_streams][11][2];
// tp_bits: [n_streams][2] or NULL; nonfinite: [n_streams]; call_tp: [n_streams]
void emu_true_peak(const float *in, int n_streams, long long frames, const float *hist_in, float *hist_out, uint32_t *tp_bits,
                   unsigned long long *nonfinite, uint32_t *call_tp) {
    awk::TruePeakParams p{};
    p.in = in; p.frames = frames; p.n_streams = n_streams;
    p.hist_in = hist_in; p.hist_out = hist_out; p.tp_bits = tp_bits; p.nonfinite = nonfinite; p.call_tp = call_tp;
    float c[awtp::kCoefficients];
    awtp::filter(c);
    std::memcpy(p.c, c, sizeof(c));
    const long long tiles = (frames + awk::kTpTile - 1) / awk::kTpTile;
    StageEmuShared sh(awk::kTpThreads, sizeof(float) * awk::kTpLdsFloats);
    for (int s = 0; s < n_streams; ++s)
        for (long long tile = 0; tile < tiles; ++tile)
            emu_workgroup(awk::kTpThreads, [&](int t) { awk::truepeak_tile(StageEmuCtx<float>{t, &sh}, p, s, tile); });
}

// the header's rule over the same buffers, stream by stream (hist carried in place)
void emu_true_peak_sequential(const float *in, int n_streams, long long frames, float *hist, uint32_t *tp_bits, unsigned long long *nonfinite,
                              uint32_t *call_tp) {
    float c[awtp::kCoefficients];
    awtp::filter(c);
    for (int s = 0; s < n_streams; ++s) {
        awtp::Record r{{tp_bits[2 * s], tp_bits[2 * s + 1]}, call_tp[s], nonfinite[s]};
        awtp::sequential(c, in + (size_t)s * frames * 2, frames, hist + (size_t)s * 22, r);
        tp_bits[2 * s] = r.tp_bits[0]; tp_bits[2 * s + 1] = r.tp_bits[1]; call_tp[s] = r.call_tp_bits; nonfinite[s] = r.nonfinite;
    }
}

}
