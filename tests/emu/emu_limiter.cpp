// emu_limiter.cpp — TEST-ONLY: the limiter kernel (airwave_amd/csrc/device/limiter_tile.hpp, the code hipcc compiles) on the CPU over
// emu_stage_ctx.hpp's context: one emulated workgroup of kLimThreads threads per tile and stream, the grid launch_limiter makes.  Beside
// it the header's sequential rule, its detector, and the true-peak rule for measuring an output.
#include "emu_stage_ctx.hpp"

#include "../../airwave_amd/csrc/device/limiter_tile.hpp"

extern "C" {

int emu_limiter_tile() { return awk::kLimTile; }
int emu_limiter_halo(int L, int H) { return awlim::halo(L, H); }
int emu_limiter_delay(int L) { return awlim::delay(L); }
void emu_limiter_filter(float *c) { float f[awtp::kCoefficients]; awtp::filter(f); std::memcpy(c, f, sizeof(f)); }

// in / out: [n_streams][frames][2] at any float (the test shifts them to try every alignment); gain: [n_streams] or NULL;
// hist_in / hist_out: [n_streams][halo][2]; min_gain, limited, nonfinite: [n_streams]
void emu_limiter(const float *in, float *out, int n_streams, long long frames, const float *gain, int L, int H, float ceiling,
                 const float *hist_in, float *hist_out, uint32_t *min_gain, unsigned long long *limited, unsigned long long *nonfinite) {
    awk::LimiterParams p{};
    p.in = in; p.out = out; p.frames = frames; p.n_streams = n_streams; p.gain = gain;
    p.hist_in = hist_in; p.hist_out = hist_out; p.min_gain = min_gain; p.limited = limited; p.nonfinite = nonfinite;
    p.L = L; p.H = H; p.ceiling = ceiling;
    float c[awtp::kCoefficients];
    awtp::filter(c);
    std::memcpy(p.c, c, sizeof(c));
    const long long tiles = (frames + awk::kLimTile - 1) / awk::kLimTile;
    StageEmuShared sh(awk::kLimThreads, awk::kLimLdsBytes);
    for (int s = 0; s < n_streams; ++s)
        for (long long tile = 0; tile < tiles; ++tile)
            emu_workgroup(awk::kLimThreads, [&](int t) { awk::limiter_tile(StageEmuCtx<unsigned char>{t, &sh}, p, s, tile); });
}

// the header's rule over the same buffers, stream by stream (hist carried in place); g_out [n_streams][frames] and p_out likewise, or NULL
void emu_limiter_sequential(const float *in, float *out, int n_streams, long long frames, const float *gain, int L, int H, float ceiling,
                            float *hist, uint32_t *min_gain, unsigned long long *limited, unsigned long long *nonfinite, float *g_out,
                            uint32_t *p_out) {
    float c[awtp::kCoefficients];
    awtp::filter(c);
    const size_t hl = 2 * (size_t)awlim::halo(L, H);
    for (int s = 0; s < n_streams; ++s) {
        awlim::Record r;
        r.min_gain_bits = min_gain[s]; r.limited_frames = limited[s]; r.nonfinite = nonfinite[s];
        awlim::sequential(c, L, H, ceiling, gain ? gain[s] : 1.0f, in + (size_t)s * frames * 2, frames, hist + (size_t)s * hl,
                          out + (size_t)s * frames * 2, r, g_out ? g_out + (size_t)s * frames : nullptr, p_out ? p_out + (size_t)s * frames : nullptr);
        min_gain[s] = r.min_gain_bits; limited[s] = r.limited_frames; nonfinite[s] = r.nonfinite;
    }
}

// awtp::sequential over one stream from silence: the bits of the larger ear's true peak
uint32_t emu_limiter_true_peak(const float *y, long long frames) {
    float c[awtp::kCoefficients], hist[2 * awtp::kHistory] = {};
    awtp::filter(c);
    awtp::Record r{};
    awtp::sequential(c, y, frames, hist, r);
    return r.tp_bits[0] > r.tp_bits[1] ? r.tp_bits[0] : r.tp_bits[1];
}

}
