// emu_rateconv_pcm.cpp — TEST-ONLY: the PCM form of the sample-rate converter's kernel (airwave_amd/csrc/device/rateconv_tile.hpp,
// rateconv_tile_pcm: the code hipcc compiles) on the CPU over emu_stage_ctx.hpp's context, on the grid launch_rateconv_pcm makes.  Beside
// it the reference: the COMPOSITION of the separately tested rules, element by element and never through the kernel's vector paths —
// awp::decode_at, awrc::sequential, the gain product, awp::encode_dithered_at with the key rule of include/airwave_hip.h.
#include "emu_stage_ctx.hpp"

#include "../../airwave_amd/csrc/device/rateconv_tile.hpp"

namespace {

// what a call carries beside its buffers (ctypes mirrors this layout)
struct Settings {
    int in_format, out_format, dither, reserved;
    unsigned long long seed, first_stream;
    const float *gains;                  // [n_streams] or NULL
    awk::RateconvLevels *levels;         // [n_streams] or NULL
    unsigned long long *clipped;         // or NULL
};

constexpr unsigned long long kPairKey = 0xA0761D6478BD642Full;

}  // namespace

extern "C" {

unsigned long long emu_rateconv_pcm_key(unsigned long long seed, unsigned long long global_stream, int channel) {
    return awp::dither_key(seed, global_stream) + (unsigned long long)(channel >> 1) * kPairKey;
}

float emu_rateconv_pcm_dither(int mode, unsigned long long key, unsigned long long n, int e) { return awp::dither_value(mode, key, n, e); }

// One call of the kernel's PCM form.  in: [n_streams][in_frames][channels] elements of st->in_format at any byte, or NULL for zeros; out:
// dense in the count returned, elements of st->out_format at any byte; the rest as emu_rateconv (emu_rateconv.cpp).
long long emu_rateconv_pcm(double in_rate, double out_rate, int channels, const void *in, int n_streams, long long in_frames, const float *hist_in,
                           float *hist_out, long long *counts, long long *dev_counts, void *out, const Settings *st) {
    awrc::Plan pl;
    if (awrc::plan(in_rate, out_rate, pl) != awrc::kPlanOk || in_frames <= 0) return -1;
    awk::RateconvParams p{};
    p.in = static_cast<const float *>(in); p.in_frames = in_frames; p.out = static_cast<float *>(out);
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
    const long long tiles = (p.out_frames + p.tile - 1) / p.tile;
    StageEmuShared sh(awk::kRcThreads, sizeof(float) * awk::kRcLdsFloats);
    for (int s = 0; s < n_streams; ++s)
        for (long long tile = 0; tile < (tiles > 0 ? tiles : 1); ++tile)
            emu_workgroup(awk::kRcThreads, [&](int t) { awk::rateconv_tile_pcm(StageEmuCtx<float>{t, &sh}, p, s, tile); });
    counts[0] += in_frames; counts[1] += p.out_frames;
    return p.out_frames;
}

// The composition over the same buffers, stream by stream and element by element (hist carried in place); in NULL: zeros.
long long emu_rateconv_pcm_composition(double in_rate, double out_rate, int channels, const void *in, int n_streams, long long in_frames, float *hist,
                                       long long *counts, void *out, const Settings *st) {
    awrc::Plan pl;
    if (awrc::plan(in_rate, out_rate, pl) != awrc::kPlanOk || in_frames <= 0) return -1;
    const int C = channels, bi = awp::format_bytes(st->in_format), bo = awp::format_bytes(st->out_format);
    if (!bi || !bo) return -3;
    std::vector<float> c((size_t)pl.L * pl.taps), x((size_t)in_frames * C, 0.0f);
    awrc::filter(pl, c.data());
    const long long n_out = awrc::outputs_after(counts[0] + in_frames, pl.L, pl.M, pl.latency) - counts[1];
    std::vector<float> y((size_t)(n_out > 0 ? n_out : 0) * C);
    awrc::Counts after{counts[0], counts[1]};
    for (int s = 0; s < n_streams; ++s) {
        if (in)                                                                                       // 1. decode
            for (size_t i = 0; i < x.size(); ++i) x[i] = awp::decode_at(st->in_format, static_cast<const unsigned char *>(in) + ((size_t)s * x.size() + i) * bi);
        awrc::Counts n{counts[0], counts[1]};
        const long long made = awrc::sequential(pl, c.data(), x.data(), in_frames, C, hist + (size_t)s * (pl.taps - 1) * C, n, y.data());      // 2. convert
        if (made != n_out) return -2;
        after = n;
        unsigned long long clipped = 0, nonfinite = 0;
        float peak = 0.0f;
        for (long long f = 0; f < made; ++f)
            for (int ch = 0; ch < C; ++ch) {
                const float v = y[(size_t)f * C + ch];
                if (std::isfinite(v)) peak = std::fabs(v) > peak ? std::fabs(v) : peak; else ++nonfinite;
                const float u = st->gains ? v * st->gains[s] : v;                                     // 3. gain
                unsigned clip = 0;
                awp::encode_dithered_at(st->out_format, st->dither, u, emu_rateconv_pcm_key(st->seed, st->first_stream + (unsigned long long)s, ch),
                                        (uint64_t)(counts[1] + f), ch & 1, static_cast<unsigned char *>(out) + (((size_t)s * made + f) * C + ch) * bo, &clip);      // 4. encode
                clipped += clip;
            }
        if (st->levels) {
            awk::RateconvLevels &r = st->levels[s];
            float old;
            std::memcpy(&old, &r.peak_bits, 4);
            if (peak > old) std::memcpy(&r.peak_bits, &peak, 4);
            r.frames += (unsigned long long)made; r.clipped += clipped; r.nonfinite += nonfinite;
        }
        if (st->clipped) *st->clipped += clipped;
    }
    counts[0] = after.consumed; counts[1] = after.produced;
    return n_out;
}

}
