// rateconv.hpp — rules of the batch sample-rate converter (aw_rateconv_*, include/airwave_hip.h), shared by the kernel (rateconv_tile.hpp,
// rateconv_kernels.hip), the handle in rateconv_runtime.cpp and CPU tests that compile this header with plain g++.
//
// The reference resamples one thing, an HRIR at activation, by two-point linear interpolation (Resampler.swift:31-68; aw_resample here).
// That is right for an impulse response whose spectrum has rolled off long before Nyquist; applied to audio it images and aliases at about
// -30 dB.  Audio-rate conversion has no counterpart in the reference, so audio never takes that path: it goes through the polyphase
// Kaiser-windowed sinc below.
//
// Rates are positive integers in Hz.  g = gcd(in, out), L = out / g, M = in / g; equal rates and reduced terms above 640 are refused (640
// covers every pair among 44100, 48000, 88200, 96000, 176400 and 192000).  One quality: Z = 48 zero crossings a side, Kaiser beta = 10.
//   rho = min(1, L / M),  W = Z / rho,  D = ceil(W),  T = 2 D taps per phase,
//   A = beta / 0.1102 + 8.7,  delta = (A - 7.95) / (14.36 * 2 Z),  f_c = 0.5 - delta / 2      (the stopband starts at the lower Nyquist)
//   h(t) = 2 f_c rho sinc(2 f_c rho t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta)  for |t| <= W, else 0;   sinc(x) = sin(pi x) / (pi x)
//   c[p][k] = (float)h(k - D + p / L),  p = 0 .. L-1,  k = 0 .. T-1                              formed in double, rounded once.
// With x[j] the stream's input since the last reset (0 for j < 0), n the absolute output index, i_n = floor(n M / L), p_n = (n M) mod L
// (64-bit integers),
//   y[n] = fmaf(c[p_n][T-1], x[i_n+D-(T-1)], .. fmaf(c[p_n][1], x[i_n+D-1], c[p_n][0] * x[i_n+D]) ..)     float32, k = 0, 1, .., T-1, per channel.
// Output n sits at input time n M / L exactly (time aligned) and exists once input frame i_n + D has arrived: after N input frames there
// are max(0, ceil((N - D) L / M)) outputs.  Inputs are not sanitised: a NaN reaches the outputs whose windows hold it.
//
// fmaf is correctly rounded on host and device, so y[n] is a pure function of the stream's input since the reset: splitting calls in
// time, sharding streams over handles and the kernel's tiling change no bit.  A stream carries its last T - 1 input frames and the two
// 64-bit counts of frames consumed and produced.
//
// Integer PCM in and out (aw_pcm_rateconv_*): the same rule between a decode and an encode, both pcm.hpp's.  For stream s of the handle
// (global stream first_stream + s) and channel ch: x = awp::decode_at of the input element (F32 as it is; the history stays decoded
// float32, so formats may change from call to call); y as above; u = (float)(y * g_s) under a fixed gain, else y; F32 output is u, s32
// output awp::encode_s32(u), s16 / s24 output awp::encode_dithered_at's rule with d = awp::dither_value(mode, K_j, n, e), where n is the
// stream's absolute output index since the last reset or flush (the same n as above), j = ch >> 1, e = ch & 1 and
//   K_j = awp::dither_key(seed, first_stream + s) + j * 0xA0761D6478BD642F   (mod 2^64).
// K_0 is the spatializer's key, so a stereo converter's noise at frame n is the spatializer's at position n; further channel pairs get
// keys of their own, for the spatializer's 2 p + ear counter would collide from the third channel on.  Per stream, while metering is on:
// peak = max |y| over finite samples of all channels (before the gain), nonfinite = NaN / +-inf y, frames = output frames written,
// clipped = samples the integer encode clipped (after gain and dither): maxima and integer sums, so every field is exact and, like every
// output byte, independent of call splitting, sharding, byte alignment and tiling.
//
// True peak of the converted output (aw_tp_rateconv_*): truepeak.hpp's rule, per channel, on the converter's own float32 output.  For
// stream s, channel ch and the absolute output index n since the last reset or flush: y[n] as above, BEFORE gain, dither and encode;
// v[n] = awtp::filter_input(y[n]) (y where finite, else 0) and v[n] = 0 for n < 0; frame n of channel ch contributes
// awtp::frame_peak_bits over v[n], v[n-1], .., v[n-11] of that channel.  Per stream: true_peak = the max of the contributions over
// channels and frames, sample_peak = max |v| over the same frames, frames = output frames measured: maxima of bit patterns and an
// integer sum, so every field is exact and independent of call splitting, sharding, alignment, formats and tiling.  A stream carries
// its last 11 cleaned output frames [11][channels]; flush and reset zero them, a call that produces nothing leaves them, a call of fewer
// than 11 outputs carries a mix of old and new ones.  The six-frame look-ahead of the centred filter is not flushed (the spatializer's
// rule).  The ceiling is host arithmetic over a measuring pass: g = tp > c ? c / tp : 1 in float32 (ceiling_gain below), then a fixed gain.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "pcm.hpp"
#include "truepeak.hpp"

namespace awrc {

constexpr int kZeroCrossings = 48;       // Z
constexpr double kBeta = 10.0;           // Kaiser beta
constexpr int kMaxTerm = 640;            // the largest reduced L or M
constexpr int kMaxChannels = 16;

struct Plan {
    int L = 0, M = 0;                    // out / g, in / g
    int taps = 0, latency = 0;           // T, D (input frames)
};

enum PlanError { kPlanOk = 0, kPlanNotIntegral, kPlanEqual, kPlanTooLarge };

inline PlanError plan(double in_rate, double out_rate, Plan &p) {
    if (!(in_rate >= 1.0) || !(out_rate >= 1.0) || !(in_rate <= 2147483647.0) || !(out_rate <= 2147483647.0) ||
        in_rate != std::floor(in_rate) || out_rate != std::floor(out_rate))
        return kPlanNotIntegral;
    const long long a = (long long)in_rate, b = (long long)out_rate;
    if (a == b) return kPlanEqual;
    long long g = a, r = b;
    while (r) { const long long t = g % r; g = r; r = t; }
    if (a / g > kMaxTerm || b / g > kMaxTerm) return kPlanTooLarge;
    p.L = (int)(b / g); p.M = (int)(a / g);
    p.latency = p.M > p.L ? (kZeroCrossings * p.M + p.L - 1) / p.L : kZeroCrossings;      // ceil(Z / rho)
    p.taps = 2 * p.latency;
    return kPlanOk;
}

// I0 by its power series: the terms ((x / 2)^m / m!)^2 fall monotonically from m > x / 2 on
inline double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int m = 1; m < 500; ++m) {
        term *= q / ((double)m * (double)m);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

// c [L][T]
inline void filter(const Plan &p, float *c) {
    const double rho = p.M > p.L ? (double)p.L / (double)p.M : 1.0;
    const double W = (double)kZeroCrossings / rho;
    const double A = kBeta / 0.1102 + 8.7;
    const double delta = (A - 7.95) / (14.36 * 2.0 * (double)kZeroCrossings);
    const double fc2 = 2.0 * (0.5 - 0.5 * delta) * rho;
    const double i0b = bessel_i0(kBeta);
    for (int ph = 0; ph < p.L; ++ph)
        for (int k = 0; k < p.taps; ++k) {
            const double t = (double)(k - p.latency) + (double)ph / (double)p.L;
            double h = 0.0;
            if (std::fabs(t) <= W) {
                const double u = t / W, v = 1.0 - u * u, x = M_PI * fc2 * t;
                h = fc2 * (x == 0.0 ? 1.0 : std::sin(x) / x) * bessel_i0(kBeta * std::sqrt(v > 0.0 ? v : 0.0)) / i0b;
            }
            c[(size_t)ph * p.taps + k] = (float)h;
        }
}

// i_n and p_n
AWP_HD long long input_index(long long n, int L, int M) { return n * (long long)M / (long long)L; }
AWP_HD int phase(long long n, int L, int M) { return (int)(n * (long long)M % (long long)L); }

// outputs that exist after N input frames: max(0, ceil((N - D) L / M))
AWP_HD long long outputs_after(long long N, int L, int M, int D) {
    return N > D ? ((N - D) * (long long)L + M - 1) / M : 0;
}

// y[n] of one channel: c = c[p_n], x[-k * stride] = the channel's input frame i_n + D - k
AWP_HD float output_sample(const float *c, const float *x, int taps, long long stride) {
    float y = c[0] * x[0];
    for (int k = 1; k < taps; ++k) y = __builtin_fmaf(c[k], x[-(long long)k * stride], y);
    return y;
}

// What a stream carries beside its last T - 1 input frames.
struct Counts {
    long long consumed = 0, produced = 0;
};

// The rule, output by output: x [frames][channels] continues a stream whose last T - 1 frames are hist [T-1][channels] (oldest first),
// which is carried on with the counts.  Writes the outputs that now exist to y [..][channels], dense, and returns how many.
inline long long sequential(const Plan &p, const float *c, const float *x, long long frames, int channels, float *hist, Counts &n, float *y) {
    const int T = p.taps, C = channels;
    if (frames <= 0) return 0;
    std::vector<float> ext((size_t)(T - 1 + frames) * C);        // input frames consumed - (T - 1) .. consumed + frames - 1
    for (size_t i = 0; i < (size_t)(T - 1) * C; ++i) ext[i] = hist[i];
    for (size_t i = 0; i < (size_t)frames * C; ++i) ext[(size_t)(T - 1) * C + i] = x[i];
    const long long end = outputs_after(n.consumed + frames, p.L, p.M, p.latency);
    long long made = 0;
    for (long long o = n.produced; o < end; ++o, ++made) {
        const long long top = input_index(o, p.L, p.M) + p.latency - (n.consumed - (T - 1));      // in ext; >= T - 1
        const float *row = c + (size_t)phase(o, p.L, p.M) * T;
        for (int ch = 0; ch < C; ++ch) y[made * C + ch] = output_sample(row, ext.data() + top * C + ch, T, C);
    }
    for (size_t i = 0; i < (size_t)(T - 1) * C; ++i) hist[i] = ext[(size_t)frames * C + i];
    n.consumed += frames;
    n.produced = end;
    return made;
}

// One stream's true-peak record (aw_rateconv_true_peak is its layout).
struct TruePeakRecord {
    uint32_t true_peak_bits;             // the bits of the largest frame contribution over channels and frames
    uint32_t sample_peak_bits;           // ... of max |v| over the same frames
    unsigned long long frames;           // output frames measured
};

// The true-peak rule, frame by frame: y [frames][channels] are a stream's next outputs, hist [11][channels] its last 11 cleaned output
// frames (oldest first), which are carried on.  c: awtp::filter.
inline void true_peak_sequential(const float *c, const float *y, long long frames, int channels, float *hist, TruePeakRecord &rec) {
    const int H = awtp::kHistory;
    for (int ch = 0; ch < channels; ++ch) {
        float w[awtp::kTaps];            // w[k] = v[n - k]
        w[0] = 0.0f;
        for (int k = 1; k <= H; ++k) w[k] = hist[(H - k) * channels + ch];
        for (long long n = 0; n < frames; ++n) {
            if (n > 0) for (int k = H; k > 0; --k) w[k] = w[k - 1];
            unsigned nonfinite = 0;
            w[0] = awtp::filter_input(y[n * channels + ch], nonfinite);
            const uint32_t a = awtp::float_bits(w[0]) & 0x7FFFFFFFu, m = awtp::frame_peak_bits(c, w, 1);
            if (a > rec.sample_peak_bits) rec.sample_peak_bits = a;
            if (m > rec.true_peak_bits) rec.true_peak_bits = m;
        }
        if (frames > 0) for (int k = 1; k <= H; ++k) hist[(H - k) * channels + ch] = w[k - 1];
    }
    rec.frames += (unsigned long long)(frames > 0 ? frames : 0);
}

// The gain that holds ceiling c over a stream whose measured true peak is tp.
inline float ceiling_gain(float tp, float c) { return tp > c ? c / tp : 1.0f; }

}  // namespace awrc
