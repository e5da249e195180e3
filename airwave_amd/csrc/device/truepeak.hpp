// truepeak.hpp — rules of the per-stream true peak of the batch entries (ITU-R BS.1770-4 Annex 2, judged by EBU Tech 3341's tolerance;
// aw_stream_true_peak, aw_spatializer_set_true_peak / _get_true_peak, aw_true_peak_filter, AW_GAIN_TRUE_PEAK_CEILING,
// include/airwave_hip.h), shared by the true-peak kernel (truepeak_tile.hpp, truepeak_kernels.hip), the read-out in runtime.cpp and a CPU
// test that compiles this header with plain g++.
//
// The measurement taps the float32 output y BEFORE the gain, like the level meter.  Per ear, y is oversampled four times by a 49-tap
// Hann-windowed sinc (the libebur128 construction), whatever the sample rate:
//   h[j] = sinc((j - 24) / 4) * (0.5 - 0.5 cos(2 pi j / 48)),  j = 0 .. 48,
// formed in double on the host and rounded once to float32.  Phase 0 (j = 0, 4, ..) is the identity and is never computed; the phases
// p = 1, 2, 3 have twelve taps each, c[p][k] = h[p + 4k].  With v[i] = y[i] where y[i] is finite, else 0 (counted), and v[i] for i < 0
// the carried history (zero after a reset),
//   t_p[n] = fmaf(c[p][11], v[n-11], .. fmaf(c[p][1], v[n-1], c[p][0] * v[n]) ..)        float32, k = 0, 1, .., 11 in this order,
// and frame n contributes max(|v[n]|, |t_1[n]|, |t_2[n]|, |t_3[n]|), kept as the bit pattern of the absolute value (integer max, as
// levels.hpp does), so the true peak is never below the sample peak.  The six-frame lookahead of a centred filter is not flushed: the
// last frames of a call contribute their windows when later frames arrive.
//
// fmaf is correctly rounded on host and device and max commutes, so every field is a pure function of the stream's samples since the
// last reset: chunking by streams, sample formats, pinned or pageable buffers, sharding AND splitting calls in time change no bit.
#pragma once
#include <cmath>
#include <cstdint>

#include "pcm.hpp"

#if defined(__clang__)
#define AWTP_UNROLL _Pragma("unroll")
#else
#define AWTP_UNROLL
#endif

namespace awtp {

constexpr int kPhases = 3;               // the computed phases 1, 2, 3 of the 4x interpolator
constexpr int kTaps = 12;                // taps per phase
constexpr int kHistory = kTaps - 1;      // frames a stream carries from call to call
constexpr int kCoefficients = kPhases * kTaps;

// c[(p - 1) * 12 + k] = (float)h[p + 4k]
inline void filter(float (&c)[kCoefficients]) {
    for (int p = 1; p <= kPhases; ++p)
        for (int k = 0; k < kTaps; ++k) {
            const int j = p + 4 * k;
            const double x = M_PI * (double)(j - 24) / 4.0;           // (never 0: j - 24 is no multiple of 4)
            c[(p - 1) * kTaps + k] = (float)(std::sin(x) / x * (0.5 - 0.5 * std::cos(2.0 * M_PI * (double)j / 48.0)));
        }
}

AWP_HD uint32_t float_bits(float y) { uint32_t u; __builtin_memcpy(&u, &y, 4); return u; }
AWP_HD float bits_float(uint32_t u) { float y; __builtin_memcpy(&y, &u, 4); return y; }

// What enters the filter: y, or 0 for a NaN / inf y, which is counted.
AWP_HD float filter_input(float y, unsigned &nonfinite) {
    if ((float_bits(y) & 0x7F800000u) == 0x7F800000u) { nonfinite += 1; return 0.0f; }
    return y;
}

// One phase's interpolated value at frame n; w[k * stride] = v[n - k].
AWP_HD float phase_value(const float *c, const float *w, int stride) {
    float t = c[0] * w[0];
    AWTP_UNROLL
    for (int k = 1; k < kTaps; ++k) t = __builtin_fmaf(c[k], w[k * stride], t);
    return t;
}

// The contribution of frame n of one ear: the bits of max(|v[n]|, |t_1[n]|, |t_2[n]|, |t_3[n]|); w[k * stride] = v[n - k].
AWP_HD uint32_t frame_peak_bits(const float *c, const float *w, int stride) {
    uint32_t m = float_bits(w[0]) & 0x7FFFFFFFu;
    AWTP_UNROLL
    for (int p = 0; p < kPhases; ++p) {
        const uint32_t a = float_bits(phase_value(c + p * kTaps, w, stride)) & 0x7FFFFFFFu;
        m = a > m ? a : m;
    }
    return m;
}

// What a stream accumulates.
struct Record {
    uint32_t tp_bits[2];               // bits of the true peak per ear since the last reset
    uint32_t call_tp_bits;             // ... of the larger ear over the last call
    unsigned long long nonfinite;      // NaN / inf samples, both ears, that entered as 0
};

// The rule, frame by frame: y [frames][2] continues a stream whose last kHistory cleaned frames are hist [kHistory][2] (oldest first),
// which is carried on.  Adds to rec (call_tp_bits included: the caller zeroes it per call).
inline void sequential(const float *c, const float *y, long long frames, float *hist, Record &rec) {
    float w[2][kTaps];                   // w[e][k] = v[n - k]
    for (int e = 0; e < 2; ++e) {
        w[e][0] = 0.0f;
        for (int k = 1; k < kTaps; ++k) w[e][k] = hist[(kHistory - k) * 2 + e];
    }
    for (long long n = 0; n < frames; ++n)
        for (int e = 0; e < 2; ++e) {
            if (n > 0) for (int k = kTaps - 1; k > 0; --k) w[e][k] = w[e][k - 1];
            unsigned nf = 0;
            w[e][0] = filter_input(y[2 * n + e], nf);
            rec.nonfinite += nf;
            const uint32_t m = frame_peak_bits(c, w[e], 1);
            if (m > rec.tp_bits[e]) rec.tp_bits[e] = m;
            if (m > rec.call_tp_bits) rec.call_tp_bits = m;
        }
    if (frames > 0)
        for (int e = 0; e < 2; ++e)
            for (int k = 1; k < kTaps; ++k) hist[(kHistory - k) * 2 + e] = w[e][k - 1];
}

}  // namespace awtp
