// limiter.hpp — rules of the look-ahead true-peak limiter of the batch entries (aw_stream_limiter, aw_spatializer_set_limiter /
// _get_limiter, include/airwave_hip.h), shared by the limiter kernel (limiter_tile.hpp, limiter_kernels.hip), the single-stream
// page-locked path in runtime.cpp and a CPU test that compiles this header with plain g++.
//
// Per stream, stereo-linked; n is the frame index since the last reset, c the ceiling, L the attack = release frames, H the hold frames,
// g_s the stream's pre-gain (the AW_GAIN_FIXED gain, or 1), W = L + 12 + H, D = L + 11:
//   1. u[n][e] = (float)(y[n][e] * g_s); the detector sees v = u where finite, else 0 (counted, awtp::filter_input);
//   2. p[n] = the larger ear of awtp::frame_peak_bits over v (truepeak.hpp: the same 36 coefficients, the same fmaf order);
//   3. r[n] = awl::auto_gain(p[n], c), 1 for n < 0; q[n] = (uint32_t)floor((double)r[n] * 2^30);
//   4. m[n] = min(q[n], .., q[n - (W - 1)]);
//   5. S[n] = m[n] + .. + m[n - (L - 1)] in uint64_t (exact, whatever the order: this is why the rule is in fixed point),
//      g[n] = (float)((double)S[n] / ((double)L * 2^30));
//   6. z[n][e] = (float)(u[n - D][e] * g[n]), u = 0 before the stream's first frame.
// floor, the integer mean, the double division and the float rounding are monotone, so g[n] <= r[k] for every detector frame k in
// [n - D - H, n - D + 11]: the gain is down to what every window that touches the delayed frame asks for, and flat over the twelve
// frames of an isolated peak's window.
//
// What a stream carries from call to call is the last halo(L, H) = W + L - 2 + 11 frames of the RAW u (not cleaned: u[n - D] goes to
// the output as it is, and cleaning it again for the detector costs a compare), oldest first, zero after a reset: p of silence is 0,
// r is 1 and q is 2^30, which is what steps 3 and 6 ask for before the first frame.  Every field is a pure function of the stream's
// samples since the last reset: chunking, sample formats, sharding and splitting calls in time change no bit.
#pragma once
#include <cstdint>
#include <vector>

#include "levels.hpp"
#include "truepeak.hpp"

namespace awlim {

constexpr int kMinAttack = 16, kMaxAttack = 512, kMaxHold = 1024;
constexpr uint32_t kOne = 1u << 30;                      // q of a gain of 1
constexpr uint32_t kOneBits = 0x3F800000u;               // the bits of 1.0f: a record's min_gain before anything was limited

AWP_HD int window(int L, int H) { return L + awtp::kTaps + H; }                    // W
AWP_HD int delay(int L) { return L + awtp::kHistory; }                              // D
AWP_HD int q_halo(int L, int H) { return window(L, H) + L - 2; }                    // frames of q in front of the first output frame
AWP_HD int halo(int L, int H) { return q_halo(L, H) + awtp::kHistory; }             // frames of u carried from call to call
constexpr int kMaxHalo = kMaxAttack + awtp::kTaps + kMaxHold + kMaxAttack - 2 + awtp::kHistory;      // 2069

AWP_HD bool config_ok(int L, int H, float c) { return L >= kMinAttack && L <= kMaxAttack && H >= 0 && H <= kMaxHold && c > 0.0f && c <= 1.0f; }

// step 3: the detector's bits (non-negative, finite) -> q.  r lies in (0, 1], so the truncation is the floor and q <= 2^30.
AWP_HD uint32_t required_q(uint32_t p_bits, float c) {
    return (uint32_t)((double)awl::auto_gain(awl::bits_float(p_bits), c) * 1073741824.0);
}
// step 5
AWP_HD float ramp_gain(uint64_t S, int L) { return (float)((double)S / ((double)L * 1073741824.0)); }
// steps 1 and 6: one float32 product each (nothing to fuse them with: levels.hpp)
AWP_HD float pre_gain(float y, float g_s) { return awl::apply_gain(y, g_s); }
AWP_HD float limit(float u_delayed, float g) { return u_delayed * g; }

// What a stream accumulates (the host adds the frames: aw_spatializer_get_limiter).  g lies in [0, 1], so its bits order as it does
// and the device can use an unsigned atomic min.
struct Record {
    uint32_t min_gain_bits = kOneBits;
    unsigned long long limited_frames = 0;     // output frames with g < 1
    unsigned long long nonfinite = 0;          // NaN / inf samples of u, both ears, that entered the detector as 0
};

// Step 2 over an image of raw u: the bits of p of the frame whose ear-0 sample is at u2 (u2[-2 k + e] is ear e of the frame k before).
AWP_HD uint32_t detector_bits(const float *c, const float *u2) {
    uint32_t p = 0;
    for (int e = 0; e < 2; ++e) {
        float w[awtp::kTaps];
        unsigned ignored = 0;
        for (int k = 0; k < awtp::kTaps; ++k) w[k] = awtp::filter_input(u2[e - 2 * k], ignored);
        const uint32_t m = awtp::frame_peak_bits(c, w, 1);
        p = m > p ? m : p;
    }
    return p;
}

// The rule, frame by frame: y [frames][2] continues a stream whose last halo(L, H) frames of raw u are hist [halo][2] (oldest first),
// which is carried on.  z [frames][2] may be y itself.  c36: awtp::filter.  Adds to rec.  g_out / p_out (optional, [frames]): the gain
// applied to each output frame and the detector's bits of each input frame.
inline void sequential(const float *c36, int L, int H, float ceiling, float g_s, const float *y, long long frames, float *hist, float *z,
                       Record &rec, float *g_out = nullptr, uint32_t *p_out = nullptr) {
    if (frames <= 0) return;
    const long long HL = halo(L, H), QH = q_halo(L, H), W = window(L, H), D = delay(L);
    std::vector<float> u((size_t)(HL + frames) * 2);                // frame n of the call is u[HL + n]
    for (long long i = 0; i < HL * 2; ++i) u[(size_t)i] = hist[i];
    for (long long i = 0; i < frames * 2; ++i) {
        const float x = pre_gain(y[i], g_s);
        unsigned nf = 0;
        (void)awtp::filter_input(x, nf);
        rec.nonfinite += nf;
        u[(size_t)(HL * 2 + i)] = x;
    }
    std::vector<uint32_t> q((size_t)(QH + frames)), m((size_t)(L - 1 + frames));      // q[QH + n], m[L - 1 + n]
    for (long long i = 0; i < QH + frames; ++i) {
        const uint32_t p = detector_bits(c36, &u[(size_t)(i + awtp::kHistory) * 2]);
        q[(size_t)i] = required_q(p, ceiling);
        if (p_out && i >= QH) p_out[i - QH] = p;
    }
    for (long long i = 0; i < L - 1 + frames; ++i) {                // m[i] is frame i - (L - 1): q index i + W - 1 down to i
        uint32_t v = q[(size_t)i];
        for (long long k = 1; k < W; ++k) v = q[(size_t)(i + k)] < v ? q[(size_t)(i + k)] : v;
        m[(size_t)i] = v;
    }
    for (long long n = 0; n < frames; ++n) {
        uint64_t S = 0;
        for (long long k = 0; k < L; ++k) S += m[(size_t)(n + k)];
        const float g = ramp_gain(S, L);
        const uint32_t gb = awl::float_bits(g);
        if (gb < rec.min_gain_bits) rec.min_gain_bits = gb;
        if (gb < kOneBits) rec.limited_frames += 1;
        if (g_out) g_out[n] = g;
        for (int e = 0; e < 2; ++e) z[2 * n + e] = limit(u[(size_t)(HL + n - D) * 2 + e], g);
    }
    for (long long i = 0; i < HL * 2; ++i) hist[i] = u[(size_t)(frames * 2 + i)];
}

}  // namespace awlim
