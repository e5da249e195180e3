// loudness.hpp — rules of the per-stream integrated loudness of the batch entries (ITU-R BS.1770-4; aw_stream_loudness,
// aw_spatializer_set_loudness / _get_loudness / _get_loudness_hops, aw_loudness_gain, include/airwave_hip.h), shared by the loudness kernels
// (loudness_scan.hpp, loudness_kernels.hip), the read-out in runtime.cpp and a CPU test that compiles this header with plain g++.
//
// The measurement taps the float32 output y BEFORE the gain, like the level meter.  Per ear, y runs through the two K-weighting biquads
// in Float64 (transposed direct form II, the recurrence of eq_cascade.hpp); the device keeps one number per stream and 100 ms hop,
//   E[s][h] = sum over the frames of hop h of (k_L^2 + k_R^2)        (both ears: channel weight 1),
// and everything after that — 400 ms blocks at 75 % overlap, the absolute and the relative gate — is a pure function of the hop energies
// that runs on the host at read-out (gate, below).  True peak, momentary / short-term loudness and LRA are not computed; the hop energies
// are what a host needs for the latter three.
#pragma once
#include <cmath>
#include <cstdint>

#include "pcm.hpp"

namespace awlo {

// ---- K-weighting --------------------------------------------------------------------------------------------------------------------
// The analog prototypes behind the BS.1770 table (which is given for 48 kHz only), through the bilinear transform with K = tan(pi f0 / fs).
// At 48 kHz this reproduces the twelve table values to 1e-15.
constexpr double kShelfF0 = 1681.974450955533, kShelfGainDb = 3.999843853973347, kShelfQ = 0.7071752369554196, kShelfBandExp = 0.4996667741545416;
constexpr double kHighpassF0 = 38.13547087602444, kHighpassQ = 0.5003270373238773;
constexpr int kFilters = 2;              // shelf, then high-pass
constexpr double kOffsetLufs = -0.691, kAbsoluteGateLufs = -70.0, kRelativeGateLu = -10.0;
constexpr int kHopsPerBlock = 4;         // 400 ms blocks of 100 ms hops: 75 % overlap
constexpr int kHopsPerSecond = 10;

// c[filter] = b0 b1 b2 a1 a2, normalised by a0 (the layout of the EQ tables' first five entries)
inline void k_weighting(double fs, double (&c)[kFilters][5]) {
    {
        const double K = std::tan(M_PI * kShelfF0 / fs), Vh = std::pow(10.0, kShelfGainDb / 20.0), Vb = std::pow(Vh, kShelfBandExp);
        const double a0 = 1.0 + K / kShelfQ + K * K;
        c[0][0] = (Vh + Vb * K / kShelfQ + K * K) / a0;
        c[0][1] = 2.0 * (K * K - Vh) / a0;
        c[0][2] = (Vh - Vb * K / kShelfQ + K * K) / a0;
        c[0][3] = 2.0 * (K * K - 1.0) / a0;
        c[0][4] = (1.0 - K / kShelfQ + K * K) / a0;
    }
    {
        const double K = std::tan(M_PI * kHighpassF0 / fs);
        const double a0 = 1.0 + K / kHighpassQ + K * K;
        c[1][0] = 1.0; c[1][1] = -2.0; c[1][2] = 1.0;
        c[1][3] = 2.0 * (K * K - 1.0) / a0;
        c[1][4] = (1.0 - K / kHighpassQ + K * K) / a0;
    }
}

// Frames per hop of a sample rate, or 0 where the rate is not a finite positive multiple of 10 Hz (no whole number of frames makes 100 ms).
inline long long hop_frames(double fs) {
    if (!std::isfinite(fs) || !(fs > 0.0) || fs > 1e12) return 0;
    const double h = fs / kHopsPerSecond;
    return h == std::floor(h) ? (long long)h : 0;
}

// ---- per sample ---------------------------------------------------------------------------------------------------------------------
// What enters the filter: y, or 0 for a NaN / inf y, which is counted — one bad sample does not poison the recurrence for good.
AWP_HD double filter_input(float y, unsigned &nonfinite) {
    uint32_t u;
    __builtin_memcpy(&u, &y, 4);
    if ((u & 0x7F800000u) == 0x7F800000u) { nonfinite += 1; return 0.0; }
    return (double)y;
}

// ---- gating -------------------------------------------------------------------------------------------------------------------------
struct Gated {
    double integrated_lufs, relative_threshold_lufs;     // -INFINITY where no block is left to average
    uint32_t blocks, blocks_above_absolute, blocks_gated;
};

inline double lufs_of(double mean_square) { return kOffsetLufs + 10.0 * std::log10(mean_square); }

// Block j covers the complete hops j .. j+3: z_j = (E[j] + .. + E[j+3]) / (4 hop), l_j = -0.691 + 10 log10 z_j.  The absolute gate keeps
// l_j > -70; the relative threshold is the loudness of the mean of z over those blocks, less 10; the integrated loudness is the loudness
// of the mean of z over the blocks above both.
inline Gated gate(const double *e, long long n_hops, long long hop) {
    Gated g{-INFINITY, -INFINITY, 0, 0, 0};
    if (n_hops < kHopsPerBlock) return g;
    const long long nb = n_hops - (kHopsPerBlock - 1);
    const double scale = (double)kHopsPerBlock * (double)hop;
    auto z = [&](long long j) { return (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / scale; };
    g.blocks = (uint32_t)nb;
    double sum = 0.0;
    long long n = 0;
    for (long long j = 0; j < nb; ++j) {
        const double zj = z(j);
        if (lufs_of(zj) > kAbsoluteGateLufs) { sum += zj; n += 1; }
    }
    g.blocks_above_absolute = (uint32_t)n;
    if (n == 0) return g;
    g.relative_threshold_lufs = lufs_of(sum / (double)n) + kRelativeGateLu;
    sum = 0.0; n = 0;
    for (long long j = 0; j < nb; ++j) {
        const double zj = z(j), l = lufs_of(zj);
        if (l > kAbsoluteGateLufs && l > g.relative_threshold_lufs) { sum += zj; n += 1; }
    }
    g.blocks_gated = (uint32_t)n;
    if (n > 0) g.integrated_lufs = lufs_of(sum / (double)n);
    return g;
}

// The gain that brings a measured loudness to a target: 10^((target - lufs) / 20) as float32.  False (no gain) for a non-finite loudness
// or target — a silent stream measures -INFINITY and must not produce an infinite gain — and where the gain is no finite float32.
inline bool gain_to_target(double lufs, double target_lufs, float *gain) {
    if (!std::isfinite(lufs) || !std::isfinite(target_lufs)) return false;
    const float g = (float)std::pow(10.0, (target_lufs - lufs) / 20.0);
    if (!std::isfinite(g)) return false;
    *gain = g;
    return true;
}

}  // namespace awlo
