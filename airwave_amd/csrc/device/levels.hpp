// levels.hpp — rules of the per-stream level meter and output gain of the batch entries (aw_stream_levels, aw_spatializer_set_metering /
// _set_gain, include/airwave_hip.h), shared by the levels / scale / gained encode kernels (pcm_kernels.hip), the single-stream host path
// (runtime.cpp) and a CPU test that compiles this header with plain g++.
//
// The meter sees every float32 output sample y BEFORE the gain; the gain multiplies y once, in float32, and the encode of pcm.hpp then
// sees the product.  Peaks are kept as the bit pattern of |y|: non-negative floats order as their bits do, so an integer max serves
// (denormals and -0 included, whatever the float mode) and the device can use an unsigned atomic max.
#pragma once
#include <cstdint>

#include "pcm.hpp"

namespace awl {

enum GainMode : int { kGainNone = 0, kGainFixed = 1, kGainPeakCeiling = 2 };

// What a handle accumulates per stream on the device (the host adds frames and the gain: aw_spatializer_get_levels).
struct Record {
    uint32_t peak_bits[2];             // bits of max |y| per ear over finite samples
    double energy[2];                  // sum of y^2 per ear over finite samples
    unsigned long long clipped;        // samples the integer encodes clipped
    unsigned long long nonfinite;      // NaN / inf samples, both ears
};

AWP_HD uint32_t float_bits(float y) { uint32_t u; __builtin_memcpy(&u, &y, 4); return u; }
AWP_HD float bits_float(uint32_t u) { float y; __builtin_memcpy(&y, &u, 4); return y; }
AWP_HD bool finite_bits(uint32_t u) { return (u & 0x7F800000u) != 0x7F800000u; }

// One sample's contribution: a non-finite y counts in nonfinite and in nothing else; otherwise peak = max(peak, |y|) and
// energy += (double)y * (double)y (the product of two float32 values is exact in double; only the order of the additions is free).
AWP_HD void contribute(float y, uint32_t &peak_bits, double &energy, unsigned &nonfinite) {
    const uint32_t u = float_bits(y);
    if (!finite_bits(u)) { nonfinite += 1; return; }
    const uint32_t a = u & 0x7FFFFFFFu;
    if (a > peak_bits) peak_bits = a;
    energy += (double)y * (double)y;
}

// The gained sample: the float32 product, one rounding.  The encode multiplies it by a power of two (exact), so whether the compiler
// contracts that scale multiply and the dither add into an FMA cannot change the result (pcm.hpp), and y * g itself feeds a multiply,
// not an add: there is nothing to fuse it with.
AWP_HD float apply_gain(float y, float g) { return y * g; }

// The automatic gain of a stream whose call-local peak (the larger ear, finite samples only) is p, under ceiling c: c / p correctly
// rounded to float32 where p exceeds c, else 1.  The double quotient of two float32 values rounds to the float32 quotient exactly
// (53 >= 2 * 24 + 2 bits: no double rounding); no reciprocal.
AWP_HD float auto_gain(float p, float c) { return p > c ? (float)((double)c / (double)p) : 1.0f; }

// encode_dithered_at (pcm.hpp) of the gained sample; float32 output stores the product itself.
AWP_HD void encode_gained_at(int fmt, int mode, float y, float g, uint64_t key, uint64_t p, int ear, unsigned char *out, unsigned *clip) {
    awp::encode_dithered_at(fmt, mode, apply_gain(y, g), key, p, ear, out, clip);
}

}  // namespace awl
