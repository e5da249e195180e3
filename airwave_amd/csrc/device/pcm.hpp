// pcm.hpp — element rules of the integer PCM sample formats (aw_sample_format, include/airwave_hip.h), shared by the decode / encode
// kernels (pcm_kernels.hip), the single-stream host path (runtime.cpp) and a CPU test that compiles this header with plain g++.
//
// Decode is aw_wav_load's rule (host/host_api.cpp): s / 2^15, s / 2^23, s / 2^31.  Every scale is a power of two, so the product
// with 0x1p-15f (and so on) is the same float; for s32, (float)s rounds to nearest-even exactly as (float)((double)s / 2^31) does.
// Encode is the inverse scale, rounded to nearest with ties to even, then saturated; s32 is computed in double.  NaN encodes to 0.
// A sample is clipped when the rounded value lies outside the integer range, or when it is NaN or +-inf.
// Dither (s16 and s24 only; the rules are at the end of this file) adds a value in (-1, 1) LSB before the rounding.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define AWP_HD __host__ __device__ __forceinline__
#else
#define AWP_HD inline
#endif

namespace awp {

enum Format : int { kF32 = 0, kS16 = 1, kS24 = 2, kS32 = 3 };

AWP_HD int format_bytes(int f) { return f == kF32 || f == kS32 ? 4 : f == kS16 ? 2 : f == kS24 ? 3 : 0; }

AWP_HD float decode_s16(int32_t s) { return (float)s * 0x1p-15f; }
// b0..b2: the three little-endian bytes of a packed s24 sample
AWP_HD float decode_s24(uint32_t b0, uint32_t b1, uint32_t b2) {
    const int32_t s = (int32_t)((b0 | (b1 << 8) | (b2 << 16)) << 8) >> 8;     // sign-extend bit 23
    return (float)s * 0x1p-23f;
}
AWP_HD float decode_s32(int32_t s) { return (float)s * 0x1p-31f; }

// Returns the integer sample; *clip is set to 1 when the sample clipped (left untouched otherwise).
AWP_HD int32_t encode_s16(float x, unsigned *clip) {
    const float v = rintf(x * 32768.0f);
    if (v >= -32768.0f && v <= 32767.0f) return (int32_t)v;
    *clip = 1;
    return v > 0.0f ? 32767 : v < 0.0f ? -32768 : 0;                         // (NaN: neither)
}
AWP_HD int32_t encode_s24(float x, unsigned *clip) {
    const float v = rintf(x * 8388608.0f);
    if (v >= -8388608.0f && v <= 8388607.0f) return (int32_t)v;
    *clip = 1;
    return v > 0.0f ? 8388607 : v < 0.0f ? -8388608 : 0;
}
AWP_HD int32_t encode_s32(float x, unsigned *clip) {
    const double v = rint((double)x * 2147483648.0);
    if (v >= -2147483648.0 && v <= 2147483647.0) return (int32_t)v;
    *clip = 1;
    return v > 0.0 ? 2147483647 : v < 0.0 ? (int32_t)(-2147483647 - 1) : 0;
}

// One element at byte address p (any alignment), for the host path and the kernels' unaligned heads and tails.
AWP_HD float decode_at(int fmt, const unsigned char *p) {
    switch (fmt) {
        case kS16: return decode_s16((int16_t)(uint16_t)(p[0] | (p[1] << 8)));
        case kS24: return decode_s24(p[0], p[1], p[2]);
        case kS32: return decode_s32((int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)));
        default: {
            const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            float f;
            __builtin_memcpy(&f, &u, 4);
            return f;
        }
    }
}
AWP_HD void encode_at(int fmt, float x, unsigned char *p, unsigned *clip) {
    uint32_t u;
    switch (fmt) {
        case kS16: u = (uint32_t)encode_s16(x, clip); break;
        case kS24: u = (uint32_t)encode_s24(x, clip); break;
        case kS32: u = (uint32_t)encode_s32(x, clip); break;
        default: __builtin_memcpy(&u, &x, 4); break;
    }
    const int n = format_bytes(fmt);
    for (int i = 0; i < n; ++i) p[i] = (unsigned char)(u >> (8 * i));
}

// ---- dither of the s16 / s24 encode (aw_dither, aw_spatializer_set_dither) -------------------------------------------------------------
// Stateless: the noise of output sample (stream g, frame p, ear) is a hash of its coordinates, where g is the global stream index and p
// the frame's absolute position since create / reset.  Chunking a call by streams or splitting it in time therefore changes no bit.
enum Dither : int { kDitherNone = 0, kDitherTpdf = 1, kDitherTpdfHp = 2 };

// The splitmix64 finaliser (also aw_synth_fill's generator).
AWP_HD uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// K of global stream g; the salt keeps the dither independent of aw_synth_fill input made with the same seed
AWP_HD uint64_t dither_key(uint64_t seed, uint64_t g) { return ((seed ^ 0xD1B54A32D192ED03ull) + g) * 0x9E3779B97F4A7C15ull; }

// TPDF from h = splitmix64(K + 2p + ear): the difference of two 24-bit uniforms, in LSB (-1, 1).  Exact in float.
AWP_HD float tpdf_from_hash(uint64_t h) { return (float)((int32_t)(h >> 40) - (int32_t)((h >> 16) & 0xFFFFFFu)) * 0x1p-24f; }
// High-pass TPDF from h_p = splitmix64(K + p) and h_prev = splitmix64(K + p - 1): r(p, ear) - r(p - 1, ear), where r takes bits 40..63
// (left ear) or 16..39 (right ear) of the frame's hash as a uniform in [0, 1).  The integer difference scaled by 2^-24 is the float
// difference r(p) - r(p - 1) exactly.
AWP_HD float tpdf_hp_from_hashes(uint64_t h_p, uint64_t h_prev, int ear) {
    const int sh = ear ? 16 : 40;
    return (float)((int32_t)((h_p >> sh) & 0xFFFFFFu) - (int32_t)((h_prev >> sh) & 0xFFFFFFu)) * 0x1p-24f;
}
// The dither value in LSB of (key, frame position p, ear) under mode; p - 1 wraps mod 2^64 at p = 0.
AWP_HD float dither_value(int mode, uint64_t key, uint64_t p, int ear) {
    if (mode == kDitherTpdf) return tpdf_from_hash(splitmix64(key + 2 * p + (uint64_t)ear));
    if (mode == kDitherTpdfHp) return tpdf_hp_from_hashes(splitmix64(key + p), splitmix64(key + p - 1), ear);
    return 0.0f;
}

// encode_s16 / encode_s24 with d LSB of dither added before the rounding; saturation, the NaN rule and the clip rule are theirs (a sample
// that the dither pushes past full scale counts as clipped).  The scale is a power of two, so x * scale is exact and contraction into an
// FMA cannot change the sum.
AWP_HD int32_t encode_s16_dithered(float x, float d, unsigned *clip) {
    const float v = rintf(x * 32768.0f + d);
    if (v >= -32768.0f && v <= 32767.0f) return (int32_t)v;
    *clip = 1;
    return v > 0.0f ? 32767 : v < 0.0f ? -32768 : 0;
}
AWP_HD int32_t encode_s24_dithered(float x, float d, unsigned *clip) {
    const float v = rintf(x * 8388608.0f + d);
    if (v >= -8388608.0f && v <= 8388607.0f) return (int32_t)v;
    *clip = 1;
    return v > 0.0f ? 8388607 : v < 0.0f ? -8388608 : 0;
}

// encode_at under a dither mode, for the host path and the kernels' edge elements: s16 and s24 are dithered with the value of (key, p,
// ear); s32, f32 and kDitherNone are encode_at itself.
AWP_HD void encode_dithered_at(int fmt, int mode, float x, uint64_t key, uint64_t p, int ear, unsigned char *out, unsigned *clip) {
    if (mode == kDitherNone || (fmt != kS16 && fmt != kS24)) { encode_at(fmt, x, out, clip); return; }
    const float d = dither_value(mode, key, p, ear);
    const uint32_t u = fmt == kS16 ? (uint32_t)encode_s16_dithered(x, d, clip) : (uint32_t)encode_s24_dithered(x, d, clip);
    const int n = format_bytes(fmt);
    for (int i = 0; i < n; ++i) out[i] = (unsigned char)(u >> (8 * i));
}

}  // namespace awp
