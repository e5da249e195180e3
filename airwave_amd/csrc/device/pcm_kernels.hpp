// pcm_kernels.hpp — host-callable launchers of the PCM kernels (pcm_kernels.hip; element rules: pcm.hpp): decode, the one encode
// launcher (plain, dithered, gained / metered), levels and scale.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "levels.hpp"

namespace awk {

// n elements of format fmt (awp::kS16 / kS24 / kS32) at src, any byte alignment -> n floats at dst (4-byte aligned).
hipError_t launch_pcm_decode(int fmt, const void *src, float *dst, int64_t n, hipStream_t stream);
// The dither of an encode launch (aw_spatializer_set_dither; rules: pcm.hpp): the launch's n samples are whole streams of 2 * frames
// samples, the first of them global stream first_stream, and the call they belong to began at frame position `position`.
struct PcmDither {
    int mode;                       // awp::kDitherTpdf / kDitherTpdfHp; awp::kDitherNone only beside a PcmGain
    uint64_t seed, first_stream, position;
    int64_t frames;
};
// Levels and gain (aw_spatializer_set_metering / _set_gain; rules: levels.hpp).  Every launch covers whole streams of 2 * frames
// samples; the pointers below are device pointers at the entry of the launch's first stream.
struct PcmGain {
    int mode;                       // awl::kGainNone (every gain 1: a metered encode), kGainFixed, kGainPeakCeiling
    float ceiling;                  // kGainPeakCeiling
    const float *gain;              // kGainFixed: one gain per stream
    const uint32_t *call_peak;      // kGainPeakCeiling: the bits of each stream's peak over this call, as launch_levels left them
    awl::Record *rec;               // NULL, or the streams' records: the encode adds each stream's clipped samples to its record
};
// n floats at src (4-byte aligned) -> n elements of format fmt at dst, any byte alignment.  clipped: NULL, or a device counter that the
// launch atomically adds its clipped-sample count to (one add per wave that clipped).  dither and gain NULL: the plain encode.  dither
// only: the dithered encode, for fmt awp::kS16 / kS24 (anything else, or n not a whole number of streams: hipErrorInvalidValue).  gain
// (with dither, whose frames it shares; dither->mode may be awp::kDitherNone, and s32 ignores it): src[i] * gain of i's stream.
hipError_t launch_pcm_encode(int fmt, const float *src, void *dst, int64_t n, unsigned long long *clipped, const PcmDither *dither,
                             const PcmGain *gain, hipStream_t stream);
// Adds peak, energy and non-finite count of every stream of the n floats at src (4-byte aligned) to rec (NULL: not wanted), and
// raises call_peak[s] (zeroed by the caller at the start of the call) to the bits of stream s's larger ear peak.
hipError_t launch_levels(const float *src, int64_t n, int64_t frames, awl::Record *rec, uint32_t *call_peak, hipStream_t stream);
// buf[i] *= gain of i's stream, in place (4-byte aligned).
hipError_t launch_scale(float *buf, int64_t n, int64_t frames, const PcmGain &gain, hipStream_t stream);

}  // namespace awk
