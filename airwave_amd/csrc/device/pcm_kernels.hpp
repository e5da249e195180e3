// pcm_kernels.hpp — host-callable launchers of the PCM decode / encode kernels (pcm_kernels.hip; element rules: pcm.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace awk {

// n elements of format fmt (awp::kS16 / kS24 / kS32) at src, any byte alignment -> n floats at dst (4-byte aligned).
hipError_t launch_pcm_decode(int fmt, const void *src, float *dst, int64_t n, hipStream_t stream);
// n floats at src (4-byte aligned) -> n elements of format fmt at dst, any byte alignment.  clipped: NULL, or a device counter that
// the launch atomically adds its clipped-sample count to (one add per wave that clipped).
hipError_t launch_pcm_encode(int fmt, const float *src, void *dst, int64_t n, unsigned long long *clipped, hipStream_t stream);

// The dither of an encode launch (aw_spatializer_set_dither; rules: pcm.hpp): the launch's n samples are whole streams of 2 * frames
// samples, the first of them global stream first_stream, and the call they belong to began at frame position `position`.
struct PcmDither {
    int mode;                       // awp::kDitherTpdf / kDitherTpdfHp
    uint64_t seed, first_stream, position;
    int64_t frames;
};
// launch_pcm_encode with dither, for fmt awp::kS16 / kS24 (anything else, or n not a whole number of streams: hipErrorInvalidValue).
hipError_t launch_pcm_encode_dithered(int fmt, const PcmDither &dither, const float *src, void *dst, int64_t n, unsigned long long *clipped,
                                      hipStream_t stream);

}  // namespace awk
