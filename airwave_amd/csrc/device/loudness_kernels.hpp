// loudness_kernels.hpp — host-callable launcher of the K-weighted hop-energy kernels (loudness_kernels.hip; device code in
// loudness_scan.hpp, rules in loudness.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "loudness_scan.hpp"

namespace awk {

hipError_t prepare_loudness_kernels();     // dynamic-LDS attribute of the scan kernel (more than 64 KB); once per context
// p.frames frames of n_streams streams from p.in on (p.stride_frames apart), continuing at p.frame0 frames since the last reset: the
// chunk-parallel kernel over the whole chunks, the sequential one over the < kEqChunk frame tail (and over everything where a hop is
// shorter than a chunk).  Adds into p.hops / p.nonfinite and carries p.z.  Reads 8 bytes per frame, stores nothing per frame.
hipError_t launch_loudness(const LoudnessParams &p, int n_streams, hipStream_t stream);

}  // namespace awk
