// limiter_kernels.hpp — host-callable launcher of the limiter kernel (limiter_kernels.hip; device code in limiter_tile.hpp, rules in
// limiter.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "limiter_tile.hpp"

namespace awk {

hipError_t prepare_limiter_kernels();      // once per context
// p.frames frames of p.n_streams streams from p.in to p.out (another buffer): one workgroup per tile of kLimTile frames and stream.
// Lowers p.min_gain, adds to p.limited / p.nonfinite, reads p.hist_in and writes p.hist_out.  Reads 8 and stores 8 bytes per frame.
hipError_t launch_limiter(const LimiterParams &p, hipStream_t stream);

}  // namespace awk
