// truepeak_kernels.hpp — host-callable launcher of the true-peak kernel (truepeak_kernels.hip; device code in truepeak_tile.hpp, rules in
// truepeak.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "truepeak_tile.hpp"

namespace awk {

hipError_t prepare_truepeak_kernels();     // once per context
// p.frames frames of p.n_streams streams from p.in on: one workgroup per tile of kTpTile frames and stream.  Raises p.tp_bits / p.call_tp,
// adds to p.nonfinite, reads p.hist_in and writes p.hist_out.  Reads 8 bytes per frame, stores nothing per frame.
hipError_t launch_truepeak(const TruePeakParams &p, hipStream_t stream);

}  // namespace awk
