// rateconv_kernels.hpp — host-callable launcher of the sample-rate converter's kernel (rateconv_kernels.hip; device code in
// rateconv_tile.hpp, rules in rateconv.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "rateconv_tile.hpp"

namespace awk {

// One call of p.in_frames input frames of p.n_streams streams: one workgroup per tile of p.tile output frames and stream (one per stream
// when the call produces nothing).  Writes p.out, p.hist_out and p.counts; reads p.in, p.hist_in and p.c.
hipError_t launch_rateconv(const RateconvParams &p, hipStream_t stream);
// The PCM form of the same call: p.in and p.out are byte buffers of p.in_format and p.out_format (awp::Format) at any byte alignment,
// and p.dither, p.gains, p.levels and p.clipped apply (rateconv.hpp, "integer PCM in and out").  Also adds to p.levels and *p.clipped.
hipError_t launch_rateconv_pcm(const RateconvParams &p, hipStream_t stream);
// The PCM form, measured (rateconv.hpp, "true peak of the converted output"): one workgroup per tile of tp.tile output frames.  Beside
// what launch_rateconv_pcm does it adds to tp.records and, when the call produces frames, writes tp.hist_out.
hipError_t launch_rateconv_pcm_tp(const RateconvParams &p, const RateconvTp &tp, hipStream_t stream);
// The measurement alone: p.hist_out, p.counts, tp.records and tp.hist_out as above; p.out, p.levels and p.clipped are not touched.
hipError_t launch_rateconv_tp_measure(const RateconvParams &p, const RateconvTp &tp, hipStream_t stream);

}  // namespace awk
