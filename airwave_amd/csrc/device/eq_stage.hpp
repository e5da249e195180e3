// eq_stage.hpp — the records of the batch entries' equalizer stage (aw_spatializer_set_equalizer): ONE preset per stream.  Plain structs,
// no HIP and no pragmas: shared by the kernels (eq_cascade.hpp), the stage's layout (host/stage_records.hpp) and the runtime.
//
// Rule: a stream whose map entry is p >= 0 goes through ParametricEqualizerState.process of preset p (ParametricEqualizerProcessor.swift:
// 58-91: preamp, the enabled biquads in Float64, one rounding to float32) in place on the convolution's float32 output, its Float64 state
// carried from call to call; a stream whose entry is -1 is not touched.  The state is [stream][kmax][4] doubles, kmax = the largest
// enabled-filter count among the presets: a stream uses the first n_filters rows of its own.
#pragma once

namespace awk {

// One per preset, read by a workgroup through its stream's map entry.  Offsets count doubles from the start of the stage's tables.
struct EqStagePreset {
    double preamp;            // 10^(dB/20)
    long long tab_off;        // [n_filters][kEqTabDoubles]  (EqTables::tab)
    long long plane_off;      // [n_filters][64][4]          (EqTables::plane)
    int n_filters, reserved;
};
static_assert(sizeof(EqStagePreset) == 32, "EqStagePreset");

// A target change (aw_spatializer_set_equalizer_target) fades over T = max(1, round(0.020 * rate)) frames on ONE clock per handle.  While it
// runs, a stream whose target entry is not kEqKeep is a fading stream: its active preset goes on from its state (-1: the sample itself), its
// target preset starts from a zeroed state of its own in a second bank (-1: the sample itself), both renderings are rounded to float32 and
// frame i of the fade (counted from 1) is Float(fma(Double(old), 1 - g, Double(new) * g)), g = i / T: aw_eq_blend_kernel's arithmetic.  When the clock
// reaches T the target entry and the second bank's rows become the stream's active ones.  The presets of both sides lie in the stage's one
// table: the setter rebuilds it from the presets still in use and the new ones.
constexpr int kEqKeep = -2;   // AW_EQ_KEEP: the stream is not part of the change

}  // namespace awk
