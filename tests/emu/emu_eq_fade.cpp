// emu_eq_fade.cpp — TEST-ONLY: the device functions of a target change of the equalizer stage (airwave_amd/csrc/device/eq_cascade.hpp:
// eq_stage_fade_stream / eq_stage_fade_sequential, the code hipcc compiles) under the CPU thread emulation of emu_ctx.hpp, one segment of a
// call at a time: emulated workgroups of kEqThreads per stream (or per stream and ear) for the chunk-aligned part, the sequential form for
// the rest — the split the runtime makes.  The cuts come from the runtime's own planner (host/eq_fade_plan.hpp).  The presets are prepared
// as emu_eq_stage.cpp prepares them; this unit takes that one in whole, so the plain stage is here to compare with.
#include "emu_eq_stage.cpp"

#include "../../airwave_amd/csrc/host/eq_fade_plan.hpp"

extern "C" {

// One segment.  y: the segment's first frame of stream 0, streams `stride` frames apart, processed in place; z / z_to: [stream][kmax][4];
// map / to_map: [stream].  fade = 0: the plain stage over the segment (to_map is not looked at).
int emu_eq_fade_segment(float *y, long long stride, double *z, double *z_to, const int *map, const int *to_map, int n_streams, long long frames,
                        long long t0, long long length, int fade, double sample_rate, const double *preamps_db, const int *counts, const double *filters,
                        int n_presets, int kmax, int ear_split) {
    using namespace awk;
    Prepared pr;
    const int rc = prepare(sample_rate, preamps_db, counts, filters, n_presets, pr);
    if (rc) return rc;
    if (kmax != pr.kmax) return -100;
    EqFadeParams f{};
    EqStageParams &p = f.s;
    p.z = z; p.map = map; p.presets = pr.headers.data(); p.tables = pr.tables.data();
    p.stride_frames = stride; p.kmax = kmax;
    f.z_to = z_to; f.to_map = to_map; f.length = length;
    const long long body = frames - frames % kEqChunk;
    if (body > 0) {
        p.y = y; p.frames = body; f.t0 = t0;
        EmuShared sh(kEqThreads, (size_t)kEqFadeLdsBytes / sizeof(cf));
        for (int s = 0; s < n_streams; ++s)
            for (int ear = 0; ear < (ear_split ? 2 : 1); ++ear)
                emu_workgroup(kEqThreads, [&](int t) {
                    EmuCtx ctx{t, &sh};
                    if (!fade) {
                        if (ear_split) eq_stage_stream<EmuCtx, 1>(ctx, p, p.map, p.presets, p.tables, s, ear);
                        else eq_stage_stream<EmuCtx, 2>(ctx, p, p.map, p.presets, p.tables, s, 0);
                    } else if (ear_split) eq_stage_fade_stream<EmuCtx, 1>(ctx, f, p.map, f.to_map, p.presets, p.tables, s, ear);
                    else eq_stage_fade_stream<EmuCtx, 2>(ctx, f, p.map, f.to_map, p.presets, p.tables, s, 0);
                });
    }
    if (frames > body) {
        p.y = y + body * 2; p.frames = frames - body; f.t0 = t0 + body;
        for (int s = 0; s < n_streams; ++s)
            for (int ear = 0; ear < 2; ++ear) {
                if (fade) eq_stage_fade_sequential(f, s, ear);
                else eq_stage_sequential(p, s, ear);
            }
    }
    return 0;
}

long long emu_eq_fade_length(double sample_rate) { return awef::fade_length(sample_rate); }
int emu_eq_keep() { return awk::kEqKeep; }

// clock: length, frame, fading, pending -> the clock after the call; segs: [3][6] = first, frames, t0, fade, begins, ends.  Returns the cuts' count.
int emu_eq_fade_plan(long long *clock, long long frames, long long *segs) {
    awef::Clock c;
    c.length = clock[0]; c.frame = clock[1]; c.fading = clock[2] != 0; c.pending = clock[3] != 0;
    const awef::Plan p = awef::plan(c, frames);
    for (int i = 0; i < p.n; ++i) {
        const awef::Segment &g = p.seg[i];
        long long *o = segs + i * 6;
        o[0] = g.first; o[1] = g.frames; o[2] = g.t0; o[3] = g.fade; o[4] = g.begins; o[5] = g.ends;
    }
    clock[0] = p.after.length; clock[1] = p.after.frame; clock[2] = p.after.fading; clock[3] = p.after.pending;
    return p.n;
}

}  // extern "C"
