// eq_fade_plan.hpp — the clock of the equalizer stage's target changes (aw_spatializer_set_equalizer_target) and how it cuts a batch call.
// Host only, no HIP, pure: tests/test_eq_fade_host.py holds it to cuts written out by hand.
//
// One clock per handle.  A published target begins at the first frame of the next call, or, while a fade runs, at the frame where that
// fade ends (ParametricEqualizerProcessor.swift:356-371: finishTransition starts the pending target), also in the middle of a call.  A call
// is cut at every frame where a fade begins or ends; every stream runs the pieces in order, each as a call of its own.
#pragma once
#include <cmath>
#include <cstdint>

namespace awef {

struct Clock {
    int64_t length = 1, frame = 0;          // T; frames of the running fade already rendered
    bool fading = false, pending = false;   // a fade runs; a target is published and has not begun
};

// :155, as aw_eq_create computes it (std::round: half away from zero)
inline int64_t fade_length(double sample_rate) {
    const long long t = (long long)std::round(sample_rate * 0.020);
    return t > 1 ? (int64_t)t : 1;
}

struct Segment {
    int64_t first, frames;     // of the call
    int64_t t0;                // fade: the clock at the segment's first frame
    bool fade;                 // the fading streams mix two renderings
    bool begins, ends;         // the published target begins at `first`; the fade ends with the segment's last frame
};

struct Plan {
    Segment seg[3];            // at most: the rest of a fade, the published target's whole fade, what follows it
    int n = 0;
    Clock after;               // the clock once the call is over
};

inline Plan plan(Clock c, int64_t frames) {
    Plan p;
    int64_t pos = 0;
    bool begins = false;
    if (!c.fading && c.pending) { c.fading = true; c.pending = false; c.frame = 0; begins = true; }
    while (pos < frames) {
        Segment &s = p.seg[p.n++];
        s.first = pos; s.t0 = 0; s.begins = begins; s.ends = false;
        begins = false;
        s.fade = c.fading;
        if (!c.fading) { s.frames = frames - pos; pos = frames; break; }
        s.t0 = c.frame;
        s.frames = frames - pos < c.length - c.frame ? frames - pos : c.length - c.frame;
        c.frame += s.frames; pos += s.frames;
        if (c.frame == c.length) {
            s.ends = true;
            c.fading = c.pending; c.pending = false; c.frame = 0;
            begins = c.fading;
        }
    }
    // (a target that would begin exactly where the call ends begins with the next call: its segment carries the mark)
    if (begins) { c.fading = false; c.pending = true; }
    p.after = c;
    return p;
}

}  // namespace awef
