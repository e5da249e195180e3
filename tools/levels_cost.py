"""Cost of the level meter and the automatic gain (aw_spatializer_set_metering / _set_gain) on the s16 entries with float32 input: G stereo
frames/s of the page-locked host entry and of the device entry, plain, metered and under AW_GAIN_PEAK_CEILING, alternating (the order
rotates every repetition); then one profiled call per case for aw_levels_kernel next to aw_pcm_encode_kernel (HIP events around each
launch).  On a build without the meter only the plain case runs, so the same script times the parent commit.

    python tools/levels_cost.py [--channels 8] [--taps 4320] [--streams 128] [--seconds 10] [--reps 3]

One JSON line per measurement and a summary line per entry and case (min / median / max, and the ratio to plain)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import airwave_amd as aw  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--taps", type=int, default=4320)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    C, S, F = a.channels, a.streams, int(round(a.seconds * 48000))
    rng = np.random.default_rng(1)
    h = (rng.standard_normal((14, a.taps)) * np.exp(-np.arange(a.taps) / (a.taps / 6.0)) * 0.05).astype(np.float32)
    lt, rt = (np.arange(C) % 14).astype(np.int32), ((np.arange(C) + 7) % 14).astype(np.int32)
    base = (rng.standard_normal((4, F, C)) * 0.1).astype(np.float32)
    ctx = aw.Context(0)
    sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    has_meter = hasattr(sp, "set_metering")
    if has_meter:
        sp.set_metering(True)                       # the records exist before the reserve; the cases below switch the meter itself
        sp.set_metering(False)
    sp.reserve_pcm(F, "f32", "s16")
    x, y = ctx.pinned_empty((S, F, C), np.float32), ctx.pinned_empty((S, F, 2), np.int16)
    for i in range(S):
        x[i] = base[i % 4]
    d_in, d_out = ctx.alloc(x.nbytes), ctx.alloc(y.nbytes)
    ctx.h2d(d_in, x)
    cases = ["plain"] + (["metered", "peak_ceiling"] if has_meter else [])

    def setup(case):
        if has_meter:
            sp.set_metering(case == "metered")
            sp.set_gain("peak_ceiling", ceiling=0.98) if case == "peak_ceiling" else sp.set_gain("none")

    def call(entry, case):
        setup(case)
        t = time.perf_counter()
        if entry == "host":
            sp.process_host_into(x, y, in_format="f32", out_format="s16")
        else:
            sp.process_pcm_device(d_in, "f32", d_out, "s16", F)
            ctx.synchronize()
        return time.perf_counter() - t

    runs = [(e, c) for e in ("host", "device") for c in cases]
    for e, c in runs:
        call(e, c)
    rates = {}
    for rep in range(a.reps):
        for e, c in runs[rep % len(runs):] + runs[:rep % len(runs)]:
            dt_s = call(e, c)
            rates.setdefault((e, c), []).append(S * F / dt_s / 1e9)
            print(json.dumps({"entry": e, "case": c, "rep": rep, "channels": C, "taps": a.taps, "streams": S, "frames": F, "seconds": round(dt_s, 4),
                              "g_frames_per_s": round(S * F / dt_s / 1e9, 4)}), flush=True)
    for e, c in runs:
        sp.set_profiling(True)
        call(e, c)
        stages = {name: {"ms": round(ms, 3), "launches": n} for name, ms, n in sp.stage_times()}
        sp.set_profiling(False)
        r = rates[(e, c)]
        print(json.dumps({"summary": e, "case": c, "g_frames_per_s_min": round(min(r), 4), "median": round(float(np.median(r)), 4), "max": round(max(r), 4),
                          "vs_plain_median": round(float(np.median(r)) / float(np.median(rates[(e, "plain")])), 4),
                          "kernels": {k: stages[k] for k in ("aw_levels_kernel", "aw_pcm_encode_kernel", "aw_scale_kernel") if k in stages}}), flush=True)
    setup("plain")
    ctx.free(d_in)
    ctx.free(d_out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
