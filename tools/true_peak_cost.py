"""Cost of the true-peak measurement (aw_spatializer_set_true_peak) on cfg 3's shape through aw_spatializer_process: 1024 streams x 10 s
of 7-channel float32 at 48 kHz in device memory, a 14 x 32768-tap HRIR, the level meter on.  Device time of whole calls between
aw_context_timer_start / _stop, with the true peak off and on alternating in one process; then one profiled call for the time of
aw_true_peak_kernel itself next to aw_levels_kernel (HIP events around their launches) and the device's measured read rate
(aw_context_bandwidth_probe), against which the kernel's 8 bytes per output frame are put.  On a build without the measurement only the
"off" case runs, so the same script times the parent commit.

    python tools/true_peak_cost.py [--streams 1024] [--seconds 10] [--taps 32768] [--reps 5]

One JSON line per call and a summary line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import airwave_amd as aw  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--taps", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    C, S, F = 7, a.streams, int(round(a.seconds * 48000))
    rng = np.random.default_rng(1234)
    h = (rng.standard_normal((14, a.taps)) * np.exp(-np.arange(a.taps) / (a.taps / 6.0)) * 0.02).astype(np.float32)
    lt, rt = np.array([0, 8, 6, 4, 12, 2, 10], np.int32), np.array([1, 7, 13, 5, 11, 3, 9], np.int32)
    ctx = aw.Context(0)
    sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    has_true_peak = hasattr(sp, "set_true_peak")
    sp.set_metering(True)
    if has_true_peak:
        sp.set_true_peak(True)                      # the records exist before the reserve; the cases below switch the measurement itself
        sp.set_true_peak(False)
    sp.reserve(F)
    d_in, d_out = ctx.alloc(S * F * C * 4), ctx.alloc(S * F * 2 * 4)
    ctx.synth_fill(d_in, S, F, C)
    cases = ["off"] + (["on"] if has_true_peak else [])

    def call(case):
        if has_true_peak:
            sp.set_true_peak(case == "on")
        sp.reset()
        ctx.synchronize()
        ctx.timer_start()
        sp.process_device(d_in, d_out, F)
        return ctx.timer_stop()

    for c in cases:
        call(c)
    ms = {c: [] for c in cases}
    for rep in range(a.reps):
        for c in (cases if rep % 2 == 0 else cases[::-1]):
            t = call(c)
            ms[c].append(t)
            print(json.dumps({"case": c, "rep": rep, "streams": S, "frames": F, "taps": a.taps, "ms": round(t, 3),
                              "g_frames_per_s": round(S * F / t / 1e6, 3)}), flush=True)
    sp.set_profiling(True)
    call(cases[-1])
    ctx.synchronize()
    kernels = {name: {"ms": round(t, 3), "launches": n} for name, t, n in sp.stage_times() if name in ("aw_true_peak_kernel", "aw_levels_kernel")}
    sp.set_profiling(False)
    if has_true_peak:
        tp = sp.true_peak(0, min(S, 4))
        print(json.dumps({"dbtp_of_the_first_streams": [round(float(20 * np.log10(v.max())), 3) for v in tp["true_peak"]],
                          "sample_peak_db": [round(float(20 * np.log10(v.max())), 3) for v in sp.levels(0, min(S, 4))["peak"]],
                          "frames": int(tp["frames"][0])}), flush=True)
        sp.set_true_peak(False)
    bw = ctx.bandwidth_probe(1 << 30, 3)
    read_ms = S * F * 8 / (bw["read"] * 1e9) * 1e3
    out = {"summary": "true_peak_cost", "streams": S, "frames": F, "taps": a.taps, "read_gb_per_s": round(bw["read"], 1),
           "ms_of_reading_8_bytes_per_frame": round(read_ms, 3), "kernels": kernels}
    for c in cases:
        out[f"{c}_ms_min"], out[f"{c}_ms_median"], out[f"{c}_ms_max"] = round(min(ms[c]), 3), round(float(np.median(ms[c])), 3), round(max(ms[c]), 3)
    if has_true_peak:
        out["on_minus_off_ms_median"] = round(out["on_ms_median"] - out["off_ms_median"], 3)
        if "aw_true_peak_kernel" in kernels:
            out["kernel_over_read_time"] = round(kernels["aw_true_peak_kernel"]["ms"] / read_ms, 2)
            if "aw_levels_kernel" in kernels:
                out["kernel_over_levels_kernel"] = round(kernels["aw_true_peak_kernel"]["ms"] / kernels["aw_levels_kernel"]["ms"], 2)
    print(json.dumps(out), flush=True)
    ctx.free(d_in)
    ctx.free(d_out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
