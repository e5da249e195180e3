"""Cost of the look-ahead true-peak limiter (aw_spatializer_set_limiter) on cfg 2's shape through aw_spatializer_process: 128 streams x
10 s of 7.1 (8-channel) float32 at 48 kHz in device memory, the RoomSH1.0 HeSuVi preset, a fixed gain on every stream.  Device time of
whole calls between aw_context_timer_start / _stop, with the limiter off and on alternating in one process; then one profiled call of
each for the time of aw_limiter_kernel (on) and of aw_scale_kernel (off) — the kernel that reads and writes the same 16 bytes per frame
and the natural yardstick — and the device's measured copy rate (aw_context_bandwidth_probe), against which those 16 bytes are put.  On
a build without the limiter only the "off" case runs, so the same script times the parent commit.

    python tools/limiter_cost.py [--streams 128] [--seconds 10] [--attack 64] [--hold 128] [--reps 5]

One JSON line per call and a summary line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import airwave_amd as aw  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--attack", type=int, default=64)
    ap.add_argument("--hold", type=int, default=128)
    ap.add_argument("--ceiling", type=float, default=0.891)
    ap.add_argument("--gain", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    C, S, F = 8, a.streams, int(round(a.seconds * 48000))
    ctx = aw.Context(0)
    mgr = aw.HRIRManager(ctx)
    sp = mgr.activatePreset(os.path.join(ROOT, "tests", "golden", "hrtf", "RoomSH1.0.wav"), 48000.0, aw.InputLayout.detect(C), n_streams=S)
    has_limiter = hasattr(sp, "set_limiter")
    sp.set_gain("fixed", [a.gain])
    if has_limiter:
        sp.set_limiter(True, a.ceiling, a.attack, a.hold)      # everything is allocated before the reserve; the cases below switch it
        sp.reserve(F)
        sp.set_limiter(False)
    else:
        sp.reserve(F)
    d_in, d_out = ctx.alloc(S * F * C * 4), ctx.alloc(S * F * 2 * 4)
    ctx.synth_fill(d_in, S, F, C)
    cases = ["off"] + (["on"] if has_limiter else [])

    def call(case):
        if has_limiter:
            sp.set_limiter(case == "on", a.ceiling, a.attack, a.hold)
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
            print(json.dumps({"case": c, "rep": rep, "streams": S, "frames": F, "ms": round(t, 3), "g_frames_per_s": round(S * F / t / 1e6, 3)}),
                  flush=True)
    kernels = {}
    for c in cases:
        sp.set_profiling(True)
        call(c)
        ctx.synchronize()
        kernels.update({name: {"ms": round(t, 3), "launches": n} for name, t, n in sp.stage_times()
                        if name == ("aw_limiter_kernel" if c == "on" else "aw_scale_kernel")})
        sp.set_profiling(False)
    if has_limiter:
        rec = sp.limiter(0, min(S, 4))
        print(json.dumps({"min_gain_of_the_first_streams": [round(float(v), 4) for v in rec["min_gain"]],
                          "limited_frames": [int(v) for v in rec["limited_frames"]], "frames": int(rec["frames"][0])}), flush=True)
        sp.set_limiter(False)
    bw = ctx.bandwidth_probe(1 << 30, 3)
    rate = bw.get("copy", bw["read"])
    move_ms = S * F * 16 / (rate * 1e9) * 1e3
    out = {"summary": "limiter_cost", "streams": S, "frames": F, "attack": a.attack, "hold": a.hold, "gb_per_s": round(rate, 1),
           "ms_of_moving_16_bytes_per_frame": round(move_ms, 3), "kernels": kernels}
    for c in cases:
        out[f"{c}_ms_min"], out[f"{c}_ms_median"], out[f"{c}_ms_max"] = round(min(ms[c]), 3), round(float(np.median(ms[c])), 3), round(max(ms[c]), 3)
    if has_limiter:
        out["on_minus_off_ms_median"] = round(out["on_ms_median"] - out["off_ms_median"], 3)
        if "aw_limiter_kernel" in kernels and "aw_scale_kernel" in kernels:
            out["limiter_over_scale_kernel"] = round(kernels["aw_limiter_kernel"]["ms"] / kernels["aw_scale_kernel"]["ms"], 2)
    print(json.dumps(out), flush=True)
    ctx.free(d_in)
    ctx.free(d_out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
