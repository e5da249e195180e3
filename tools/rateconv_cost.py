"""Cost of the batch sample-rate converter ("Batch sample-rate converter", the cost table): aw_context_timer_* around one call
of `streams` streams x `seconds` of stereo, median of `reps` calls after `warmup`, for 44.1 -> 48 kHz and 96 -> 44.1 kHz.  The float32
entry (aw_rateconv_process) first; then, where the library has them, the PCM entries (aw_pcm_rateconv_process): f32 -> f32, s16 -> s16
plain, s16 -> s16 with TPDF dither, s24 -> s24 with high-pass TPDF, fixed gain and metering; then, where the library has them, the
true-peak entries: s16 -> s16 plain with measuring on, and aw_tp_rateconv_measure of the same s16 input.  On a build without the PCM or
the true-peak entries those cases are left out, so the same script times an earlier commit.

    python tools/rateconv_cost.py [--streams 1024] [--seconds 10] [--reps 7] [--warmup 2] [--probe] [--cases s16,aw_rateconv]

One JSON line per case: the calls' milliseconds, their median and spread ((max - min) / median), the bytes the call moves."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import airwave_amd as aw  # noqa: E402

BYTES = {"f32": 4, "s16": 2, "s24": 3, "s32": 4}
# name -> (input format, output format, dither, fixed gain, metering[, true peak: "on" measured and written, "only" aw_tp_rateconv_measure]);
# None: the float32 entry
CASES = [("f32->f32 aw_rateconv_process", None), ("f32->f32 pcm entry", ("f32", "f32", "none", None, False)), ("s16->s16 plain", ("s16", "s16", "none", None, False)),
         ("s16->s16 tpdf", ("s16", "s16", "tpdf", None, False)), ("s24->s24 tpdf_hp gain metering", ("s24", "s24", "tpdf_hp", 0.7, True)),
         ("s16->s16 plain, true peak on", ("s16", "s16", "none", None, False, "on")), ("s16 aw_tp_rateconv_measure", ("s16", "s16", "none", None, False, "only"))]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="", help="comma-separated substrings: only the cases whose name holds one of them")
    ap.add_argument("--probe", action="store_true", help="also measure the device's copy rate (aw_context_bandwidth_probe)")
    a = ap.parse_args()
    S, C = a.streams, 2
    ctx = aw.Context(0)
    has_pcm, has_tp = hasattr(aw.RateConverter, "process_pcm_device"), hasattr(aw.RateConverter, "measure_device")
    wanted = [w for w in a.cases.split(",") if w]
    if a.probe:
        print(json.dumps({"copy_rate_gb_s": round(ctx.bandwidth_probe()["copy"], 1)}), flush=True)
    rng = np.random.default_rng(1)
    for in_rate, out_rate in ((44100, 48000), (96000, 44100)):
        F = int(round(a.seconds * in_rate))
        rc = aw.RateConverter(in_rate, out_rate, S, C, ctx=ctx)
        cap = -(-F * out_rate // in_rate) + 8                       # (a call in steady state makes F L / M frames, the first one fewer)
        d_in, d_out = ctx.alloc(S * F * C * 4), ctx.alloc(S * cap * C * 4)
        filled = None
        for name, form in CASES:
            tp = form[5] if form is not None and len(form) > 5 else None
            if (form is not None and not has_pcm) or (tp and not has_tp) or (wanted and not any(w in name for w in wanted)):
                continue
            fi, fo = ("f32", "f32") if form is None else form[:2]
            if filled != fi:                                         # the input in its format: synthetic float32, or random integer PCM
                if fi == "f32":
                    ctx.synth_fill(d_in, S, F, C)
                else:
                    block = rng.integers(0, 256, (16, F, C, BYTES[fi]), dtype=np.uint8)          # (every byte pattern is a sample)
                    for s0 in range(0, S, 16):
                        n = min(16, S - s0)
                        ctx.h2d(d_in + s0 * F * C * BYTES[fi], block[:n])
                filled = fi
            if has_pcm:
                rc.set_dither("none" if form is None else form[2], 7, 0)
                rc.set_gain("none") if form is None or form[3] is None else rc.set_gain("fixed", [form[3]])
                rc.set_metering(bool(form and form[4]))
            if has_tp:
                rc.set_true_peak(bool(tp))
            rc.reset()
            ms, frames = [], 0
            for i in range(a.warmup + a.reps):
                n_out = rc.output_frames(F)
                ctx.timer_start()
                if form is None:
                    made = rc.process_device(d_in, F, d_out, cap)
                elif tp == "only":
                    made = rc.measure_device(d_in, fi, F)
                else:
                    made = rc.process_pcm_device(d_in, fi, F, d_out, fo, cap)
                t = ctx.timer_stop()
                assert made == n_out
                if i >= a.warmup:
                    ms.append(t)
                    frames = made
            med = float(np.median(ms))
            print(json.dumps({"pair": f"{in_rate}->{out_rate}", "case": name, "streams": S, "in_frames": F, "out_frames": frames,
                              "bytes": S * C * (F * BYTES[fi] + (0 if tp == "only" else frames * BYTES[fo])), "ms": [round(t, 3) for t in ms], "median_ms": round(med, 3),
                              "spread": round((max(ms) - min(ms)) / med, 4)}), flush=True)
        ctx.free(d_in)
        ctx.free(d_out)
        rc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
