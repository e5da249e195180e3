"""What a target change of the equalizer stage costs (equalizer stage: target changes), at cfg 2's shape: 128 streams x 10 s
at 48 kHz, the five-filter preset of tests/test_gpu_eq.py installed on every stream.

  python tools/eq_fade_cost.py [--streams 128] [--seconds 10] [--reps 10] [--out eq_fade_cost.json]
  python tools/eq_fade_cost.py --stage-only --package-root <checkout of another commit, built>      aw_eq_stage_kernel on that commit

One process, everything warm.  Every repetition runs, in this order:
  stage     a batch call with the stage on and nothing published: device time of aw_eq_stage_kernel (aw_spatializer_stage_time)
  fade      the same call right after set_equalizer_target for every stream: the stage's kernels by name, and the whole call between
            two events (--stage-only leaves this and the next out: a commit without the entry can be measured)
  aw_eq     aw_eq_process over the stage-off output with a target set: its fade is two cascade launches over the 960 frames into two
            scratch buffers and a blend launch, then the rest of the call; between two events, beside the same call with no target
The convolution in front is a unit impulse on two channels: it only fills the buffer the equalizer works on."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILTERS = [(1, 105.0, -2.8, 0.7), (0, 65.3, 1.0, 1.68), (0, 1000.0, 6.0, 0.707), (2, 10000.0, -5.2, 0.7), (0, 20.0, 3.0, 4.0)]      # tests/test_gpu_eq.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--stage-only", action="store_true", help="time aw_eq_stage_kernel alone (works on commits without the target entry)")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose airwave_amd is measured")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, os.path.abspath(a.package_root))
    import airwave_amd as aw
    assert os.path.dirname(os.path.dirname(os.path.abspath(aw.__file__))) == os.path.abspath(a.package_root), aw.__file__
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures device time and has no other mode")
    fs = 48000.0
    S, F = a.streams, int(a.seconds * fs)
    F -= F % 32                                                      # whole chunks: one stage launch per call
    preset = aw.EqualizerDefinition(-2.56, [aw.EqualizerFilter(1, None, True, t, f, g, q) for t, f, g, q in FILTERS])
    other = aw.EqualizerDefinition(-1.0, [aw.EqualizerFilter(1, None, True, t, f * 1.1, g, q) for t, f, g, q in FILTERS])
    ctx = aw.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    h = np.zeros((2, 256), np.float32)
    h[0, 0] = 1.0
    lt, rt = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    make = lambda: aw.Spatializer(aw.HRIR(h, sample_rate=fs, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    x = torch.empty((S, F, 2), dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    ctx.synth_fill(x.data_ptr(), S, F, 2, seed=77)
    staged, plain = make(), make()
    staged.set_equalizer([preset])
    for sp in (staged, plain):
        sp.reserve(F)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(sp):
        """-> (the whole call between two events, {kernel name: ms})"""
        sp.set_profiling(True)                                       # (starts the sums again)
        e0.record()
        sp.process_device(x.data_ptr(), y.data_ptr(), F)
        e1.record()
        ctx.synchronize()
        return e0.elapsed_time(e1), {n: t * k for n, t, k in sp.stage_times() if n.startswith("aw_eq_")}

    def eq_call(proc):
        e0.record()
        proc.process_device(y.data_ptr(), y.data_ptr(), F)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    names = ["stage_kernel"] if a.stage_only else ["stage_kernel", "call", "fade_call", "fade_kernel", "fade_call_stage_kernel", "fade_turns", "aw_eq_call", "aw_eq_fade_call"]
    times = {k: [] for k in names}
    proc = None if a.stage_only else aw.ParametricEqualizerProcessor(fs, 0, n_streams=S, ctx=ctx)
    if proc is not None:
        proc.setTarget(preset)
        eq_call(proc)
        proc.drainRetiredStates()
    for rep in range(a.reps + 2):                                    # the first two repetitions warm everything up
        whole, k = call(staged)
        row = {"stage_kernel": k["aw_eq_stage_kernel"], "call": whole}
        if not a.stage_only:
            staged.set_equalizer_target([other if rep % 2 == 0 else preset])
            whole, k = call(staged)
            row.update(fade_call=whole, fade_kernel=k["aw_eq_stage_fade_kernel"], fade_call_stage_kernel=k["aw_eq_stage_kernel"], fade_turns=k["aw_eq_stage_turn_kernel"])
            plain.process_device(x.data_ptr(), y.data_ptr(), F)
            row["aw_eq_call"] = eq_call(proc)
            proc.drainRetiredStates()
            plain.process_device(x.data_ptr(), y.data_ptr(), F)
            proc.setTarget(other if rep % 2 == 0 else preset)
            row["aw_eq_fade_call"] = eq_call(proc)
            proc.drainRetiredStates()
        if rep >= 2:
            for name in names:
                times[name].append(row[name])
    res = {"package_root": os.path.relpath(os.path.abspath(a.package_root), ROOT), "streams": S, "frames": F, "sample_rate": fs, "reps": a.reps, "filters": len(FILTERS)}
    for k, v in times.items():
        res[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
