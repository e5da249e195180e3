"""What the equalizer stage of the batch entries costs (equalizer stage): device time of aw_eq_stage_kernel against
aw_eq_cascade_kernel over the same buffer, cfg 4's equalizer shape (512 streams x 10 s at 96 kHz, CCA CRA ParametricEq.txt) unless
--streams / --rate / --five-filters say otherwise.

  python tools/eq_stage_cost.py [--streams 512] [--seconds 10] [--reps 10] [--out eq_stage_cost.json]
  python tools/eq_stage_cost.py --cascade-only --package-root <checkout of another commit, built>     the yardstick on that commit

One process, everything warm, the three cases alternating inside every repetition:
  cascade   a plain spatializer's call, then aw_eq_state_process in place on its output: HIP events around that one launch
  stage     the same spatializer with the preset installed for every stream: the stage's own event pair (aw_spatializer_stage_time)
  stage x2  two presets (the fixture and Bass Booster.txt) alternating by stream, likewise
The convolution in front is a unit impulse on two channels: it only fills the buffer the equalizer works on."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--rate", type=float, default=96000.0, help="sample rate (cfg 2's shape: --streams 128 --rate 48000 --five-filters)")
    ap.add_argument("--five-filters", action="store_true", help="the five-filter preset of tests/test_gpu_eq.py instead of the fixture's ten")
    ap.add_argument("--cascade-only", action="store_true", help="time the cascade leg alone (works on commits without the stage)")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose airwave_amd is measured (its presets are read from this one)")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, os.path.abspath(a.package_root))
    import airwave_amd as aw
    assert os.path.dirname(os.path.dirname(os.path.abspath(aw.__file__))) == os.path.abspath(a.package_root), aw.__file__
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures device time and has no other mode")
    fs = a.rate
    S, F = a.streams, int(a.seconds * fs)
    F -= F % 32                                                      # whole chunks: one launch per call on either side
    eq_dir = os.path.join(ROOT, "tests", "golden", "eq")
    parse = lambda name: aw.EqualizerAPOParser.parse(open(os.path.join(eq_dir, name), "rb").read(), name)
    fixture, other = parse("CCA CRA ParametricEq.txt"), parse("Bass Booster.txt")
    if a.five_filters:
        five = [(1, 105.0, -2.8, 0.7), (0, 65.3, 1.0, 1.68), (0, 1000.0, 6.0, 0.707), (2, 10000.0, -5.2, 0.7), (0, 20.0, 3.0, 4.0)]
        fixture = aw.EqualizerDefinition(-2.56, [aw.EqualizerFilter(1, None, True, t, f, g, q) for t, f, g, q in five])
    ctx = aw.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    h = np.zeros((2, 256), np.float32)
    h[0, 0] = 1.0
    lt, rt = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    make = lambda: aw.Spatializer(aw.HRIR(h, sample_rate=fs, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    x = torch.empty((S, F, 2), dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    ctx.synth_fill(x.data_ptr(), S, F, 2, seed=77)
    plain = make()
    one = two = None
    if not a.cascade_only:
        one, two = make(), make()
        one.set_equalizer([fixture])
        two.set_equalizer([fixture, other], [s & 1 for s in range(S)])
    state = aw.ParametricEqualizerState(fixture, fs, n_streams=S, ctx=ctx)
    for sp in (plain, one, two):
        if sp is not None:
            sp.reserve(F)
    times = {"cascade": []} if a.cascade_only else {"cascade": [], "stage": [], "stage_two_presets": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def staged(sp):
        sp.set_profiling(True)                                       # (starts the sums again)
        sp.process_device(x.data_ptr(), y.data_ptr(), F)
        ctx.synchronize()
        (ms,) = [t for n, t, k in sp.stage_times() if n == "aw_eq_stage_kernel"]
        return ms

    for rep in range(a.reps + 2):                                    # the first two repetitions warm everything up
        plain.process_device(x.data_ptr(), y.data_ptr(), F)
        e0.record()
        state.process_device(y.data_ptr(), y.data_ptr(), F)
        e1.record()
        torch.cuda.synchronize()
        row = (e0.elapsed_time(e1),) if a.cascade_only else (e0.elapsed_time(e1), staged(one), staged(two))
        if rep >= 2:
            for k, v in zip(times, row):
                times[k].append(v)
    res = {"package_root": os.path.relpath(os.path.abspath(a.package_root), ROOT), "streams": S, "frames": F, "sample_rate": fs, "reps": a.reps, "filters": [state.filterCount, len(other.filters)]}
    for k, v in times.items():
        res[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}
    if not a.cascade_only:
        res["stage_over_cascade"] = res["stage"]["median_ms"] / res["cascade"]["median_ms"]
        res["two_presets_over_cascade"] = res["stage_two_presets"]["median_ms"] / res["cascade"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
