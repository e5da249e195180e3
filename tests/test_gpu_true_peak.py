"""Per-stream true peak of the batch entries on the MI355X (aw_spatializer_set_true_peak / _get_true_peak, AW_GAIN_TRUE_PEAK_CEILING).
Two references, both over the float32 output the same call wrote: true_peak_ref.py (the windows in numpy float64, with the library's own
float32 coefficients; allowed: the per-window bound 12 * 2^-24 * sum |c| |v| of twelve correctly rounded operations) and the header's
sequential rule compiled by g++ (tests/emu/emu_true_peak.cpp), which the device must equal bit for bit.  Chunking, sample formats,
sharding, the page-locked single-stream path and splitting calls in time must change no bit: the convolution kernels themselves may round
differently when a call is cut (tests/test_gpu_loudness.py), so a cut run is held bit for bit to the rule over the output IT wrote, and to
the uncut run wherever the two outputs are the same bits."""
import ctypes
import os
import sys

import numpy as np
import pytest

import true_peak_ref as ref
from test_gpu_loudness import delta_spatializer, device_call, host_call, real_spatializer
from test_gpu_pcm_dither import F32, S16, context, encode

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_true_peak as emu  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(4, 0.0, 0.5), (4, 45.0, 0.5), (6, 60.0, 0.5), (8, 67.5, 0.5), (4, 45.0, 1.41)]      # (fs / frequency, phase in degrees, amplitude)


def rule(calls):
    """The header's sequential rule over the calls [S][F][2] of a run: (true peaks [S][2] float32, last call's peak [S], non-finite [S])."""
    m = emu.Meter(calls[0].shape[0], False)
    for y in calls:
        m.process(y)
    return m.tp.view(np.float32).copy(), m.call.view(np.float32).copy(), m.nonfinite.copy()


def check(tp, calls, what, coefficients):
    """tp: sp.true_peak() after the calls (float32 outputs [S][F][2])."""
    want_tp, want_call, want_bad = rule(calls)
    y = np.concatenate(calls, axis=1)
    for s in range(y.shape[0]):
        r = ref.measure(y[s], coefficients)
        err = np.abs(tp["true_peak"][s].astype(np.float64) - r["peak"])
        print(f"{what}: stream {s}: true peak {tp['true_peak'][s]} reference {r['peak']} difference {err} bound {r['bound']}")
        assert np.all(err <= r["bound"]), (what, s)
        assert tp["nonfinite"][s] == r["nonfinite"]
    assert np.array_equal(tp["true_peak"].view(np.uint32), want_tp.view(np.uint32)), what
    assert np.array_equal(tp["call_true_peak"].view(np.uint32), want_call.view(np.uint32)), what
    assert np.array_equal(tp["nonfinite"], want_bad) and np.all(tp["frames"] == y.shape[1]) and not tp["reserved"].any(), what


# ---- 1. known answers -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", [44100, 48000, 96000])
def test_sines_read_their_amplitude(rate):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    x = np.stack([ref.faded_sine(rate, rate / div, phase, amp) for div, phase, amp in CASES])
    sp = delta_spatializer(aw, ctx, rate, len(CASES))
    sp.set_true_peak(True)
    sp.set_metering(True)
    assert sp.info()["true_peak"] == 1
    y = host_call(sp, x)
    tp, lv = sp.true_peak(), sp.levels()
    c = aw.true_peak_filter()
    for s, (div, phase, amp) in enumerate(CASES):
        want = ref.measure(y[s], c)
        for e in range(2):
            got_db, ref_db = ref.db(float(tp["true_peak"][s, e])), ref.db(want["peak"][e])
            print(f"{rate} Hz fs/{div} at {phase} deg, amplitude {amp}, ear {e}: {got_db:.3f} dBTP (reference {ref_db:.3f}), sample peak "
                  f"{ref.db(float(lv['peak'][s, e])):.3f} dBFS")
            assert -0.4 <= got_db - ref.db(amp) <= 0.2 and -0.4 <= ref_db - ref.db(amp) <= 0.2
    assert ref.db(float(lv["peak"][1, 0])) < -9.0                       # the sample peak of the 45 degree case under-reads by 3 dB
    assert np.all(tp["true_peak"] >= lv["peak"])
    check(tp, [y], f"sines at {rate} Hz", c)


# ---- 2. parity on a real layout -------------------------------------------------------------------------------------------------------

def test_parity_with_numpy_on_a_real_layout(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    x = np.random.default_rng(61).uniform(-0.5, 0.5, (3, 4099, 7)).astype(np.float32)
    sp = real_spatializer(aw, ctx, oracle, 3)
    sp.set_true_peak(True)
    sp.set_metering(True)
    y = device_call(torch, sp, x)
    check(sp.true_peak(), [y], "real layout", aw.true_peak_filter())
    assert np.all(sp.true_peak()["true_peak"] >= sp.levels()["peak"])


# ---- 3. invariances -------------------------------------------------------------------------------------------------------------------

def test_chunking_formats_and_sharding_change_no_bit(oracle):
    import torch
    import airwave_amd as aw
    S, F = 5, 16411                                                   # (enough input bytes for AW_HOST_CHUNK_MB=1 to chunk 5 streams)
    x = np.random.default_rng(62).uniform(-0.5, 0.5, (S, F, 7)).astype(np.float32)
    x[2] *= np.float32(0.01)
    ctx, small = context(aw, torch, chunk_mb=64), context(aw, torch, chunk_mb=1)

    def measured(c, streams, first, run):
        sp = real_spatializer(aw, c, oracle, streams)
        sp.set_true_peak(True)
        run(sp, x[first:first + streams])
        return sp.true_peak(), sp

    kept = {}
    one, _ = measured(ctx, S, 0, lambda sp, xs: kept.update(y=device_call(torch, sp, xs)))
    check(one, [kept["y"]], "device entry", aw.true_peak_filter())
    chunked, sp_c = measured(small, S, 0, lambda sp, xs: host_call(sp, xs))
    assert 0 < sp_c.info()["host_chunk_streams"] < S
    assert chunked.tobytes() == one.tobytes()
    for run in (lambda sp, xs: host_call(sp, xs, S16), lambda sp, xs: device_call(torch, sp, xs, S16)):
        for c in (ctx, small):
            assert measured(c, S, 0, run)[0].tobytes() == one.tobytes()
    shards = [measured(ctx, k, first, lambda sp, xs: device_call(torch, sp, xs))[0] for first, k in ((0, 2), (2, 3))]
    assert np.concatenate(shards).tobytes() == one.tobytes()


def test_splitting_calls_in_time_changes_no_bit(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, F = 5, 4099
    x = np.random.default_rng(63).uniform(-0.5, 0.5, (S, F, 7)).astype(np.float32)
    c = aw.true_peak_filter()
    runs = []
    for splits in ((F,), (5, 11, 4083)):
        sp = real_spatializer(aw, ctx, oracle, S)
        sp.set_true_peak(True)
        ys, at = [], 0
        for n in splits:
            ys.append(device_call(torch, sp, x[:, at:at + n]))
            at += n
        tp = sp.true_peak()
        check(tp, ys, f"calls of {splits}", c)
        runs.append((np.concatenate(ys, axis=1), tp))
    same_y = np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    print(f"outputs of the cut and the uncut run identical: {same_y}")
    if same_y:
        assert np.array_equal(runs[0][1]["true_peak"].view(np.uint32), runs[1][1]["true_peak"].view(np.uint32))
    # through a unit impulse the outputs do not depend on the cut on any kernel path that reproduces its input exactly: checked, then held
    runs = []
    xd = np.random.default_rng(64).uniform(-0.9, 0.9, (S, F, 2)).astype(np.float32)
    for splits in ((F,), (5, 11, 4083)):
        sp = delta_spatializer(aw, ctx, 48000, S)
        sp.set_true_peak(True)
        ys, at = [], 0
        for n in splits:
            ys.append(host_call(sp, xd[:, at:at + n]))
            at += n
        check(sp.true_peak(), ys, f"unit impulse, calls of {splits}", c)
        runs.append((np.concatenate(ys, axis=1), sp.true_peak()))
    if np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32)):
        assert np.array_equal(runs[0][1]["true_peak"].view(np.uint32), runs[1][1]["true_peak"].view(np.uint32))


def test_single_stream_callback_path_equals_the_stream_inside_a_batch():
    """One stream, callback-sized calls of the host entry: the kernels write page-locked memory and the true-peak kernel reads it."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    calls = [4096, 3]
    x = np.random.default_rng(65).uniform(-0.9, 0.9, (3, sum(calls), 2)).astype(np.float32)
    c = aw.true_peak_filter()
    one, batch = delta_spatializer(aw, ctx, 44100, 1), delta_spatializer(aw, ctx, 44100, 3)
    one.reserve_host(4096)
    got = {}
    for name, sp, xs in (("callback", one, x[1:2]), ("batch", batch, x)):
        sp.set_true_peak(True)
        ys, at = [], 0
        for n in calls:
            ys.append(host_call(sp, xs[:, at:at + n]))
            at += n
        check(sp.true_peak(), ys, name, c)
        got[name] = (np.concatenate(ys, axis=1), sp.true_peak())
    assert one.info()["host_chunk_streams"] == 0
    if np.array_equal(got["callback"][0].view(np.uint32), got["batch"][0][1:2].view(np.uint32)):
        assert got["callback"][1].tobytes() == got["batch"][1][1:2].tobytes()


# ---- 4. rules -------------------------------------------------------------------------------------------------------------------------

def test_reset_off_on_and_getter_errors():
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    rng = np.random.default_rng(66)
    a, b = (rng.uniform(-0.9, 0.9, (2, 300, 2)).astype(np.float32) for _ in range(2))
    b *= np.float32(0.5)
    sp = delta_spatializer(aw, ctx, 48000, 2)
    with pytest.raises(aw.AirwaveError):
        sp.true_peak()                                                # neither the setter nor the gain mode was ever used
    assert sp.info()["true_peak"] == 0
    sp.set_true_peak(True)
    with pytest.raises(ValueError):
        sp.true_peak(1, 2)
    assert sp._lib.aw_spatializer_get_true_peak(sp._h, -1, 1, None) == 1 and sp._lib.aw_spatializer_get_true_peak(sp._h, 0, 3, None) == 1
    assert sp._lib.aw_spatializer_get_true_peak(sp._h, 0, 1, None) == 1
    ya = host_call(sp, a)
    tp_a = sp.true_peak()
    check(tp_a, [ya], "first call", aw.true_peak_filter())
    sp.set_true_peak(False)
    assert sp.info()["true_peak"] == 0 and sp.true_peak().tobytes() == tp_a.tobytes()      # readable, and unmeasured calls leave it alone
    host_call(sp, a)
    assert sp.true_peak().tobytes() == tp_a.tobytes()
    sp.set_true_peak(True)                                            # off -> on: the history is zeroed, the peaks stay
    yb = host_call(sp, b)
    tp = sp.true_peak()
    alone_tp, alone_call, _ = rule([yb])
    assert np.array_equal(tp["call_true_peak"].view(np.uint32), alone_call.view(np.uint32))
    assert np.array_equal(tp["true_peak"], np.maximum(tp_a["true_peak"], alone_tp)) and np.all(tp["true_peak"] == tp_a["true_peak"])
    assert np.all(tp["frames"] == 600)
    for reset in (sp.reset_levels, sp.reset):
        host_call(sp, a)
        reset()
        z = sp.true_peak()
        assert not z["true_peak"].any() and not z["call_true_peak"].any() and not z["frames"].any() and not z["nonfinite"].any()
        y = host_call(sp, b)                                          # the history started over too
        check(sp.true_peak(), [y], "after a reset", aw.true_peak_filter())
        reset()


def test_off_means_off(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    x = np.random.default_rng(67).uniform(-0.5, 0.5, (3, 5003, 7)).astype(np.float32)
    for fout in (F32, S16):
        plain, measured = real_spatializer(aw, ctx, oracle, 3), real_spatializer(aw, ctx, oracle, 3)
        measured.set_true_peak(True)
        for sp in (plain, measured):
            sp.set_profiling(True)
        for run in (lambda sp: device_call(torch, sp, x, fout), lambda sp: host_call(sp, x, fout)):
            a, b = run(plain), run(measured)
            assert a.tobytes() == b.tobytes()
        ctx.synchronize()
        assert "aw_true_peak_kernel" not in [n for n, _, _ in plain.stage_times()]
        assert "aw_true_peak_kernel" in [n for n, _, _ in measured.stage_times()]
        allocs = measured.info()["device_allocs"]
        measured.set_true_peak(False)
        measured.set_gain("peak_ceiling", ceiling=0.5)                # off, and a gain that is not the new mode: no true-peak launch
        measured.set_profiling(True)
        host_call(measured, x, fout)
        ctx.synchronize()
        names = [n for n, _, _ in measured.stage_times()]
        assert "aw_true_peak_kernel" not in names and "aw_levels_kernel" in names
        measured.set_gain("none")
        allocs = measured.info()["device_allocs"]
        measured.set_true_peak(True)                                  # the records and the allocation stay
        assert measured.info()["device_allocs"] == allocs and measured.true_peak()["frames"][0] == 2 * 5003


# ---- 5. the gain that holds a true-peak ceiling ------------------------------------------------------------------------------------------

def auto_gain(tp, c):
    tp = np.asarray(tp, np.float32)
    return np.where(tp > np.float32(c), (np.float64(np.float32(c)) / tp.astype(np.float64)).astype(np.float32), np.float32(1.0))


@pytest.mark.parametrize("entry", ["batch", "callback"])
def test_true_peak_ceiling_gain(entry):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    rate, c = 48000, 0.5
    S = 3 if entry == "batch" else 1
    x = np.stack([ref.faded_sine(rate, rate / 4, 45.0, 0.9)] * S)
    if S > 1:
        x[-1] *= np.float32(0.25)                                     # (the batch's last stream stays under the ceiling: gain 1)

    def handle():
        sp = delta_spatializer(aw, ctx, rate, S)
        if entry == "callback":
            sp.reserve_host(4096)
            return sp, x[:, :4096]
        return sp, x

    plain, xs = handle()
    y = host_call(plain, xs)
    _, want_call, _ = rule([y])
    g = auto_gain(want_call, c)
    assert S == 1 or (g[0] < 1.0 and g[-1] == 1.0)
    for fout in (F32, S16):
        sp, _ = handle()
        sp.set_gain("true_peak_ceiling", ceiling=c)                   # (set_true_peak stays off: the kernel runs for the gain alone)
        assert sp.info()["gain_mode"] == 3 and sp.info()["true_peak"] == 0
        sp.set_profiling(True)
        out = host_call(sp, xs, fout)
        lv, tp = sp.levels(), sp.true_peak()
        assert np.array_equal(tp["call_true_peak"].view(np.uint32), want_call.view(np.uint32)) and not tp["true_peak"].any() and not tp["frames"].any()
        assert np.array_equal(lv["gain"].view(np.uint32), auto_gain(tp["call_true_peak"], c).view(np.uint32))
        yg = y * g[:, None, None]
        if fout == F32:
            assert np.array_equal(out.view(np.uint32), yg.view(np.uint32))
            over = float(np.max(ref.measure(out[0], aw.true_peak_filter())["peak"]))
            print(f"{entry}: true peak of the gained output {over:.7f} (ceiling {c})")
        else:
            assert np.array_equal(out, encode(S16, yg)[0])
        if entry == "batch":
            ctx.synchronize()
            names = [n for n, _, _ in sp.stage_times()]
            assert "aw_true_peak_kernel" in names and "aw_levels_kernel" not in names
        sp.set_gain("peak_ceiling", ceiling=c)
        host_call(sp, xs, fout)
        assert sp.info()["gain_mode"] == 2 and np.all(sp.levels()["gain"][: max(1, S - 1)] > lv["gain"][: max(1, S - 1)])
        sp.set_gain("true_peak_ceiling", ceiling=c)
        for bad in (0.0, -0.5, 1.5, float("nan")):
            assert sp._lib.aw_spatializer_set_gain(sp._h, 3, None, 0, ctypes.c_float(bad)) == 1
            with pytest.raises(ValueError):
                sp.set_gain("true_peak_ceiling", ceiling=bad)
        assert sp.info()["gain_mode"] == 3
        sp.set_metering(True)
        sp.set_true_peak(True)
        sp.reset()                                                    # (the stream starts over: the same frames behind silence)
        out2 = host_call(sp, xs, fout)
        assert out2.tobytes() == out.tobytes()                        # the records do not touch the gain
        assert np.all(sp.true_peak()["true_peak"] >= sp.levels()["peak"]) and sp.true_peak()["frames"][0] == xs.shape[1]
