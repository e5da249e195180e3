"""The equalizer stage of the batch entries on the MI355X (aw_spatializer_set_equalizer): one preset per stream between the convolution
and the first meter.  The reference is the two-call path the stage replaces — the same handle's output with the stage off, then a
ParametricEqualizerState of the stream's preset over the same calls — which the stage must equal bit for bit: it runs the same function
template on the same tables at the same frame positions.  Chunking by streams, sample formats, sharding and the page-locked
single-stream path must change no bit; the meters, the gain, the limiter and the encode must see the equalized signal."""
import ctypes
import os
import sys

import numpy as np
import pytest

from test_gpu_loudness import all_hops, check_against_reference, device_call, host_call, reference_hops
from test_gpu_pcm_dither import F32, S16, S24, context, encode, from_dev, out_host, to_dev

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

pytestmark = pytest.mark.gpu

ULP = 6e-8               # tests/test_gpu_eq.py: 2^-24, one unit in the last place at |y| < 1
RATE, TAPS = 48000.0, 300
LT, RT = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
FILTERS = [(1, 105.0, -2.8, 0.7), (0, 65.3, 1.0, 1.68), (0, 1000.0, 6.0, 0.707), (2, 10000.0, -5.2, 0.7), (0, 20.0, 3.0, 4.0)]        # tests/test_gpu_eq.py
MANY = [(i % 3, 100.0 + 300.0 * i, ((i % 5) - 2) * 1.5, 0.5 + 0.1 * i) for i in range(64)]                                            # its 64-filter set
A, B, C = (-2.56, FILTERS), (-6.0, MANY), (6.0, [])
PRESETS = [A, B, C]
MAP9 = [0, 1, 2, -1, 0, 1, 2, -1, 0]
LEVEL = 0.15             # input level: the convolution's output then peaks near 0.25 and every equalized stream stays under 1
# The level of the test that also compares with the float64 truth.  That comparison's bound is absolute (ULP), and the signal the stage is
# handed is the convolution kernels' float32 output, not the truth's: the project holds those kernels to 1e-5 of the output's peak
# (tests/test_gpu_parity.py), and at LEVEL they are 2.1e-7 away from the truth at a peak of 0.23 — 9e-7 of the peak, 3.5 x ULP before the
# equalizer has run.  So that the bound sees the stage and not the kernels in front of it, the signal is small enough for 9e-7 of its peak
# to stay well under ULP: a peak near 0.008, at most doubled by a preset, leaves about 1.5e-8.  What the bound then catches is a wrong
# preset, a wrong state row or a lost carry (1e-4 and more at this level); the last bit is held at LEVEL, by the bit-for-bit comparison and
# by the oracle's recurrence over the float32 signal the stage was handed.
TRUTH_LEVEL = 0.005


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def adef(aw, preset):
    return aw.EqualizerDefinition(preset[0], [aw.EqualizerFilter(1, None, True, t, f, g, q) for t, f, g, q in preset[1]])


def odef(oracle, preset):
    return oracle.EqualizerDefinition(preset[0], [oracle.EqualizerFilter(1, None, True, t, f, g, q) for t, f, g, q in preset[1]])


def hrir(oracle):
    return oracle.synth_hrir(2, TAPS, seed=61)


def spatializer(aw, ctx, oracle, streams, stream_map=None, presets=PRESETS):
    sp = aw.Spatializer(aw.HRIR(hrir(oracle), sample_rate=RATE, ctx=ctx), LT, RT, n_streams=streams, ctx=ctx)
    if stream_map is not None:
        sp.set_equalizer([adef(aw, p) for p in presets], stream_map)
    return sp


def two_call(aw, ctx, y_calls, stream_map, presets=PRESETS):
    """The path the stage replaces: ParametricEqualizerState of every preset over its streams of the calls' float32 outputs."""
    outs = [np.array(y, np.float32) for y in y_calls]
    for p, preset in enumerate(presets):
        idx = [s for s, m in enumerate(stream_map) if m == p]
        if not idx:
            continue
        st = aw.ParametricEqualizerState(adef(aw, preset), RATE, n_streams=len(idx), ctx=ctx)
        for y, o in zip(y_calls, outs):
            o[idx] = st.process_batch(np.ascontiguousarray(y[idx]))
    return outs


def cut(x, calls):
    at = np.concatenate([[0], np.cumsum(calls)])
    return [np.ascontiguousarray(x[:, a:b]) for a, b in zip(at[:-1], at[1:])]


def noise(seed, streams, frames, level=LEVEL):
    return np.random.default_rng(seed).uniform(-level, level, (streams, frames, 2)).astype(np.float32)


def ear_split_off_context(aw, torch):
    old = os.environ.get("AW_EQ_EAR_SPLIT")
    os.environ["AW_EQ_EAR_SPLIT"] = "0"                    # knobs are read once, at context creation
    try:
        return aw.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    finally:
        if old is None:
            del os.environ["AW_EQ_EAR_SPLIT"]
        else:
            os.environ["AW_EQ_EAR_SPLIT"] = old


# ---- 1. the two-call path, bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["ear_per_workgroup", "both_ears"])
@pytest.mark.parametrize("calls", [[31, 32, 33, 64], [8191, 8192, 8193], [10000, 3, 70000]])
def test_stage_equals_the_two_call_path_bit_for_bit(oracle, calls, form):
    """At LEVEL: bit equality with the two-call path, and every sample within ULP of the oracle's sequential recurrence over the float32
    output the stage was handed (the stage-off output: the same bits).  At TRUTH_LEVEL (see there): within ULP of the oracle over the
    float64 truth's convolution."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch) if form == "ear_per_workgroup" else ear_split_off_context(aw, torch)
    S = len(MAP9)
    h = hrir(oracle)
    for level in (LEVEL, TRUTH_LEVEL):
        xs = cut(noise(sum(calls), S, sum(calls), level), calls)
        plain, staged = spatializer(aw, ctx, oracle, S), spatializer(aw, ctx, oracle, S, MAP9)
        assert staged.info()["equalizer"] == 3 and staged.info()["equalizer_filters"] == 64 and plain.info()["equalizer"] == 0
        ys = [plain.process(x) for x in xs]
        got = [staged.process(x) for x in xs]
        want = two_call(aw, ctx, ys, MAP9)
        for n, g, w, y in zip(calls, got, want, ys):
            for s, m in enumerate(MAP9):
                assert np.array_equal(bits(g[s]), bits(w[s])), (level, n, s, m)
                if m < 0:
                    assert np.array_equal(bits(g[s]), bits(y[s])), (level, n, s)
        whole_x, whole_y, whole_in = np.concatenate(xs, axis=1), np.concatenate(got, axis=1), np.concatenate(ys, axis=1)
        for s in (0, 1, 2):                                          # one stream per preset
            if level == LEVEL:
                src, what = whole_in[s], "the stage's own float32 input"
            else:
                src, what = oracle.spatialize_f64(whole_x[s], h, LT, RT).astype(np.float32), "the float64 truth's convolution"
            el, er = oracle.eq_prepare(odef(oracle, PRESETS[MAP9[s]]), RATE).process(src[:, 0], src[:, 1])
            err = max(np.max(np.abs(whole_y[s, :, 0] - el)), np.max(np.abs(whole_y[s, :, 1] - er)))
            print(f"calls {calls} {form} stream {s} preset {MAP9[s]}: max |y - oracle over {what}| = {err:.3e}, peak {np.abs(whole_y[s]).max():.3f}")
            assert err <= ULP, (level, s, err)


# ---- 2. chunking, formats, sharding, the page-locked path, cuts in time ------------------------------------------------------------------

def test_chunking_formats_and_sharding_change_no_bit(oracle):
    import torch
    import airwave_amd as aw
    S, F = 9, 40003                                                  # 320 KB of input per stream: AW_HOST_CHUNK_MB=1 takes three streams a chunk
    ctx, small = context(aw, torch, chunk_mb=64), context(aw, torch, chunk_mb=1)
    x16 = np.clip(np.rint(np.random.default_rng(81).uniform(-LEVEL, LEVEL, (S, F, 2)) * 32768), -32768, 32767).astype(np.int16)
    x = x16.astype(np.float32) / np.float32(32768.0)                 # the decoded samples
    one = device_call(torch, spatializer(aw, ctx, oracle, S, MAP9), x)
    assert np.array_equal(bits(one), bits(two_call(aw, ctx, [device_call(torch, spatializer(aw, ctx, oracle, S), x)], MAP9)[0]))
    sp_c = spatializer(aw, small, oracle, S, MAP9)
    chunked = host_call(sp_c, x)
    cs = sp_c.info()["host_chunk_streams"]
    assert 0 < cs and -(-S // cs) == 3, cs
    assert chunked.tobytes() == one.tobytes()
    # s16 in / f32 out, on the device and (chunked) through the host entry
    sp16 = spatializer(aw, ctx, oracle, S, MAP9)
    xd, yd = to_dev(torch, x16), torch.empty(one.nbytes, dtype=torch.uint8, device="cuda")
    sp16.process_pcm_device(xd.data_ptr(), "s16", yd.data_ptr(), "f32", F)
    torch.cuda.synchronize()
    assert from_dev(yd, one).tobytes() == one.tobytes()
    y16 = out_host(F32, S, F)
    spatializer(aw, small, oracle, S, MAP9).process_host_into(x16, y16, in_format="s16", out_format="f32")
    assert y16.tobytes() == one.tobytes()
    # two handles of 4 + 5 streams, the map cut accordingly
    shards = [device_call(torch, spatializer(aw, ctx, oracle, k, MAP9[first:first + k]), x[first:first + k]) for first, k in ((0, 4), (4, 5))]
    assert np.concatenate(shards).tobytes() == one.tobytes()


def test_single_stream_callback_path_equals_the_stream_inside_a_batch(oracle):
    """One stream, callback-sized calls of the host entry: the stage's kernels run in place over the page-locked output.  Held without
    condition: the page-locked path's stage equals the two-call path over that path's own stage-off output, bit for bit.  Equality with
    the same stream inside a batch is held where the parent's convolution kernels wrote the same bits on both paths (they did, on every
    run so far; the condition is the one tests/test_gpu_true_peak.py makes): where they do not, no equalizer behind them can."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    calls = [4096, 3, 100, 33]
    x = noise(82, 3, sum(calls))
    for preset in (0, 1):
        batch_map = [2, preset, -1]
        got = {}
        for name, streams, first in (("callback", 1, 1), ("batch", 3, 0)):
            m = batch_map[first:first + streams]
            plain, staged = spatializer(aw, ctx, oracle, streams), spatializer(aw, ctx, oracle, streams, m)
            for sp in (plain, staged):
                if name == "callback":
                    sp.reserve_host(4096)
            xs = cut(x[first:first + streams], calls)
            ys = [host_call(plain, c) for c in xs]
            zs = [host_call(staged, c) for c in xs]
            if name == "callback":
                assert staged.info()["host_chunk_streams"] == 0
            want = two_call(aw, ctx, ys, m)
            assert np.array_equal(bits(np.concatenate(zs, axis=1)), bits(np.concatenate(want, axis=1))), (name, preset)
            got[name] = (np.concatenate(ys, axis=1), np.concatenate(zs, axis=1))
        same = np.array_equal(bits(got["callback"][0]), bits(got["batch"][0][1:2]))
        print(f"preset {preset}: the page-locked path's convolution wrote the batch's bits: {same}")
        if same:                                                     # (the convolution kernels of the two paths are the parent's)
            assert got["callback"][1].tobytes() == got["batch"][1][1:2].tobytes()


def test_cutting_a_call_in_time_stays_within_an_ulp(oracle):
    """Chunk boundaries move with the cut: Float64 reassociation, at most the last bit of the float32 output.  The convolution kernels in
    front of the stage depend on the cut themselves (at LEVEL their two outputs are 2.7e-7 apart at a peak of 0.25, 4.5 x ULP before the
    equalizer has run), so the signal has TRUTH_LEVEL here for the reason given there: what the absolute bound then catches is a state that
    is not carried over the cut, or carried into the wrong row."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, F = 4, 8256
    m = [0, 1, 2, 0]
    x = noise(83, S, F, TRUTH_LEVEL)
    whole = spatializer(aw, ctx, oracle, S, m).process(x)
    parts = spatializer(aw, ctx, oracle, S, m)
    got = np.concatenate([parts.process(c) for c in cut(x, [100, 8156])], axis=1)
    plain_whole = spatializer(aw, ctx, oracle, S).process(x)
    plain_parts = spatializer(aw, ctx, oracle, S)
    conv = np.max(np.abs(np.concatenate([plain_parts.process(c) for c in cut(x, [100, 8156])], axis=1) - plain_whole))
    err = np.max(np.abs(got - whole))
    print(f"one call of {F} against [100, 8156]: max difference {err:.3e} (the convolution alone: {conv:.3e})")
    assert err <= ULP


# ---- 3. order in the chain -------------------------------------------------------------------------------------------------------------

def test_every_later_stage_sees_the_equalized_signal(oracle):
    """Metering, loudness, true peak, AW_GAIN_FIXED, the limiter and s24 output behind the stage, each against the reference the project
    holds that stage to, applied to the two-call path's output (the stage-off output through ParametricEqualizerState): the s24 output
    is the limiter's sequential rule (tests/emu/emu_limiter.cpp) encoded by numpy, bit for bit, with the limiter's records; the level
    meter's peak is that signal's peak exactly; the true-peak records are the header's sequential rule (tests/emu/emu_true_peak.cpp),
    bit for bit; the loudness hops are the float64 recurrence's within the project's reassociation bound.  (A second spatializer cannot
    stand in for those references: the parent has no entry that feeds stereo to the stages without a convolution, and a unit impulse
    through its FFT kernels returns its input only to 8e-7, on no stream exactly.)"""
    import torch
    import airwave_amd as aw
    import emu_limiter
    import emu_true_peak
    ctx = context(aw, torch)
    S, F = 5, 24000                                                  # half a second: two gating blocks of the loudness measurement
    m = [0, 1, 2, -1, 2]
    c, L, H = 0.5, 64, 128
    x = noise(84, S, F)
    y = spatializer(aw, ctx, oracle, S).process(x)
    x[4] *= np.float32(0.4 / np.abs(y[4]).max())                    # stream 4 (preset C, +6 dB) peaks at 0.4 in front of the stage
    y = spatializer(aw, ctx, oracle, S).process(x)
    assert abs(np.abs(y[4]).max() - 0.4) < 1e-3
    y_eq = two_call(aw, ctx, [y], m)[0]
    gains = np.array([1.5, 1.2, 0.9, 1.0, 0.7], np.float32)

    def stages(sp):
        sp.set_metering(True)
        sp.set_loudness(True, 10.0)
        sp.set_true_peak(True)
        sp.set_gain("fixed", gains)
        sp.set_limiter(True, c, L, H)
        return sp

    staged = stages(spatializer(aw, ctx, oracle, S, m))
    out = device_call(torch, staged, x, S24)
    lv, ld, tp, lim = staged.levels(), staged.loudness(), staged.true_peak(), staged.limiter()
    # the meter sits behind the stage: +6 dB on a stream that peaks at 0.4
    assert abs(lv["peak"][4].max() - 0.4 * 10 ** (6 / 20)) < 2e-3 and abs(lv["peak"][4].max() - 0.4) > 0.3
    assert np.array_equal(lv["peak"], np.abs(y_eq).max(axis=1))
    rule = emu_limiter.Limiter(S, L, H, c, gains)
    z = rule.process(y_eq)
    assert out.tobytes() == encode(S24, z)[0].tobytes()
    assert np.array_equal(lim["min_gain"].view(np.uint32), rule.min_gain) and np.array_equal(lim["limited_frames"], rule.limited)
    # true peak: the header's sequential rule (tests/emu/emu_true_peak.cpp, what tests/test_gpu_true_peak.py holds the device to) over
    # the two-call path's output, bit for bit
    meter = emu_true_peak.Meter(S, False)
    meter.process(y_eq)
    assert np.array_equal(tp["true_peak"].view(np.uint32), meter.tp) and np.array_equal(tp["call_true_peak"].view(np.uint32), meter.call)
    assert np.array_equal(tp["nonfinite"], meter.nonfinite) and np.all(tp["frames"] == F) and not tp["reserved"].any()
    # loudness: no bit-exact rule exists for it (the hop sums' order is the kernel's): the hop energies of the two-call path's output by
    # the frame-by-frame float64 recurrence, within the project's reassociation bound, the gating counts equal, the integrated figure
    # within 4.35 x that bound (tests/test_gpu_loudness.py)
    want_hops, want_bad = reference_hops(y_eq, int(RATE))
    check_against_reference(ld, all_hops(staged, want_hops.shape[1]), want_hops, int(RATE), "behind the stage")
    assert np.array_equal(ld["nonfinite"], want_bad) and np.all(ld["frames"] == F) and np.all(np.isfinite(ld["integrated_lufs"]))
    assert np.all(lim["frames"] == F) and np.all(lv["frames"] == F)
    # ... and they are NOT what the unequalized signal gives
    plain_meter = emu_true_peak.Meter(S, False)
    plain_meter.process(y)
    assert all(not np.array_equal(meter.tp[s], plain_meter.tp[s]) for s in (0, 1, 2, 4)) and np.array_equal(meter.tp[3], plain_meter.tp[3])


# ---- 4. off means off; refusals; lifecycle ---------------------------------------------------------------------------------------------

def test_off_means_off_refusals_and_lifecycle(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, F = 5, 4131                                                   # whole chunks and a tail: both kernels run
    m = [0, -1, 1, 0, 2]
    x = noise(85, S, F)
    names = lambda sp: [n for n, _, _ in sp.stage_times()]
    for fout in (F32, S16):
        plain, switched = spatializer(aw, ctx, oracle, S), spatializer(aw, ctx, oracle, S, m)
        switched.set_equalizer([])
        assert switched.info()["equalizer"] == 0 and switched.info()["equalizer_filters"] == 0
        for sp in (plain, switched):
            sp.set_metering(True)
            sp.set_profiling(True)
        for run in (lambda sp: device_call(torch, sp, x, fout), lambda sp: host_call(sp, x, fout)):
            assert run(plain).tobytes() == run(switched).tobytes()
        ctx.synchronize()
        assert names(plain) == names(switched)
        assert "aw_eq_stage_kernel" not in names(switched) and "aw_eq_stage_tail_kernel" not in names(switched)
        for field in ("peak", "frames", "clipped", "nonfinite"):    # (the energies are sums whose order is free: device/levels.hpp)
            assert np.array_equal(plain.levels()[field], switched.levels()[field]), field
    sp = spatializer(aw, ctx, oracle, S, m)
    assert sp.info()["equalizer"] == 3 and sp.info()["equalizer_filters"] == 64
    sp.reserve_pcm(F, "f32", "s16")
    sp.set_profiling(True)
    first = device_call(torch, sp, x)
    host_call(sp, x, S16)
    ctx.synchronize()
    assert "aw_eq_stage_kernel" in names(sp) and "aw_eq_stage_tail_kernel" in names(sp)
    allocs = sp.info()["device_allocs"]
    for _ in range(5):
        device_call(torch, sp, x)
        host_call(sp, x, S16)
    assert sp.info()["device_allocs"] == allocs
    # reset: the filter state (and the convolution's history) start over
    sp.reset()
    assert np.array_equal(bits(device_call(torch, sp, x)), bits(first))
    second = device_call(torch, sp, x)                                # (state carried: other bits)
    assert not np.array_equal(bits(second), bits(first))
    # a second setter call zeroes the state: behind the same convolution history the output is the two-call path's from fresh states
    plain = spatializer(aw, ctx, oracle, S)
    ys = [device_call(torch, plain, x) for _ in range(3)]
    sp.reset()
    device_call(torch, sp, x)
    device_call(torch, sp, x)
    sp.set_equalizer([adef(aw, p) for p in PRESETS], m)
    assert np.array_equal(bits(device_call(torch, sp, x)), bits(two_call(aw, ctx, [ys[2]], m)[0]))
    # off: the names are gone again
    sp.set_equalizer(None)
    sp.set_profiling(True)
    assert np.array_equal(bits(device_call(torch, sp, x)), bits(device_call(torch, plain, x)))
    ctx.synchronize()
    assert "aw_eq_stage_kernel" not in names(sp) and "aw_eq_stage_tail_kernel" not in names(sp)

    # refusals: each returns its status and leaves the old stage working
    sp = spatializer(aw, ctx, oracle, S, m)
    plain = spatializer(aw, ctx, oracle, S)
    lib = sp._lib
    fn = lib.aw_spatializer_set_equalizer
    handles = [adef(aw, p)._handle() for p in PRESETS]
    bad_filter = aw.EqualizerDefinition(0.0, [aw.EqualizerFilter(7, None, True, 0, 1000.0, 1.0, 1.0), aw.EqualizerFilter(9, None, True, 0, 30000.0, 1.0, 1.0)])._handle()
    too_many = aw.EqualizerDefinition(0.0, [aw.EqualizerFilter(1, None, True, 0, 500.0 + i, 1.0, 1.0) for i in range(65)])._handle()
    huge = aw.EqualizerDefinition(1e9, [])._handle()
    try:
        arr = lambda hs: ctypes.cast((ctypes.c_void_p * len(hs))(*hs), ctypes.POINTER(ctypes.c_void_p))
        imap = lambda v: (ctypes.c_int32 * len(v))(*v)
        calls = 0

        def still_works():
            nonlocal calls
            assert sp.info()["equalizer"] == 3 and sp.info()["equalizer_filters"] == 64
            y = device_call(torch, plain, x)
            got = device_call(torch, sp, x)
            if calls == 0:
                assert np.array_equal(bits(got), bits(two_call(aw, ctx, [y], m)[0]))
            for s in (1,):
                assert np.array_equal(bits(got[s]), bits(y[s]))
            assert not np.array_equal(bits(got[0]), bits(y[0]))
            calls += 1

        assert fn(None, arr(handles), 3, None) == 1
        assert fn(sp._h, arr(handles), -1, None) == 1
        still_works()
        assert fn(sp._h, None, 2, None) == 1
        assert fn(sp._h, arr([handles[0], None]), 2, None) == 1
        still_works()
        for bad in ([0, 1, 2, 3, 0], [0, 1, -2, 0, 0]):
            assert fn(sp._h, arr(handles), 3, imap(bad)) == 1
        still_works()
        assert fn(sp._h, arr([handles[0], bad_filter]), 2, None) == 16                  # AW_ERR_EQ_INVALID_FILTER
        msg = lib.aw_last_error_message()
        assert b"Filter 2 is invalid" in msg and b"(definition 1)" in msg, msg
        idx, kind, line = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        assert lib.aw_last_eq_filter_error(ctypes.byref(idx), ctypes.byref(kind), ctypes.byref(line)) == 1
        assert (idx.value, kind.value, line.value) == (1, 2, 9)
        assert fn(sp._h, arr([too_many]), 1, None) == 15                                # AW_ERR_EQ_TOO_MANY_FILTERS
        assert fn(sp._h, arr([handles[0], handles[1], huge]), 3, None) == 14            # AW_ERR_EQ_NON_FINITE_PREAMP
        assert b"(definition 2)" in lib.aw_last_error_message()
        still_works()
        # (no `pytest.raises(...) as e` here: the traceback it keeps would hold this frame's handles in a cycle, and the cyclic collector
        # finalises a Context before the Spatializer that still points to it)
        refused = None
        try:
            sp.set_equalizer([adef(aw, A), aw.EqualizerDefinition(0.0, [aw.EqualizerFilter(9, None, True, 0, 30000.0, 1.0, 1.0)])])
        except aw.ParametricEqualizerPreparationError as err:
            refused = (err.kind, err.filter_error, err.source_line)
        assert refused == ("invalidFilter", "invalidFrequency", 9)
        with pytest.raises(ValueError):
            sp.set_equalizer([adef(aw, A)], [0, 0])                                      # one entry per stream
        still_works()
    finally:
        for h in handles + [bad_filter, too_many, huge]:
            lib.aw_eq_definition_destroy(h)


# ---- 6. mixed-rate batches -------------------------------------------------------------------------------------------------------------

def test_mixed_rate_batch_with_one_equalizer_per_stream(oracle):
    import airwave_amd as aw
    rates = [48000.0, 44100.0, 48000.0, 44100.0]
    da, db = adef(aw, A), adef(aw, B)
    eqs = [da, None, db, adef(aw, A)]                                 # (an equal definition is the same preset)
    h7 = oracle.synth_hrir(7, TAPS, seed=62)
    layout = aw.InputLayout.detect(2)
    with pytest.raises(ValueError):
        aw.MixedRateBatch(h7, 48000.0, layout, rates, equalizer=da, stream_equalizers=eqs)
    batch, plain = aw.MixedRateBatch(h7, 48000.0, layout, rates, stream_equalizers=eqs), aw.MixedRateBatch(h7, 48000.0, layout, rates)
    assert [batch.buckets[r].spatializer.info()["equalizer"] for r in (48000.0, 44100.0)] == [2, 1]
    assert all(b.equalizer is None for b in batch.buckets.values())
    F = {48000.0: 5003, 44100.0: 4100}
    rng = np.random.default_rng(86)
    streams = [rng.uniform(-LEVEL, LEVEL, (F[r], 2)).astype(np.float32) for r in rates]
    got, ys = batch.process(streams, rates), plain.process(streams, rates)
    for i, (r, d) in enumerate(zip(rates, eqs)):
        want = ys[i] if d is None else aw.ParametricEqualizerState(d, r, n_streams=1).process_batch(ys[i][None])[0]
        assert np.array_equal(bits(got[i]), bits(want)), i
