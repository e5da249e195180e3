"""The converter's true-peak entries on the device (aw_tp_rateconv_*, RateConverter.set_true_peak and friends): bit-for-bit parity of the
records and of the output bytes with the composition of the separately tested rules (tests/emu/emu_rateconv_tp.py, plain g++), through
process and through measure; the invariances the rule promises (calls cut in time, streams sharded over handles, buffers at odd bytes);
the contract of the entries; the float32 family untouched; and the ceiling pass, whose output must read at most c (1 + 2^-16) by the
float64 reference: each reading makes at most 13 roundings of 2^-24 (12 fmaf steps and the gain's product) on sums whose absolute
coefficients add to less than 4, and there are two readings, so the excess is below 2 * 13 * 4 * 2^-24 < 2^-16 of the peak."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402
import emu_rateconv_pcm as pcm  # noqa: E402
import emu_rateconv_tp as tp  # noqa: E402
import true_peak_ref as ref  # noqa: E402
from emu_rateconv_pcm import F32, S16, S24, NONE, TPDF  # noqa: E402
from test_emu_rateconv_tp import call_lengths, exact_cuts  # noqa: E402
from test_gpu_rateconv_pcm import device, flush, output, process, refused  # noqa: E402

pytestmark = pytest.mark.gpu

STREAMS = 3
SEED = 0x5EED0123456789AB
FIRST = 11
GAINS = [0.5, 1.25, 0.8]
SHAPES = [((44100, 48000), 2), ((96000, 44100), 2), ((48000, 96000), 3), ((192000, 44100), 16)]
SHORT = ((48000, 8000), 16)                               # a measuring tile of 5 outputs: a tile's predecessors span two earlier tiles and the history
CEILING = 0.891
_cases = {}


class Env:
    pass


@pytest.fixture(scope="module")
def G():
    import torch
    import airwave_amd as aw
    g = Env()
    g.torch, g.aw = torch, aw
    g.ctx = aw.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    return g


def converter(G, pair, S, C, dither=NONE, gains=None, first=FIRST, true_peak=True, metering=True):
    rc = G.aw.RateConverter(pair[0], pair[1], S, C, ctx=G.ctx)
    rc.set_dither(dither, SEED, first)
    if gains is not None:
        rc.set_gain("fixed", gains)
    if metering:
        rc.set_metering(True)
    if true_peak:
        rc.set_true_peak(True)
    return rc


def same(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


def measure(G, rc, x, fi, shift=0):
    keep, p_in = device(G, x, shift)
    n = rc.measure_device(p_in, fi, x.shape[1])
    G.torch.cuda.synchronize()
    del keep
    return n


def case(pair, C):
    """The calls of tests/test_emu_rateconv_tp.py (s16 in, s24 out, TPDF, fixed gains) of STREAMS streams, what the composition makes of
    them and its records after every call and after the flush; computed once, left unchanged."""
    key = (pair, C)
    if key not in _cases:
        rng = np.random.default_rng(pair[0] + C)
        xs = [pcm.random_input(rng, (STREAMS, n, C), S16) for n, _, _ in call_lengths(pair, C)]
        q = tp.Composition(pair[0], pair[1], STREAMS, C, TPDF, SEED, FIRST, GAINS)
        want, records, levels = [], [], []
        for run in [lambda x=x: q.process(x, S16, S24) for x in xs] + [lambda: q.flush(S24)]:
            want.append(run())
            records.append(q.records.copy())
            levels.append(q.levels.copy())
        for a in (*xs, *want, *records, *levels):
            a.setflags(write=False)
        _cases[key] = (xs, want, records, levels)
    return _cases[key]


@pytest.mark.parametrize("pair,C", SHAPES + [SHORT], ids=str)
def test_device_equals_the_composition_through_process_and_through_measure(G, pair, C):
    check_process_and_measure(G, pair, C)


def check_process_and_measure(G, pair, C):
    """The calls of case(pair, C) and the flush through process, then through measure and measure_flush: bytes, true-peak records and
    levels after every call against the composition."""
    xs, want, records, levels = case(pair, C)
    rc = converter(G, pair, STREAMS, C, TPDF, GAINS)
    info = rc.info()
    assert info["true_peak"] == 1 and info["true_peak_tile"] == tp.tp_tile(pair[0], pair[1], C) == info["tile"] - 11
    for i, x in enumerate(xs):
        got = process(G, rc, x, S16, S24, shift=i % 4, out_shift=(2 * i + 1) % 4)
        assert got.shape == want[i].shape and np.array_equal(got, want[i]), (pair, C, i)
        assert same(rc.true_peak(), records[i]) and same(rc.levels(), levels[i]), (pair, C, i, rc.true_peak(), records[i])
    assert sum(w.shape[1] for w in want[:-1]) > 2 * info["true_peak_tile"]             # three workgroups per stream, the last ragged
    assert np.array_equal(flush(G, rc, S24), want[-1])
    assert same(rc.true_peak(), records[-1]) and same(rc.levels(), levels[-1])         # the flush reset the counts and left the records
    assert rc.info()["frames_consumed"] == 0 and rc.info()["frames_produced"] == 0
    assert same(rc.true_peak(1, 2), records[-1][1:3])
    # the same through measure: the same records, the same counts, and no levels record
    rc.reset_true_peak()
    rc.reset_levels()
    assert not rc.true_peak().view(np.uint8).any()
    for i, x in enumerate(xs):
        assert measure(G, rc, x, S16, shift=(i + 1) % 4) == want[i].shape[1]
        assert same(rc.true_peak(), records[i]), (pair, C, i)
    assert rc.info()["frames_produced"] == sum(w.shape[1] for w in want[:-1])
    assert rc.measure_flush_device() == want[-1].shape[1]
    assert same(rc.true_peak(), records[-1]) and not rc.levels().view(np.uint8).any()
    assert rc.info()["frames_consumed"] == 0 and rc.info()["frames_produced"] == 0
    # pass two starts clean: the composition's first bytes again
    assert np.array_equal(process(G, rc, xs[0], S16, S24), want[0])
    rc.close()


def test_measure_then_process_writes_what_process_then_process_writes(G):
    pair, C = (96000, 44100), 2
    xs, want, records, levels = case(pair, C)
    rc = converter(G, pair, STREAMS, C, TPDF, GAINS)
    assert measure(G, rc, xs[0], S16) == want[0].shape[1]
    assert np.array_equal(process(G, rc, xs[1], S16, S24), want[1]) and same(rc.true_peak(), records[1])
    rc.close()


@pytest.mark.parametrize("pair,C", [((44100, 48000), 2), ((192000, 44100), 16)], ids=str)
def test_invariances_change_no_bit(G, pair, C):
    xs, want, records, levels = case(pair, C)
    whole = np.concatenate(want, axis=1)
    big = max(xs, key=lambda a: a.shape[1])
    L, M, T, D = emu.plan(*pair)
    tile = tp.tp_tile(pair[0], pair[1], C)
    # buffers at odd bytes
    for shift in (1, 3):
        rc = converter(G, pair, STREAMS, C, TPDF, GAINS)
        y = np.concatenate([process(G, rc, x, S16, S24, shift, (shift + 2) % 4) for x in xs] + [flush(G, rc, S24)], axis=1)
        assert np.array_equal(y, whole) and same(rc.true_peak(), records[-1]), shift
        rc.close()
    # calls cut in time at ragged points: chunks of 1, 10, 11 and 12 outputs and one of tile - 1
    chunks = [1, 10, 11, 12, tile - 1]
    cuts = exact_cuts(pair, C, chunks)
    assert cuts is not None and cuts[-1] < big.shape[1]
    cuts = [0] + cuts + [big.shape[1]]
    q = tp.Composition(pair[0], pair[1], STREAMS, C, TPDF, SEED, FIRST, GAINS)
    y_whole = q.process(big, S16, S24)
    rc = converter(G, pair, STREAMS, C, TPDF, GAINS)
    parts = [process(G, rc, np.ascontiguousarray(big[:, a:b]), S16, S24) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [p.shape[1] for p in parts[1:1 + len(chunks)]] == chunks
    assert np.array_equal(np.concatenate(parts, axis=1), y_whole) and same(rc.true_peak(), q.records) and same(rc.levels(), q.levels)
    rc.close()
    # streams sharded over two handles
    ys, recs = [], []
    for a, b in ((0, 1), (1, 3)):
        rc = converter(G, pair, b - a, C, TPDF, GAINS[a:b], first=FIRST + a)
        ys.append(np.concatenate([process(G, rc, np.ascontiguousarray(x[a:b]), S16, S24) for x in xs] + [flush(G, rc, S24)], axis=1))
        recs.append(rc.true_peak())
        rc.close()
    assert np.array_equal(np.concatenate(ys, axis=0), whole) and same(np.concatenate(recs), records[-1])


def test_contract_of_the_entries(G):
    torch, aw = G.torch, G.aw
    pair, C, S = (44100, 48000), 2, STREAMS
    xs, want, records, levels = case(pair, C)
    x = max(xs, key=lambda a: a.shape[1])
    lib = aw._capi.load()
    meter = aw.Spatializer(aw.HRIR(np.ones((2, 8), np.float32), 48000.0, ctx=G.ctx), [0, 1], [1, 0], 1, ctx=G.ctx)
    allocs = lambda: meter.info()["device_allocs"]          # noqa: E731
    a0 = allocs()
    rc = aw.RateConverter(pair[0], pair[1], S, C, ctx=G.ctx)
    assert allocs() == a0 + 4                                                       # create allocates what it did
    assert rc.info()["true_peak"] == 0 and rc.info()["true_peak_tile"] == rc.info()["tile"] - 11
    # never switched on: get is refused; measuring off: measure is refused and leaves the counts
    assert refused(G, rc.true_peak) == "INVALID_ARGUMENT"
    keep, p_in = device(G, x)
    n = x.shape[1]
    assert refused(G, rc.measure_device, p_in, S16, n) == "INVALID_ARGUMENT" and refused(G, rc.measure_flush_device) == "INVALID_ARGUMENT"
    assert rc.info()["frames_consumed"] == 0 and rc.info()["frames_produced"] == 0
    rc.reset_true_peak()                                                            # (nothing to zero: no error, no allocation)
    assert allocs() == a0 + 4
    rc.set_true_peak(True)
    assert allocs() == a0 + 5 and rc.info()["true_peak"] == 1                       # set(on) allocates once ...
    rc.set_true_peak(False)
    rc.set_true_peak(True)
    rc.set_true_peak(True)
    assert allocs() == a0 + 5
    assert not rc.true_peak().view(np.uint8).any()
    # refusals before any HIP call write nothing and leave the counts
    n64 = ctypes.c_int64(-7)
    call = lambda *a: lib.aw_tp_rateconv_measure(rc._h, *a, ctypes.byref(n64))          # noqa: E731
    assert call(ctypes.c_void_p(p_in), 4, n) == 1 and call(ctypes.c_void_p(p_in), -1, n) == 1
    assert call(None, S16, n) == 1 and call(ctypes.c_void_p(p_in), S16, -1) == 1
    assert n64.value == -7 and rc.info()["frames_consumed"] == 0
    out = np.zeros(S + 1, aw.rateconv.RATECONV_TRUE_PEAK_DTYPE)
    for bad in ((-1, 1), (2, 2), (0, S + 1)):
        assert lib.aw_tp_rateconv_get(rc._h, bad[0], bad[1], ctypes.c_void_p(out.ctypes.data)) == 1
    assert lib.aw_tp_rateconv_get(rc._h, 0, 1, None) == 1 and not out.view(np.uint8).any()
    assert call(ctypes.c_void_p(p_in), S16, 0) == 0 and n64.value == 0 and rc.info()["frames_consumed"] == 0          # an empty call is no error
    # ... and no later call allocates: the library's own count, then (every kernel loaded) the device's free memory
    n_out = rc.output_frames(n)
    t, p_out = output(G, S * (n_out + 100) * C * 4)
    rc.measure_device(p_in, S16, n)
    rc.measure_flush_device()
    rc.process_pcm_device(p_in, S16, n, p_out, S24, n_out)
    rc.flush_pcm_device(p_out, S24, 100)
    torch.cuda.synchronize()
    a1, free0 = allocs(), torch.cuda.mem_get_info()[0]
    assert a1 == a0 + 5
    for fo in (S16, F32):
        rc.measure_device(p_in, S16, n)
        rc.measure_flush_device()
        rc.process_pcm_device(p_in, S16, n, p_out, fo, n_out)
        rc.flush_pcm_device(p_out, fo, 100)
        rc.reset_true_peak()
        rc.true_peak()
        rc.reset()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0
    assert allocs() == a1
    # switched off: the records stay readable and stay as they are
    rc.process_pcm_device(p_in, S16, n, p_out, S24, n_out)
    before = rc.true_peak()
    assert before["frames"][0] == n_out
    rc.set_true_peak(False)
    rc.process_pcm_device(p_in, S16, n, p_out, S24, rc.output_frames(n))
    assert same(rc.true_peak(), before) and rc.info()["true_peak"] == 0
    rc.close()
    del keep, t


def test_the_float32_entries_are_untouched_and_unseen(G):
    pair, C, S = (44100, 48000), 2, STREAMS
    rng = np.random.default_rng(3)
    n = call_lengths(pair, C)[1][0]
    x, x7 = (0.25 * rng.standard_normal((S, n, C))).astype(np.float32), (0.25 * rng.standard_normal((S, 7, C))).astype(np.float32)
    off, on = G.aw.RateConverter(pair[0], pair[1], S, C, ctx=G.ctx), converter(G, pair, S, C)
    y_off = np.concatenate([off.process(x), off.process(x7), off.flush()], axis=1)
    y_on = np.concatenate([on.process(x), on.process(x7), on.flush()], axis=1)
    assert np.array_equal(y_off.view(np.uint32), y_on.view(np.uint32))
    assert not on.true_peak().view(np.uint8).any()                                  # the float32 family does not measure
    # aw_rateconv_reset zeroes the carried v: a measured stream after it reads what a fresh handle reads
    process(G, on, pcm.to_bytes(x, F32), F32, F32)
    on.reset()
    on.reset_true_peak()
    fresh = converter(G, pair, S, C)
    longer = pcm.to_bytes(x[:, :200], F32)
    process(G, on, longer, F32, F32)
    process(G, fresh, longer, F32, F32)
    assert same(on.true_peak(), fresh.true_peak()) and on.true_peak()["frames"][0] > 0
    for h in (off, on, fresh):
        h.close()


def ceiling_input(rate, frames):
    """[3][frames][2] float32: a loud fs/4-ish sine at 45 degrees (its samples under-read its peak), loud noise, and quiet noise (x 0.25)."""
    rng = np.random.default_rng(7)
    s = ref.faded_sine(rate, 12000.0, 45.0, 1.2, seconds=frames / rate, fade=0.005)[:frames]
    loud = (0.4 * rng.standard_normal((frames, 2))).astype(np.float32)
    quiet = (0.25 * 0.4 * rng.standard_normal((frames, 2))).astype(np.float32)
    return np.ascontiguousarray(np.stack([s, loud, quiet]), np.float32)


def library_filter(G):
    c = G.aw.true_peak_filter()
    assert c.shape == (3, 12) and c.dtype == np.float32
    assert np.abs(c.astype(np.float64)).sum(axis=1).max() < 4.0                     # what the margin's derivation rests on
    return c


def reads(y, c):
    """The float64 reference's true peak of every stream of y [streams][frames][2]."""
    return np.array([ref.measure(y[s], c)["peak"].max() for s in range(y.shape[0])])


def test_the_ceiling_pass_holds_the_ceiling(G):
    pair, C, S = (44100, 48000), 2, 3
    c = library_filter(G)
    x = ceiling_input(pair[0], 4410)
    rc = converter(G, pair, S, C, TPDF, None, first=0, metering=True)
    assert rc.measure(x) == rc.info()["frames_produced"] > 0
    rc.measure_flush_device()
    rec = rc.true_peak()
    g = rc.ceiling_gains(CEILING)
    print("measured true peaks:", rec["true_peak"], "sample peaks:", rec["sample_peak"], "gains:", g)
    assert np.all(rec["true_peak"][:2] > CEILING) and rec["true_peak"][2] < CEILING and rec["true_peak"][0] > 1.1 * rec["sample_peak"][0]
    assert np.all(g[:2] < 1.0) and g[2] == 1.0 and g.dtype == np.float32
    assert all(g[s] == tp.ceiling_gain(rec["true_peak"][s], CEILING) for s in range(S))
    rc.set_gain("fixed", g)
    y = np.concatenate([rc.process_pcm(x, "f32")[0], rc.flush_pcm("f32")[0]], axis=1)
    got = reads(y, c)
    print("delivered true peaks:", got, "bound:", CEILING * (1 + 2.0 ** -16))
    assert np.all(got <= np.float32(CEILING).astype(np.float64) * (1.0 + 2.0 ** -16))
    assert np.all(got[:2] >= CEILING * (1.0 - 2.0 ** -16))                          # the ceiling binds: they sit at it
    assert abs(got[2] - float(rec["true_peak"][2])) <= 2.0 ** -16 * got[2]          # gain exactly 1: what was measured
    # the same pass to dithered s16: nothing clips
    rc.reset_levels()
    y16, clipped = rc.process_pcm(x, "s16")
    tail, clipped_tail = rc.flush_pcm("s16")
    assert clipped == 0 and clipped_tail == 0 and not rc.levels()["clipped"].any()
    assert np.abs(y16.astype(np.int32)).max() > 0.5 * 32768 and tail.dtype == np.int16
    rc.close()


def test_convert_with_a_true_peak_ceiling(G):
    pair = (44100, 48000)
    c = library_filter(G)
    x = ceiling_input(pair[0], 4410)
    bound = np.float32(CEILING).astype(np.float64) * (1.0 + 2.0 ** -16)
    y = G.aw.convert(x, pair[0], pair[1], ctx=G.ctx, out_format="f32", true_peak_ceiling=CEILING)
    plain = G.aw.convert(x, pair[0], pair[1], ctx=G.ctx, out_format="f32")
    got, was = reads(y, c), reads(plain, c)
    print("convert: before", was, "after", got)
    assert y.shape == plain.shape and np.all(was[:2] > CEILING) and np.all(got <= bound) and np.array_equal(y[2], plain[2])
    # with a caller's fixed gain: the smaller of the two per stream
    y = G.aw.convert(x, pair[0], pair[1], ctx=G.ctx, out_format="f32", true_peak_ceiling=CEILING, gains=[1.0, 0.25, 2.0])
    got = reads(y, c)
    assert was[1] < 3.5 and np.all(got <= bound) and abs(got[1] - 0.25 * was[1]) <= 1e-5 and np.array_equal(y[2], plain[2])
    with pytest.raises(ValueError):
        G.aw.convert(x, pair[0], pair[1], ctx=G.ctx, true_peak_ceiling=CEILING)


def test_mixed_rate_batch_with_an_output_true_peak_ceiling(G, golden_dir):
    aw = G.aw
    from test_gpu_full_size import SPEAKERS7
    w = aw.WAVLoader.load(os.path.join(golden_dir, "hrtf", "StageSH1.0.wav"))
    layout = aw.InputLayout(SPEAKERS7, "7 speakers")
    rates = [44100.0, 48000.0, 96000.0, 44100.0]
    frames = {44100.0: 3001, 48000.0: 3000, 96000.0: 5003}
    rng = np.random.default_rng(4)
    scale = [0.5, 0.5, 0.5, 0.01]
    streams = [(scale[i] * rng.standard_normal((frames[r], 7))).astype(np.float32) for i, r in enumerate(rates)]
    tracks = np.asarray(w.audio_data)
    c = library_filter(G)
    plain = aw.MixedRateBatch(tracks, w.sample_rate, layout, rates, ctx=G.ctx, output_rate=48000).process(streams, rates)
    batch = aw.MixedRateBatch(tracks, w.sample_rate, layout, rates, ctx=G.ctx, output_rate=48000, output_true_peak_ceiling=CEILING)
    y = batch.process(streams, rates)
    bound = np.float32(CEILING).astype(np.float64) * (1.0 + 2.0 ** -16)
    was = [ref.measure(p, c)["peak"].max() for p in plain]
    got = [ref.measure(p, c)["peak"].max() for p in y]
    print("batch: before", was, "after", got)
    assert was[0] > CEILING and was[2] > CEILING and was[3] < CEILING
    for i, r in enumerate(rates):
        assert y[i].shape == plain[i].shape
        if r == 48000.0:
            assert np.array_equal(y[i].view(np.uint32), plain[i].view(np.uint32))     # already at the output rate: left as it is
        else:
            assert got[i] <= bound, (i, got[i])
    assert np.array_equal(y[3].view(np.uint32), plain[3].view(np.uint32))             # under the ceiling: gain exactly 1
    batch.reset()
    assert np.array_equal(batch.process(streams, rates)[0], y[0])                     # a second call measures afresh
    with pytest.raises(ValueError):
        aw.MixedRateBatch(tracks, w.sample_rate, layout, rates, ctx=G.ctx, output_true_peak_ceiling=CEILING)
