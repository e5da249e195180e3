"""The converter's PCM entries on the device (aw_pcm_rateconv_*, RateConverter.process_pcm_device and friends): byte-for-byte and
field-for-field parity with the composition of the separately tested rules (tests/emu/emu_rateconv_pcm.cpp, built with plain g++), the
invariances the rule promises (calls cut in time, streams sharded over handles, buffers at any byte), the records and clipped_device, the
contract of the entries, stream order on a busy caller-owned stream, and the C example.  Shapes are tile-sized."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402
import emu_rateconv_pcm as pcm  # noqa: E402
from emu_rateconv_pcm import F32, S16, S24, S32, NONE, TPDF, TPDF_HP  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
STREAMS = 3
SEED = 0x5EED0123456789AB
FIRST = 11
GAINS = [0.5, 1.25, 0.8]
FORMS = {"s16-s16 tpdf": (S16, S16, TPDF, None), "s24-s24 tpdf_hp": (S24, S24, TPDF_HP, None), "f32-s16 gain": (F32, S16, NONE, GAINS),
         "s32-f32": (S32, F32, NONE, None), "f32-s32": (F32, S32, NONE, None)}
CASES = [((44100, 48000), 2, f) for f in sorted(FORMS)] + [((44100, 48000), 7, "s24-s24 tpdf_hp"), ((96000, 44100), 2, "s24-s24 tpdf_hp")]
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


@pytest.fixture(scope="module")
def delay(G):
    from test_gpu_stream_order import DELAY_MS, Delay
    return Delay(G.torch, DELAY_MS)


def device(G, b, shift=0):
    """The uint8 array b on the device, `shift` bytes past the allocation's (at least 16-byte) boundary, between sentinels."""
    t = G.torch.full((b.size + shift + 16,), SENTINEL, dtype=G.torch.uint8, device="cuda")
    t[shift:shift + b.size].copy_(G.torch.from_numpy(np.array(b, np.uint8).reshape(-1)))          # (a copy: the shared cases are read-only)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift


def output(G, nbytes, shift=0):
    t = G.torch.full((nbytes + shift + 16,), SENTINEL, dtype=G.torch.uint8, device="cuda")
    return t, t.data_ptr() + shift


def fetch(G, t, nbytes, shift=0):
    """(the nbytes written, everything behind them); the bytes in front must be untouched."""
    G.torch.cuda.synchronize()
    h = t.cpu().numpy()
    assert np.all(h[:shift] == SENTINEL)
    return h[shift:shift + nbytes].copy(), h[shift + nbytes:]


def converter(G, pair, S, C, dither=NONE, gains=None, first=FIRST, metering=True, ctx=None):
    rc = G.aw.RateConverter(pair[0], pair[1], S, C, ctx=ctx or G.ctx)
    rc.set_dither(dither, SEED, first)
    if gains is not None:
        rc.set_gain("fixed", gains)
    if metering:
        rc.set_metering(True)
    return rc


def process(G, rc, x, fi, fo, shift=0, out_shift=0, extra=3, clipped_ptr=0):
    """One aw_pcm_rateconv_process over the host bytes x [S][n][C][bytes] -> the host bytes; the capacity beyond the count stays untouched."""
    S, n, C, _ = x.shape
    keep, p_in = device(G, x, shift)
    want = rc.output_frames(n)
    nbytes = S * want * C * pcm.BYTES[fo]
    t, p_out = output(G, nbytes + extra * C * pcm.BYTES[fo], out_shift)
    made = rc.process_pcm_device(p_in, fi, n, p_out, fo, want + extra, clipped_ptr)
    assert made == want
    y, rest = fetch(G, t, nbytes, out_shift)
    assert np.all(rest == SENTINEL)
    del keep
    return y.reshape(S, made, C, pcm.BYTES[fo])


def flush(G, rc, fo, extra=3, clipped_ptr=0):
    S, C = rc.n_streams, rc.n_channels
    want = rc.flush_frames()
    nbytes = S * want * C * pcm.BYTES[fo]
    t, p_out = output(G, nbytes + extra * C * pcm.BYTES[fo])
    assert rc.flush_pcm_device(p_out, fo, want + extra, clipped_ptr) == want
    y, rest = fetch(G, t, nbytes)
    assert np.all(rest == SENTINEL)
    return y.reshape(S, want, C, pcm.BYTES[fo])


def case(pair, C, form, S=STREAMS, gains="form"):
    """(two tiles plus three frames, then seven) of S streams in the form's input format, what the composition makes of them, and its records
    after each of the three calls; computed once, left unchanged."""
    key = (pair, C, form, S, str(gains))
    if key not in _cases:
        fi, fo, dither, g = FORMS[form]
        g = g if gains == "form" else gains
        L, M, T, D = emu.plan(*pair)
        n = emu.input_frames_for(2 * emu.tile(pair[0], pair[1], C), L, M, D) + 3
        rng = np.random.default_rng(pair[0] + C + len(form))
        x, x7 = pcm.random_input(rng, (S, n, C), fi), pcm.random_input(rng, (S, 7, C), fi)
        q = pcm.Converter(pair[0], pair[1], S, C, False, dither, SEED, FIRST, None if g is None else (list(g) * S)[:S] if len(g) == 1 else g)
        want, levels = [], []
        for run in (lambda: q.process(x, fi, fo), lambda: q.process(x7, fi, fo), lambda: q.flush(fo)):
            want.append(run())
            levels.append(q.levels.copy())
        for a in (x, x7, *want, *levels):
            a.setflags(write=False)
        _cases[key] = (x, x7, want, levels, int(q.clipped[0]))
    return _cases[key]


def refused(G, fn, *args):
    """The name of the AirwaveError that fn(*args) raises, or None.  The exception is caught here and not in the test: an ExceptionInfo among
    a test's locals ties its frame, and every handle in it, into a reference cycle that is finalised whenever, in any order."""
    try:
        fn(*args)
    except G.aw.AirwaveError as err:
        return err.name
    return None


def same_levels(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("pair,C,form", CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_device_equals_the_composition_byte_for_byte(G, pair, C, form):
    check_three_calls(G, pair, C, form)


def check_three_calls(G, pair, C, form, gains="form"):
    """process (input 1 byte, output 3 bytes off a word), process and flush of case(pair, C, form, gains=gains) against the composition:
    every byte, every record field after every call, and the clipped word."""
    fi, fo, dither, g = FORMS[form]
    x, x7, want, levels, clipped = case(pair, C, form, gains=gains)
    gains = g if isinstance(gains, str) else gains
    rc = converter(G, pair, STREAMS, C, dither, gains)
    assert (rc.info()["dither"], rc.info()["gain_mode"], rc.info()["metering"]) == (dither, 1 if gains else 0, 1)
    word = G.torch.zeros(1, dtype=G.torch.int64, device="cuda")
    got = [process(G, rc, x, fi, fo, shift=1, out_shift=3, clipped_ptr=word.data_ptr())]
    assert same_levels(rc.levels(), levels[0])
    got.append(process(G, rc, x7, fi, fo, shift=2, out_shift=1, clipped_ptr=word.data_ptr()))
    assert same_levels(rc.levels(), levels[1])
    got.append(flush(G, rc, fo, clipped_ptr=word.data_ptr()))
    tile = rc.info()["tile"]
    assert 2 * tile <= got[0].shape[1] < 3 * tile                                   # three workgroups per stream, the last ragged
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (pair, C, form, i, int((g != w).sum()))
    assert rc.info()["frames_consumed"] == 0 and rc.info()["frames_produced"] == 0  # the flush reset them ...
    assert same_levels(rc.levels(), levels[2])                                      # ... and left the records
    assert int(word.item()) == clipped == int(levels[2]["clipped"].sum())
    assert int(levels[2]["frames"][0]) == sum(w.shape[1] for w in want)


def test_invariances_change_no_byte_and_no_record_field(G):
    pair, C, form = (44100, 48000), 7, "s24-s24 tpdf_hp"
    fi, fo, dither, _ = FORMS[form]
    x, x7, want, levels, clipped = case(pair, C, form, gains=GAINS)
    L, M, T, D = emu.plan(*pair)
    tile = emu.tile(pair[0], pair[1], C)
    n = x.shape[1]
    whole = np.concatenate(want, axis=1)
    # buffers shifted by 1 .. 3 bytes
    for shift in (1, 2, 3):
        rc = converter(G, pair, STREAMS, C, dither, GAINS)
        y = np.concatenate([process(G, rc, x, fi, fo, shift, (shift + 1) % 4 or 2), process(G, rc, x7, fi, fo, (shift + 2) % 4, shift), flush(G, rc, fo)], axis=1)
        assert np.array_equal(y, whole) and same_levels(rc.levels(), levels[2]), shift
    # calls cut in time: 1 frame, D frames (the first output), as many as make one tile of outputs more, the rest
    cuts = [0, 1, 1 + D, emu.input_frames_for(1 + tile, L, M, D), n]
    rc = converter(G, pair, STREAMS, C, dither, GAINS)
    parts = [process(G, rc, np.ascontiguousarray(x[:, a:b]), fi, fo) for a, b in zip(cuts[:-1], cuts[1:])]
    available = lambda N: max(0, -((N - D) * L // -M))          # noqa: E731  outputs that exist after N input frames
    assert [p.shape[1] for p in parts] == [available(b) - available(a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert parts[0].shape[1] == 0 and 1 <= parts[1].shape[1] <= 2 and tile - 1 <= parts[2].shape[1] <= tile and parts[3].shape[1] > tile
    assert np.array_equal(np.concatenate(parts, axis=1), want[0]) and same_levels(rc.levels(), levels[0])
    # streams sharded over two handles
    ys, recs = [], []
    for a, b in ((0, 1), (1, 3)):
        rc = converter(G, pair, b - a, C, dither, GAINS[a:b], first=FIRST + a)
        ys.append(np.concatenate([process(G, rc, np.ascontiguousarray(x[a:b]), fi, fo), process(G, rc, np.ascontiguousarray(x7[a:b]), fi, fo), flush(G, rc, fo)], axis=1))
        recs.append(rc.levels())
    assert np.array_equal(np.concatenate(ys, axis=0), whole) and same_levels(np.concatenate(recs), levels[2])


def test_records_and_clipped_device(G, delay):
    pair, C, form = (44100, 48000), 2, "f32-s16 gain"
    fi, fo, _, _ = FORMS[form]
    gains = [2.0, 2.5, 3.0]                                                         # full scale at 2, 1.6 and 1.33 sigma of the input
    x, x7, want, levels, clipped = case(pair, C, form, gains=gains)
    share = levels[0]["clipped"] / (want[0].shape[1] * C)
    print("clipped share of the composition per stream:", share)
    assert np.all(share > 0.01) and np.all(share < 0.5)
    torch = G.torch
    # metering off: clipped_device still counts, the records do not exist yet
    rc = converter(G, pair, STREAMS, C, NONE, gains, metering=False)
    word = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    assert np.array_equal(process(G, rc, x, fi, fo, clipped_ptr=word.data_ptr()), want[0])
    assert int(word.item()) == 5 + int(levels[0]["clipped"].sum())
    assert refused(G, rc.levels) == "INVALID_ARGUMENT"
    rc.reset()
    # metering on, behind a busy stream: get_levels returns the finished call's records
    rc.set_metering(True)
    assert not rc.levels()["frames"].any()
    keep, p_in = device(G, x)
    n_out = rc.output_frames(x.shape[1])
    t, p_out = output(G, want[0].size)
    delay.enqueue()
    assert rc.process_pcm_device(p_in, fi, x.shape[1], p_out, fo, n_out) == n_out
    assert same_levels(rc.levels(), levels[0])
    assert np.array_equal(fetch(G, t, want[0].size)[0], want[0].reshape(-1))
    assert np.array_equal(process(G, rc, x7, fi, fo), want[1]) and np.array_equal(flush(G, rc, fo), want[2])
    assert same_levels(rc.levels(), levels[2])                                      # they persist across the flush
    assert same_levels(rc.levels(1, 2), levels[2][1:3])
    for bad in ((-1, 1), (2, 2), (0, STREAMS + 1)):
        assert refused(G, rc.levels, *bad) == "INVALID_ARGUMENT"
    rc.reset_levels()
    assert not rc.levels().view(np.uint8).any()
    # metering off again: the records stay as they are
    rc.set_metering(False)
    process(G, rc, x, fi, fo)
    assert not rc.levels().view(np.uint8).any()
    rc.close()
    del keep


def test_contract_of_the_entries(G):
    torch, aw = G.torch, G.aw
    pair, C, S = (44100, 48000), 2, STREAMS
    x, x7, want, _, _ = case(pair, C, "s32-f32")
    # F32 / F32 through the new entry is aw_rateconv_process, bit for bit
    xf = pcm.from_bytes(pcm.random_input(np.random.default_rng(2), (S, x.shape[1], C), F32), F32)
    old, new = aw.RateConverter(pair[0], pair[1], S, C, ctx=G.ctx), aw.RateConverter(pair[0], pair[1], S, C, ctx=G.ctx)
    y_old = np.concatenate([old.process(xf), old.flush()], axis=1)
    y_new = np.concatenate([pcm.from_bytes(process(G, new, pcm.to_bytes(xf, F32), F32, F32, shift=3, out_shift=1), F32), pcm.from_bytes(flush(G, new, F32), F32)], axis=1)
    assert np.array_equal(y_old.view(np.uint32), y_new.view(np.uint32))
    # allocations: four in create, at most one per setter, none on a process path
    meter = aw.Spatializer(aw.HRIR(np.ones((2, 8), np.float32), 48000.0, ctx=G.ctx), [0, 1], [1, 0], 1, ctx=G.ctx)
    allocs = lambda: meter.info()["device_allocs"]          # noqa: E731
    a0 = allocs()
    rc = aw.RateConverter(pair[0], pair[1], S, C, ctx=G.ctx)
    assert allocs() == a0 + 4
    rc.set_dither("tpdf", SEED, FIRST)
    assert allocs() == a0 + 4
    rc.set_metering(True)
    assert allocs() == a0 + 5
    rc.set_metering(False)
    rc.set_metering(True)
    assert allocs() == a0 + 5
    rc.set_gain("fixed", GAINS)
    assert allocs() == a0 + 6
    rc.set_gain("none")
    assert allocs() == a0 + 6 and rc.info()["gain_mode"] == 0
    rc.set_gain("fixed", [0.5])
    a1 = allocs()
    assert a1 == a0 + 7 and rc.info()["gain_mode"] == 1
    # refusals of the setters leave the previous setting
    lib = aw._capi.load()
    g = np.array([1.0, np.inf, 1.0], np.float32)
    for mode, arr, n in ((2, GAINS, 3), (3, GAINS, 3), (1, g, 3), (1, [np.nan], 1), (1, GAINS, 2), (7, GAINS, 3)):
        a = np.asarray(arr, np.float32)
        assert lib.aw_pcm_rateconv_set_gain(rc._h, mode, a.ctypes.data_as(aw._capi.c_float_p), n) == 1, (mode, n)
    assert lib.aw_pcm_rateconv_set_gain(rc._h, 1, None, 1) == 1 and lib.aw_pcm_rateconv_set_dither(rc._h, 3, 0, 0) == 1
    assert rc.info()["gain_mode"] == 1 and rc.info()["dither"] == 1 and allocs() == a1
    # a short capacity or an unknown format leaves the handle and the output untouched
    fi, fo = S32, S16
    keep, p_in = device(G, x)
    n = x.shape[1]
    n_out = rc.output_frames(n)
    t, p_out = output(G, S * n_out * C * 2)
    n64 = ctypes.c_int64(-7)
    call = lambda *a: lib.aw_pcm_rateconv_process(rc._h, *a, ctypes.byref(n64), None)          # noqa: E731
    assert call(ctypes.c_void_p(p_in), fi, n, ctypes.c_void_p(p_out), fo, n_out - 1) == 1 and "capacity" in lib.aw_last_error_message().decode()
    assert call(ctypes.c_void_p(p_in), 4, n, ctypes.c_void_p(p_out), fo, n_out) == 1
    assert call(ctypes.c_void_p(p_in), fi, n, ctypes.c_void_p(p_out), -1, n_out) == 1
    assert call(None, fi, n, ctypes.c_void_p(p_out), fo, n_out) == 1
    assert call(ctypes.c_void_p(p_in), fi, -1, ctypes.c_void_p(p_out), fo, n_out) == 1
    assert lib.aw_pcm_rateconv_flush(rc._h, ctypes.c_void_p(p_out), 9, 1000, ctypes.byref(n64), None) == 1
    assert n64.value == -7 and rc.info()["frames_consumed"] == 0 and rc.output_frames(n) == n_out
    got, rest = fetch(G, t, S * n_out * C * 2)
    assert np.all(got == SENTINEL) and np.all(rest == SENTINEL)
    assert not rc.levels().view(np.uint8).any()
    # ... and the next call is the first call: the composition's bytes
    q = pcm.Converter(pair[0], pair[1], S, C, False, TPDF, SEED, FIRST, [0.5] * S)
    assert np.array_equal(process(G, rc, x, fi, fo), q.process(x, fi, fo)) and same_levels(rc.levels(), q.levels)
    # no device allocation on the process paths: the library's own count, then (every kernel loaded) the device's free memory
    y_cap = S * (n_out + 100) * C * 4
    t, p_out = output(G, y_cap)
    word = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc.reset()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for fo2 in (S16, S24, F32):
        rc.process_pcm_device(p_in, fi, n, p_out, fo2, n_out, word.data_ptr())
        rc.flush_pcm_device(p_out, fo2, 100, word.data_ptr())
        rc.reset_levels()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0
    assert allocs() == a1
    for h in (rc, old, new):
        h.close()
    del keep


def test_host_convenience_and_one_shot_convert(G):
    pair, C, form = (44100, 48000), 2, "s16-s16 tpdf"
    fi, fo, dither, _ = FORMS[form]
    x, x7, want, levels, clipped = case(pair, C, form)
    rc = converter(G, pair, STREAMS, C, dither)
    y, c0 = rc.process_pcm(pcm.from_bytes(x, S16), "s16")
    y7, c1 = rc.process_pcm(pcm.from_bytes(x7, S16), "s16")
    tail, c2 = rc.flush_pcm("s16")
    assert y.dtype == np.int16 and np.array_equal(np.concatenate([y, y7, tail], axis=1), pcm.from_bytes(np.concatenate(want, axis=1), S16))
    assert c0 + c1 + c2 == clipped
    # packed s24 in and out: uint8 [..., 3]
    x24, _, want24, _, _ = case(pair, C, "s24-s24 tpdf_hp")
    rc = converter(G, pair, STREAMS, C, TPDF_HP)
    y24, _ = rc.process_pcm(np.ascontiguousarray(x24), "s24", in_format="s24")
    assert y24.dtype == np.uint8 and y24.shape[-1] == 3 and np.array_equal(y24, want24[0])
    # convert(): process + flush with the dither of stream 0 on, first stream 0
    q = pcm.Converter(pair[0], pair[1], STREAMS, C, False, TPDF, 77, 0)
    both = np.concatenate([x, x7], axis=1)
    ref = np.concatenate([q.process(both, S16, S16), q.flush(S16)], axis=1)
    got = G.aw.convert(pcm.from_bytes(both, S16), pair[0], pair[1], ctx=G.ctx, out_format="s16", dither="tpdf", seed=77)
    assert got.dtype == np.int16 and np.array_equal(got, pcm.from_bytes(ref, S16))


def test_stream_order_on_a_busy_caller_owned_stream(G, delay):
    """Producer, aw_pcm_rateconv_process twice, _flush and a consumer on a caller's side stream behind a delay, no host synchronisation in
    between: the bytes are the synchronised run's, and the calls returned while the delay was still pending."""
    from test_gpu_stream_order import Sandwich, poison_left, same_bits, side_stream
    torch, aw = G.torch, G.aw
    E = Env()
    E.torch, E.aw, E.delay = torch, aw, delay
    E.probe = torch.zeros(64, device="cuda")
    pair, C, form = (44100, 48000), 2, "s16-s16 tpdf"
    fi, fo, dither, _ = FORMS[form]
    x, x7, want, levels, clipped = case(pair, C, form)
    as16 = lambda b: pcm.from_bytes(b, S16)          # noqa: E731
    n = x.shape[1]
    s = side_stream(E, [torch.cuda.default_stream()])
    ctx = aw.Context(0, stream=s.cuda_stream)
    rc = converter(G, pair, STREAMS, C, dither, ctx=ctx)
    ctx.synchronize()
    counts = {}
    sw = Sandwich(E, s, "aw_pcm_rateconv_process, _process, _flush")
    X = [sw.input(as16(x)), sw.input(as16(x7))]
    Y = [sw.output(as16(w)) for w in want]
    word = torch.zeros(1, dtype=torch.int64, device="cuda")

    def call(i, frames):
        return lambda: counts.__setitem__(i, rc.process_pcm_device(X[i].data_ptr(), fi, frames, Y[i].data_ptr(), fo, want[i].shape[1], word.data_ptr()))
    got = sw.run([("aw_pcm_rateconv_process, two tiles + 3", call(0, n), True), ("aw_pcm_rateconv_process, 7 frames", call(1, 7), True),
                  ("aw_pcm_rateconv_flush", lambda: counts.__setitem__(2, rc.flush_pcm_device(Y[2].data_ptr(), fo, want[2].shape[1], word.data_ptr())), True)])
    print(f"{sw.what}: the delay held the stream {sw.delay_ms:.1f} ms; still pending when the last call returned: {sw.pending}")
    assert [counts[i] for i in range(3)] == [w.shape[1] for w in want]
    for g, w in zip(got, want):
        assert poison_left(g, as16(w)) == 0 and same_bits(g, as16(w))
    assert sw.pending, "the calls returned only after the delay had run: they did not just enqueue"
    assert same_levels(rc.levels(), levels[2]) and int(word.item()) == clipped
    rc.close()
    ctx.close()


def test_the_example_runs_and_prints_the_compositions_counts(G, golden_dir):
    from test_example_resample_pcm import EXE, build
    build()
    aw = G.aw
    S, seconds, gain = 2, 0.05, 1.0                                                 # (unity gain: the 96 kHz bucket's peaks lie above full scale)
    wav = os.path.join(golden_dir, "hrtf", "RoomSH1.0.wav")
    r = subprocess.run([EXE, wav, str(S), str(seconds), str(gain)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "bucket 44100 Hz -> 48000 Hz: L 160 M 147 taps 96 latency 48; 2 streams, 2205 frames in, 2348 + 52 = 2400 frames out" in r.stdout
    assert "bucket 96000 Hz -> 48000 Hz: L 1 M 2 taps 192 latency 96; 2 streams, 4800 frames in, 2352 + 48 = 2400 frames out" in r.stdout
    rows = re.findall(r"stream (\d+) at (\d+) Hz: (\d+) frames at 48000 Hz, peak (\S+) before the gain of (\S+), clipped (\d+), at the rails (\d+), nonfinite (\d+)", r.stdout)
    assert len(rows) == 2 * S
    # the same run from Python: the example's generator, the preset at the bucket's rate (s16 in, float32 out), then the composition
    layout = aw.InputLayout.detect(8)
    expected = []
    for b, rate in enumerate((44100, 96000)):
        frames = int(seconds * rate)
        state, vals = 12345 + b, np.empty(S * frames * 8, np.int16)
        for i in range(vals.size):
            state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
            vals[i] = (state >> 18) - 8192
        sp = aw.HRIRManager(ctx=G.ctx).activatePreset(wav, float(rate), layout, n_streams=S)
        mid = np.zeros((S, frames, 2), np.float32)
        sp.process_host_into(vals.reshape(S, frames, 8), mid, out_format="f32")
        q = pcm.Converter(rate, 48000, S, 2, False, TPDF, 2024, b * S, [gain] * S)
        y = np.concatenate([q.process(pcm.to_bytes(mid, F32), F32, S16), q.flush(S16)], axis=1)
        v = pcm.from_bytes(y, S16)
        for i in range(S):
            expected.append((i, rate, int(q.levels["frames"][i]), np.float32(q.levels["peak"][i]), int(q.levels["clipped"][i]),
                             int(((v[i] == 32767) | (v[i] == -32768)).sum()), 0))
    got = [(int(a), int(b), int(c), np.float32(float(p)), int(k), int(rails), int(nf)) for a, b, c, p, _, k, rails, nf in rows]
    print("example:", got)
    assert got == expected
    assert all(e[2] == 2400 and 0.001 < e[3] < 100.0 for e in expected) and sum(e[4] for e in expected) > 0          # something clipped, and was counted
