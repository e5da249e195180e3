"""Stream order of the device-buffer entries (include/airwave_hip.h, "stream order"): they only enqueue on the context's stream, which
may be a caller's busy stream.  The instrument is a busy-stream sandwich: on stream s, with no host synchronisation in between, a delay
(repeated torch.mm, calibrated once), the producer of the input, the library calls, the consumer of the output.  Input and output start
as poison (quiet NaN; 0xA5 bytes for integer PCM).  A launch, memset or copy that left the stream reads poison or writes after the consumer
ran, and the delay makes that certain rather than a race.  Every case compares the consumer's copy, bit for bit, with the same calls on a
fresh handle in a context that owns its stream with the host synchronised around every call, and with the float64 truth; for the entries
that only enqueue it also checks that the call returned while the delay was still pending.

The delay: DELAY_MS, at least ten times the longest host-side enqueue time of any call below (the module prints both figures when it ends)."""
import math
import time

import numpy as np
import pytest

import spectral_ref as sr
from test_gpu_eq import FILTERS, ULP, adef, odef
from test_gpu_parity import TOL
from test_gpu_pcm_dither import S16, S24, TPDF, encode, encode_dithered

pytestmark = pytest.mark.gpu

DELAY_MS = 50.0
POISON = 0xA5
KNOBS = ("AW_WINDOW", "AW_LW", "AW_OLA", "AW_OLA_MIN_BLOCKS", "AW_PART_CMAC", "AW_PART_HERM", "AW_PART_FWD", "AW_HOP_ALIGN", "AW_HOST_CHUNK_MB",
         "AW_SPEC_SCRATCH_MB")
KINDS = ("side", "legacy", "owned")

_contexts, _truth, _times = {}, {}, []


class Delay:
    """Ordinary torch work that holds a stream for about `ms`: torch.mm on fixed operands, timed once with a pair of events."""

    def __init__(self, torch, ms):
        self.torch = torch
        n = 4096
        self.a, self.b = torch.randn(n, n, device="cuda"), torch.randn(n, n, device="cuda")
        self.c = torch.empty(n, n, device="cuda")
        for _ in range(24):                                    # (the library's first use, and the clocks)
            torch.mm(self.a, self.b, out=self.c)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(16):
            torch.mm(self.a, self.b, out=self.c)
        e1.record()
        e1.synchronize()
        self.per_ms = e0.elapsed_time(e1) / 16
        self.n = max(1, math.ceil(ms / self.per_ms))

    def enqueue(self):
        for _ in range(self.n):
            self.torch.mm(self.a, self.b, out=self.c)


class Env:
    pass


@pytest.fixture(scope="module")
def E(oracle):
    import torch
    import airwave_amd as aw
    e = Env()
    e.torch, e.aw, e.oracle = torch, aw, oracle
    e.delay = Delay(torch, DELAY_MS)
    e.probe = torch.zeros(64, device="cuda")
    yield e
    if _times:                              # the figures DELAY_MS is chosen from (the condition itself is `pending`, per case)
        longest, label = max(_times)
        print(f"FIGURE stream-order: delay {DELAY_MS:.0f} ms asked = {e.delay.n} torch.mm of {e.delay.per_ms:.3f} ms; longest enqueue of {len(_times)} calls "
              f"{longest * 1e3:.3f} ms ({label}); ratio {DELAY_MS / (longest * 1e3):.1f}")
        for t, what in sorted(_times, reverse=True)[:8]:
            print(f"FIGURE stream-order: {t * 1e3:8.3f} ms  {what}")


def runs_beside(E, s, other):
    """Work on `other` completes while the delay holds `s`: the two do not share a hardware queue (which would run them in the order
    they were submitted, whatever their streams)."""
    torch = E.torch
    torch.cuda.synchronize()
    held, done = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(s):
        E.delay.enqueue()
        held.record()
    with torch.cuda.stream(other):
        E.probe.add_(1.0)
        done.record()
    done.synchronize()
    free = not held.query()
    s.synchronize()
    return free


def side_stream(E, beside):
    """A torch side stream that runs beside every stream of `beside`.  The runtime spreads its streams over a few hardware queues; a side
    stream that shared the legacy default stream's queue would hide a launch that strayed there behind the producer."""
    for i in range(16):
        s = E.torch.cuda.Stream()
        if s.cuda_stream != 0 and all(runs_beside(E, s, o) for o in beside):
            return s
        print(f"side stream candidate {i} shares a hardware queue with a stream it must run beside: the next one")
    raise AssertionError("no torch side stream runs beside the legacy default stream on this device")


def context(E, monkeypatch, env, kind):
    """(context, torch stream) of one of the three kinds of caller stream, or kind "ref": a context that owns its stream, driven with the host
    synchronised around every call.  Knobs are read when contexts and spatializers are created, so they stay set for the test."""
    torch, aw = E.torch, E.aw
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    key = (tuple(sorted(env.items())), kind)
    if key not in _contexts:
        if kind.startswith("side"):                            # a non-blocking side stream, the stream of every real torch pipeline
            first = _contexts.get((key[0], "side"))
            s = side_stream(E, [torch.cuda.default_stream()] + ([first[1]] if first and kind != "side" else []))
            ctx = aw.Context(0, stream=s.cuda_stream)
            assert ctx.stream == s.cuda_stream
        elif kind == "legacy":                                 # the legacy default stream, handle 0
            s = torch.cuda.default_stream()
            assert s.cuda_stream == 0
            ctx = aw.Context(0, stream=0)
            assert ctx.stream == 0
        else:                                                  # the library's own stream, handed to torch through aw_context_stream
            ctx = aw.Context(0)
            assert ctx.stream != 0
            s = torch.cuda.ExternalStream(ctx.stream) if kind == "owned" else None
        _contexts[key] = (ctx, s)
    return _contexts[key]


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()          # (a copy: the shared cases are read-only)


def poisoned(torch, like):
    """Device bytes of like's size: quiet NaN for float32, POISON bytes for integer PCM."""
    t = torch.empty(like.nbytes, dtype=torch.uint8, device="cuda")
    if like.dtype == np.float32:
        t.view(torch.float32).fill_(float("nan"))
    else:
        t.fill_(POISON)
    return t


def to_host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def poison_left(got, ref):
    """Samples of the output that still are poison: NaN, or the poison bytes where the reference run has other bytes."""
    if got.dtype == np.float32:
        return int(np.isnan(got).sum())
    width = 3 if got.dtype == np.uint8 else got.dtype.itemsize          # (packed s24: uint8 [..., 3])
    g, r = got.reshape(-1).view(np.uint8).reshape(-1, width), ref.reshape(-1).view(np.uint8).reshape(-1, width)
    return int(((g == POISON).all(axis=1) & ~(r == POISON).all(axis=1)).sum())


class Sandwich:
    """Buffers first (on the default stream, alive until after the final synchronisation), poison, ONE device synchronisation, then on the
    stream: delay, producers, the calls, consumers; the event behind the delay is read straight after the last call returns."""

    def __init__(self, E, stream, what):
        self.E, self.s, self.what = E, stream, what
        self.ins, self.outs = [], []
        torch = E.torch
        self.e_start, self.e_delay = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.pending = None

    def input(self, host):
        true = to_dev(self.E.torch, host)
        x = poisoned(self.E.torch, host)
        self.ins.append((x, true))
        return x

    def output(self, like, existing=None):
        """existing: the buffer the calls write is an input (in place) or starts with a value of its own (a counter)."""
        y = poisoned(self.E.torch, like) if existing is None else existing
        self.outs.append((y, poisoned(self.E.torch, like), like))
        return y

    def hold(self):
        self.e_start.record()
        self.E.delay.enqueue()
        self.e_delay.record()

    def produce(self):
        for x, true in self.ins:
            x.copy_(true)

    def call(self, calls):
        """calls: (label, function, only_enqueues).  The host time of every call that only enqueues goes into the module's figures."""
        for label, fn, only_enqueues in calls:
            t0 = time.perf_counter()
            fn()
            if only_enqueues:
                _times.append((time.perf_counter() - t0, f"{self.what}: {label}"))
        self.pending = not self.e_delay.query()

    def consume(self):
        for y, z, _ in self.outs:
            z.copy_(y)

    def results(self):
        self.delay_ms = self.e_start.elapsed_time(self.e_delay)
        return [to_host(z, like) for _, z, like in self.outs]

    def run(self, calls, before_sync=None):
        torch = self.E.torch
        torch.cuda.synchronize()
        with torch.cuda.stream(self.s):
            self.hold()
            self.produce()
            self.call(calls)
            self.consume()
            self.extra = before_sync() if before_sync else None
        self.s.synchronize()
        return self.results()


def reference_run(E, ctx, inputs, out_likes, script, handles, inplace, existing=None):
    """The same calls with the host synchronised around each: -> the outputs."""
    torch = E.torch
    X = [to_dev(torch, a) for a in inputs]
    given = [X[inplace[i]] if i in inplace else (existing(i) if existing else None) for i in range(len(out_likes))]
    Y = [poisoned(torch, like) if y is None else y for y, like in zip(given, out_likes)]
    torch.cuda.synchronize()
    for _, fn, _ in script(handles, X, Y):
        fn()
        ctx.synchronize()
        torch.cuda.synchronize()
    return [to_host(y, like) for y, like in zip(Y, out_likes)]


def run_both(E, monkeypatch, kind, env, make, inputs, out_likes, script, what, inplace=None, asynchronous=True, before_sync=None, existing=None):
    """The reference run, then the sandwich on a stream of `kind`: bit equality, nothing left over, and — for calls that only enqueue — the
    call returned while the delay was pending.  -> (outputs, reference outputs, handles, reference handles, sandwich)."""
    inplace = inplace or {}
    ctx_r, _ = context(E, monkeypatch, env, "ref")
    h_r = make(ctx_r)
    ref = reference_run(E, ctx_r, inputs, out_likes, script, h_r, inplace, existing)
    ctx, s = context(E, monkeypatch, env, kind)
    h = make(ctx)
    sw = Sandwich(E, s, f"{what} [{kind}]")
    X = [sw.input(a) for a in inputs]
    Y = [sw.output(like, X[inplace[i]] if i in inplace else (existing(i) if existing else None)) for i, like in enumerate(out_likes)]
    got = sw.run(script(h, X, Y), (lambda: before_sync(h)) if before_sync else None)
    print(f"{sw.what}: the delay held the stream {sw.delay_ms:.1f} ms; still pending when the last call returned: {sw.pending}")
    for i, (g, r) in enumerate(zip(got, ref)):
        assert poison_left(g, r) == 0, (what, kind, i, poison_left(g, r))
        assert same_bits(g, r), (what, kind, i, int((g != r).sum()))
    if asynchronous:
        assert sw.pending, f"{what} [{kind}]: the calls returned only after the delay had run: they did not just enqueue"
    return got, ref, h, h_r, sw


def worst(oracle, y, ref):
    assert np.isfinite(y).all()
    return max(oracle.peak_rel_error(y[s, :, ear], ref[s][:, ear]) for s in range(y.shape[0]) for ear in range(2))


def f32_like(*shape):
    return np.empty(shape, np.float32)


# ---- every kernel family of aw_spatializer_process ---------------------------------------------------------------------------------------

# family -> (knobs, channels, taps, streams, frames of the calls of one sandwich, what info() shows after them; None: more than 0)
FAMILIES = {
    "ols8192": ({"AW_WINDOW": "8192", "AW_OLA": "0", "AW_LW": "0"}, 2, 600, 2, (17001, 2999), {"path": 0, "fft": 8192, "overlap_add_rows": 0, "long_window_rows": 0}),
    "ola": ({"AW_OLA": "1", "AW_OLA_MIN_BLOCKS": "0"}, 8, 3969, 2, (5001, 2999), {"path": 0, "fft": 8192, "overlap_add_rows": None, "long_window_rows": 0}),
    "ols16384": ({"AW_WINDOW": "16384", "AW_LW": "0"}, 7, 4320, 2, (25001, 2999), {"path": 0, "fft": 16384, "long_window_rows": 0}),
    "part-march": ({"AW_WINDOW": "4096", "AW_LW": "0"}, 7, 9000, 3, (5001, 2999), {"path": 1, "partitions": 3, "long_window_rows": 0}),
    "part-group": ({"AW_WINDOW": "4096", "AW_LW": "0", "AW_PART_CMAC": "group"}, 7, 9000, 3, (5001, 2999), {"path": 1, "partitions": 3, "long_window_rows": 0}),
    "lw32": ({"AW_LW": "32"}, 7, 20000, 2, (150000,), {"path": 1, "long_window_rows": 32}),
}


def family_case(oracle, family, calls=None):
    """(hrir, maps, input of every call [S][F][C], float64 truth per stream over the calls' frames in a row), computed once and left unchanged."""
    _, channels, taps, S, default_calls, _ = FAMILIES[family]
    calls = calls or default_calls
    key = (family, calls)
    if key not in _truth:
        h = oracle.synth_hrir(14, taps, seed=taps)
        lt, rt = sr.maps(channels)
        x = oracle.synth_input(S, sum(calls), channels, seed=channels)
        ref = [oracle.spatialize_f64(x[s], h, lt, rt) for s in range(S)]
        for a in (h, lt, rt, x, *ref):
            a.setflags(write=False)
        _truth[key] = (h, lt, rt, x, ref)
    return _truth[key]


def split(x, calls):
    at = np.cumsum((0,) + tuple(calls))
    return [np.ascontiguousarray(x[:, a:b]) for a, b in zip(at[:-1], at[1:])]


def spatializer(E, ctx, h, lt, rt, S, reserve):
    sp = E.aw.Spatializer(E.aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    if reserve:
        sp.reserve(reserve)
    return sp


def process_script(calls, only_enqueues=True):
    def script(sp, X, Y):
        return [(f"aw_spatializer_process, {n} frames", (lambda i=i, n=n: sp.process_device(X[i].data_ptr(), Y[i].data_ptr(), n)), only_enqueues)
                for i, n in enumerate(calls)]
    return script


def check_family(E, monkeypatch, family, kind, reserved=True):
    env, channels, taps, S, calls, info = FAMILIES[family]
    h, lt, rt, x, truth = family_case(E.oracle, family)
    got, _, sp, _, _ = run_both(E, monkeypatch, kind, env, lambda ctx: spatializer(E, ctx, h, lt, rt, S, max(calls) if reserved else 0), split(x, calls),
                                [f32_like(S, n, 2) for n in calls], process_script(calls, reserved), f"{family}{'' if reserved else ', not reserved'}", asynchronous=reserved)
    assert all(sp.info()[k] == v if v is not None else sp.info()[k] > 0 for k, v in info.items()), (family, sp.info())
    err = worst(E.oracle, np.concatenate(got, axis=1), truth)
    print(f"{family} [{kind}]: peak_rel_error against the float64 truth {err:.2e}")
    assert err < TOL, (family, kind, err)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_two_ragged_calls_of_every_kernel_family(E, monkeypatch, family, kind):
    """Two ragged calls in one sandwich (the long-window family: one long call): the history ping-pong flips with no host in between.
    Handles are reserved, so the calls only enqueue."""
    check_family(E, monkeypatch, family, kind)


def test_unreserved_long_window_call_builds_its_tables_and_is_still_in_order(E, monkeypatch):
    """The first long-window call of a handle that was not reserved builds its tables and synchronises the stream (lw_get_plan): results only."""
    check_family(E, monkeypatch, "lw32", "side", reserved=False)


@pytest.mark.parametrize("family", ["ols8192", "part-march"])
def test_reset_between_two_calls(E, monkeypatch, family):
    """aw_spatializer_reset is a memset on the stream: behind it the same input gives the first call's output again."""
    env, channels, taps, S, _, _ = FAMILIES[family]
    calls = (5001,)
    h, lt, rt, x, truth = family_case(E.oracle, family, calls)

    def script(sp, X, Y):
        run = lambda i: (lambda: sp.process_device(X[0].data_ptr(), Y[i].data_ptr(), calls[0]))
        return [("aw_spatializer_process", run(0), True), ("aw_spatializer_reset", sp.reset, True), ("aw_spatializer_process", run(1), True)]
    got, _, _, _, _ = run_both(E, monkeypatch, "side", env, lambda ctx: spatializer(E, ctx, h, lt, rt, S, calls[0]), [x], [f32_like(S, calls[0], 2)] * 2, script,
                               f"reset between two calls, {family}")
    assert same_bits(got[0], got[1])
    assert worst(E.oracle, got[1], truth) < TOL


def test_second_spatializer_of_the_context_between_two_calls(E, monkeypatch):
    """Two handles of one context share its scratch pool: the second one's call sits between the two calls of the first, partitioned path."""
    env, channels, taps, S, calls, _ = FAMILIES["part-march"]
    h, lt, rt, x, truth = family_case(E.oracle, "part-march")
    S2, C2, F2 = 2, 4, 4099
    key = "second spatializer"
    if key not in _truth:
        h2 = E.oracle.synth_hrir(14, 5000, seed=5000)
        lt2, rt2 = sr.maps(C2)
        x2 = E.oracle.synth_input(S2, F2, C2, seed=44)
        _truth[key] = (h2, lt2, rt2, x2, [E.oracle.spatialize_f64(x2[s], h2, lt2, rt2) for s in range(S2)])
    h2, lt2, rt2, x2, truth2 = _truth[key]

    def make(ctx):
        return spatializer(E, ctx, h, lt, rt, S, max(calls)), spatializer(E, ctx, h2, lt2, rt2, S2, F2)

    def script(sps, X, Y):
        a, b = sps
        return [("aw_spatializer_process", lambda: a.process_device(X[0].data_ptr(), Y[0].data_ptr(), calls[0]), True),
                ("aw_spatializer_process, second handle", lambda: b.process_device(X[2].data_ptr(), Y[2].data_ptr(), F2), True),
                ("aw_spatializer_process", lambda: a.process_device(X[1].data_ptr(), Y[1].data_ptr(), calls[1]), True)]
    got, _, sps, _, _ = run_both(E, monkeypatch, "side", env, make, split(x, calls) + [x2], [f32_like(S, n, 2) for n in calls] + [f32_like(S2, F2, 2)], script,
                                 "a second spatializer on the context")
    assert sps[0].info()["path"] == 1 and sps[1].info()["path"] == 1
    assert worst(E.oracle, np.concatenate(got[:2], axis=1), truth) < TOL and worst(E.oracle, got[2], truth2) < TOL


# ---- aw_spatializer_process_pcm with every output stage on --------------------------------------------------------------------------------

def pack_s24(s):
    u = (s.astype(np.int64) & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)


def records(sp):
    return {"levels": sp.levels(), "loudness": sp.loudness(), "hops": np.stack([sp.loudness_hops(s, 0, 2) for s in range(sp.n_streams)]),
            "true_peak": sp.true_peak(), "limiter": sp.limiter()}


def check_records(got, want, frames, what):
    """Field for field.  The meter's energy is a sum whose order is unspecified (include/airwave_hip.h: at most N 2^-53 relative)."""
    for name in ("loudness", "hops", "true_peak", "limiter"):
        assert got[name].tobytes() == want[name].tobytes(), (what, name, got[name], want[name])
    for field in got["levels"].dtype.names:
        if field == "energy":
            assert np.allclose(got["levels"][field], want["levels"][field], rtol=2 * frames * 2.0 ** -53, atol=0.0), (what, field)
        else:
            assert np.array_equal(got["levels"][field], want["levels"][field]), (what, field, got["levels"][field], want["levels"][field])
    assert np.all(got["levels"]["frames"] == frames) and np.all(got["limiter"]["frames"] == frames) and np.all(got["true_peak"]["frames"] == frames)


@pytest.mark.parametrize("kind", ["side", "legacy"])
def test_pcm_entry_with_every_output_stage(E, monkeypatch, kind):
    """s16 in, s24 out; TPDF dither, meter, fixed gain, loudness, true peak and the limiter at attack 64 / hold 128, two calls in one
    sandwich.  One getter is read while the delay is pending: it synchronises the stream itself and must see the finished calls."""
    torch, oracle = E.torch, E.oracle
    S, C, taps, calls, ceiling, seed = 3, 8, 4320, (4097, 2999), 0.5, 77
    F = sum(calls)
    key = "pcm"
    if key not in _truth:
        h = oracle.synth_hrir(14, taps, seed=21)
        lt, rt = sr.maps(C)
        x16 = np.clip(np.rint(oracle.synth_input(S, F, C, seed=8) * 32768.0), -32768, 32767).astype(np.int16)
        truth = [oracle.spatialize_f64(x16[s].astype(np.float32) / np.float32(32768), h, lt, rt) for s in range(S)]
        gains = np.array([2.0 * ceiling / np.abs(t).max() for t in truth], np.float32)          # the limiter has work: peaks at twice the ceiling
        _truth[key] = (h, lt, rt, x16, gains)
    h, lt, rt, x16, gains = _truth[key]

    def make(ctx, out="s24"):
        sp = E.aw.Spatializer(E.aw.HRIR(h, sample_rate=48000.0, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
        sp.set_metering(True)
        sp.set_gain("fixed", gains)
        sp.set_loudness(True, 2.0)
        sp.set_true_peak(True)
        sp.set_dither("tpdf", seed)
        sp.set_limiter(True, ceiling, 64, 128)
        sp.reserve_pcm(max(calls), "s16", out)
        return sp

    def script_for(out):
        def script(sp, X, Y):
            clip = Y[len(calls)].data_ptr() if len(Y) > len(calls) else 0
            return [(f"aw_spatializer_process_pcm, {n} frames", (lambda i=i, n=n: sp.process_pcm_device(X[i].data_ptr(), "s16", Y[i].data_ptr(), out, n, clip)), True)
                    for i, n in enumerate(calls)]
        return script

    def counter(i):                         # the clipped count is added to: it starts as zero, not as poison (a fresh one per run)
        return torch.zeros(8, dtype=torch.uint8, device="cuda") if i == len(calls) else None
    pending_levels = {}

    def getter_while_pending(sp):
        pending_levels["levels"] = sp.levels()                   # synchronises the context's stream, then reads with a blocking copy
    likes = [np.empty((S, n, 2, 3), np.uint8) for n in calls] + [np.empty(1, np.uint64)]
    got, ref, sp, sp_r, sw = run_both(E, monkeypatch, kind, {}, make, split(x16, calls), likes, script_for("s24"), "process_pcm, every output stage", existing=counter,
                                      before_sync=getter_while_pending)
    assert sw.e_delay.query()
    want = records(sp_r)
    check_records(records(sp), want, F, "after the final synchronisation")
    check_records(dict(records(sp), levels=pending_levels["levels"]), want, F, "get_levels while the delay was pending")
    assert np.all(want["limiter"]["limited_frames"] > 0) and np.all(want["limiter"]["min_gain"] < 0.75)          # (the stages had work)
    # the integer output is numpy's dithered encode of the float32 output the same stages give a reference handle
    ctx_r, _ = context(E, monkeypatch, {}, "ref")
    z = reference_run(E, ctx_r, split(x16, calls), [f32_like(S, n, 2) for n in calls], script_for("f32"), make(ctx_r, "f32"), {})
    n_clip, pos = 0, 0
    for i, n in enumerate(calls):
        want_pcm, k = encode_dithered(S24, TPDF, z[i], seed, first_stream=0, pos0=pos)
        assert np.array_equal(got[i], want_pcm), (kind, i)
        n_clip, pos = n_clip + k, pos + n
    assert int(got[len(calls)][0]) == n_clip == int(ref[len(calls)][0])


# ---- host entries while the stream is busy ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("pcm", [False, True], ids=["process_host", "process_host_pcm"])
def test_host_entry_behind_a_device_call_on_a_busy_stream(E, monkeypatch, pcm, pinned):
    """The host entries are synchronous.  Called while the delay is pending, directly after a device-entry call of the same handle (whose
    staging they share), they return the complete output: the reference continuation of the first call's state.  The batch crosses in
    three chunks of streams, so the copy streams take part."""
    oracle = E.oracle
    S, C, taps, F1, F2 = 5, 8, 4320, 4097, 20011
    env = {"AW_HOST_CHUNK_MB": "1"}
    key = "host"
    if key not in _truth:
        h = oracle.synth_hrir(14, taps, seed=33)
        lt, rt = sr.maps(C)
        x16 = np.clip(np.rint(oracle.synth_input(S, F1 + F2, C, seed=12) * 32768.0), -32768, 32767).astype(np.int16)
        xf = x16.astype(np.float32) / np.float32(32768)
        _truth[key] = (h, lt, rt, x16, xf, [oracle.spatialize_f64(xf[s], h, lt, rt) for s in range(S)])
    h, lt, rt, x16, xf, truth = _truth[key]
    fin, fout = ("s24", "s16") if pcm else ("f32", "f32")
    x1 = pack_s24(x16[:, :F1].astype(np.int32) * 256) if pcm else np.ascontiguousarray(x16[:, :F1])          # (the same samples in either format)
    f1 = "s24" if pcm else "s16"
    x2_host = pack_s24(x16[:, F1:].astype(np.int32) * 256) if pcm else np.ascontiguousarray(xf[:, F1:])
    out_like = np.empty((S, F2, 2), np.int16 if pcm else np.float32)

    def make(ctx, fo=fout):
        sp = spatializer(E, ctx, h, lt, rt, S, 0)
        sp.reserve_pcm(F2, fin, fo)
        empty = ctx.pinned_empty if pinned else np.empty
        x2 = empty(x2_host.shape, x2_host.dtype)
        x2[...] = x2_host
        out = empty((S, F2, 2), np.float32 if fo == "f32" else np.int16)
        out.reshape(-1).view(np.uint8)[...] = POISON
        return {"sp": sp, "x2": x2, "out": out, "fo": fo}

    def script(hd, X, Y):
        sp = hd["sp"]

        def host_call():
            hd["clipped"] = sp.process_host_into(hd["x2"], hd["out"], in_format=fin, out_format=hd["fo"])
            hd["on_return"] = np.array(hd["out"])               # what the caller sees when the call returns
            hd["chunk"] = sp.info()["host_chunk_streams"]
        return [("aw_spatializer_process_pcm", lambda: sp.process_pcm_device(X[0].data_ptr(), f1, Y[0].data_ptr(), hd["fo"], F1), True),
                ("host entry", host_call, False)]
    y1_like = np.empty((S, F1, 2), out_like.dtype)
    got, ref, hd, hd_r, sw = run_both(E, monkeypatch, "side", env, make, [x1], [y1_like], script, f"host entry ({fin} -> {fout}, {'pinned' if pinned else 'pageable'})",
                                      asynchronous=False)
    assert sw.pending is False               # the host entry returned after the delay: it waited for the context's stream
    assert 0 < hd["chunk"] and -(-S // hd["chunk"]) >= 3, hd["chunk"]                       # at least three chunks of streams
    assert same_bits(hd["on_return"], hd_r["on_return"]) and poison_left(hd["on_return"], hd_r["on_return"]) == 0
    assert hd["clipped"] == hd_r["clipped"]
    if pcm:                                 # numpy's encode of the float32 output of a reference handle
        ctx_r, _ = context(E, monkeypatch, env, "ref")
        hf = make(ctx_r, "f32")
        y1f = reference_run(E, ctx_r, [x1], [f32_like(S, F1, 2)], script, hf, {})[0]
        y2f = hf["on_return"]
        for g, f in ((got[0], y1f), (hd["on_return"], y2f)):
            want, _ = encode(S16, f)
            assert np.array_equal(g, want)
        assert hd["clipped"] == encode(S16, y2f)[1]
    else:
        y1f, y2f = got[0], hd["on_return"]
    assert worst(oracle, np.concatenate([y1f, y2f], axis=1), truth) < TOL


# ---- parametric EQ ----------------------------------------------------------------------------------------------------------------------

EQ_CALLS, EQ_S, EQ_FS = (4097, 33), 3, 48000.0


def eq_inputs(oracle):
    x = oracle.synth_input(EQ_S, sum(EQ_CALLS), 2, seed=31)
    return x, split(x, EQ_CALLS)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_eq_state_process(E, monkeypatch, in_place):
    aw, oracle = E.aw, E.oracle
    x, xs = eq_inputs(oracle)

    def script(st, X, Y):
        return [(f"aw_eq_state_process, {n} frames", (lambda i=i, n=n: st.process_device(X[i].data_ptr(), Y[i].data_ptr(), n)), True) for i, n in enumerate(EQ_CALLS)]
    got, _, _, _, _ = run_both(E, monkeypatch, "side", {}, lambda ctx: aw.ParametricEqualizerState(adef(aw, -2.56, FILTERS), EQ_FS, n_streams=EQ_S, ctx=ctx), xs,
                               [f32_like(EQ_S, n, 2) for n in EQ_CALLS], script, f"aw_eq_state_process{', in place' if in_place else ''}",
                               inplace={0: 0, 1: 1} if in_place else None)
    y = np.concatenate(got, axis=1)
    for s in range(EQ_S):
        ref = oracle.eq_prepare(odef(oracle, -2.56, FILTERS), EQ_FS)
        want = [ref.process(c[s, :, 0], c[s, :, 1]) for c in xs]
        for ear in range(2):
            assert np.max(np.abs(y[s, :, ear] - np.concatenate([w[ear] for w in want]))) <= ULP, (s, ear)


def test_eq_process_across_a_crossfade(E, monkeypatch):
    """aw_eq_process with a target published before the sandwich: the first call crossfades (copy, cascade and blend kernels) and
    finishes the fade, the second runs the new state alone."""
    aw, oracle = E.aw, E.oracle
    x, xs = eq_inputs(oracle)

    def make(ctx):
        p = aw.ParametricEqualizerProcessor(EQ_FS, maxFramesPerCallback=0, n_streams=EQ_S, ctx=ctx)
        p.setTarget(adef(aw, -2.56, FILTERS))
        return p

    def script(p, X, Y):
        return [(f"aw_eq_process, {n} frames", (lambda i=i, n=n: p.process_device(X[i].data_ptr(), Y[i].data_ptr(), n)), True) for i, n in enumerate(EQ_CALLS)]
    got, _, p, _, _ = run_both(E, monkeypatch, "side", {}, make, xs, [f32_like(EQ_S, n, 2) for n in EQ_CALLS], script, "aw_eq_process across a crossfade")
    assert p.transitionLength == 960 and not p.isTransitioning
    y = np.concatenate(got, axis=1)
    for s in range(EQ_S):
        ref = oracle.ParametricEqualizerProcessor(EQ_FS)
        ref.max_frames = 1 << 30
        ref.set_target(odef(oracle, -2.56, FILTERS))
        want = [ref.process(c[s, :, 0], c[s, :, 1]) for c in xs]
        for ear in range(2):
            assert np.max(np.abs(y[s, :, ear] - np.concatenate([w[ear] for w in want]))) <= 2 * ULP, (s, ear)


# ---- aw_synth_fill, aw_memcpy_h2d, aw_memcpy_d2h -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_synth_fill_behind_the_delay(E, monkeypatch, kind):
    S, F, C = 3, 4099, 7

    def script(ctx, X, Y):
        return [("aw_synth_fill", lambda: ctx.synth_fill(Y[0].data_ptr(), S, F, C, seed=5, first_stream=2), True)]
    got, _, _, _, _ = run_both(E, monkeypatch, kind, {}, lambda ctx: ctx, [], [f32_like(S, F, C)], script, "aw_synth_fill")
    assert np.array_equal(got[0], E.oracle.synth_input(S, F, C, seed=5, first_stream=2))


@pytest.mark.parametrize("kind", ["side", "owned"])
def test_memcpy_entries_synchronise_the_contexts_stream(E, monkeypatch, kind):
    """aw_memcpy_d2h of a tensor whose producer sits behind the delay returns the produced bytes; aw_memcpy_h2d into a buffer that the
    stream poisons behind the delay is what the consumer then sees."""
    torch = E.torch
    ctx, s = context(E, monkeypatch, {}, kind)
    data = E.oracle.synth_input(2, 5003, 3, seed=9)
    sw = Sandwich(E, s, f"aw_memcpy_d2h [{kind}]")
    x = sw.input(data)
    host = np.full(data.shape, np.nan, np.float32)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        sw.hold()
        sw.produce()
        ctx.d2h(host, x.data_ptr())
    assert sw.e_delay.query()                                   # it waited for the stream the producer was on
    assert same_bits(host, data)
    sw = Sandwich(E, s, f"aw_memcpy_h2d [{kind}]")
    y = sw.output(data)
    y.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        sw.hold()
        y.view(torch.float32).fill_(float("nan"))              # behind the delay; an upload that left the stream would land in front of it
        ctx.h2d(y.data_ptr(), data)
        assert sw.e_delay.query()
        sw.consume()
    s.synchronize()
    assert same_bits(sw.results()[0], data)


# ---- two contexts on two streams ---------------------------------------------------------------------------------------------------------

def test_two_contexts_on_two_side_streams(E, monkeypatch):
    """One host thread drives two contexts, calls interleaved, the delay on one stream only, then on the other.  Each output equals its
    serial reference, and the stream without the delay finishes while the delay is still pending: nothing of one context waits behind
    the other's stream."""
    torch = E.torch
    env, channels, taps, S, calls, _ = FAMILIES["ols8192"]
    h, lt, rt, x, truth = family_case(E.oracle, "ols8192")
    ctx_r, _ = context(E, monkeypatch, env, "ref")
    ref = reference_run(E, ctx_r, split(x, calls), [f32_like(S, n, 2) for n in calls], process_script(calls), spatializer(E, ctx_r, h, lt, rt, S, max(calls)), {})
    pair = [context(E, monkeypatch, env, "side"), context(E, monkeypatch, env, "side-second")]
    assert pair[0][1].cuda_stream != pair[1][1].cuda_stream
    for delayed in (0, 1):
        sws, scripts, sps = [], [], []
        for i, (ctx, s) in enumerate(pair):
            sp = spatializer(E, ctx, h, lt, rt, S, max(calls))
            sw = Sandwich(E, s, f"two contexts, context {i}{' (delayed)' if i == delayed else ''}")
            X = [sw.input(a) for a in split(x, calls)]
            Y = [sw.output(f32_like(S, n, 2)) for n in calls]
            sws.append(sw), scripts.append(process_script(calls)(sp, X, Y)), sps.append(sp)
        done = [torch.cuda.Event(), torch.cuda.Event()]
        torch.cuda.synchronize()
        for i, (_, s) in enumerate(pair):
            with torch.cuda.stream(s):
                if i == delayed:
                    sws[i].hold()
                sws[i].produce()
        for k in range(len(calls)):                             # interleaved: A, B, A, B
            for i in range(2):
                sws[i].call([scripts[i][k]])
        for i, (_, s) in enumerate(pair):
            with torch.cuda.stream(s):
                sws[i].consume()
                done[i].record()
        done[1 - delayed].synchronize()
        assert not sws[delayed].e_delay.query() and not done[delayed].query(), f"the stream without the delay finished only after the other stream's delay (round {delayed})"
        for _, s in pair:
            s.synchronize()
        for i in range(2):
            got = [to_host(z, like) for _, z, like in sws[i].outs]
            for g, r in zip(got, ref):
                assert poison_left(g, r) == 0 and same_bits(g, r), (delayed, i)
            assert worst(E.oracle, np.concatenate(got, axis=1), truth) < TOL


# ---- teardown with work pending ----------------------------------------------------------------------------------------------------------

def test_destroying_handle_and_context_with_work_pending(E, monkeypatch):
    """aw_spatializer_destroy waits for the context's stream before it frees, aw_context_destroy leaves a borrowed stream alone: the
    spatializer, then the context, are destroyed while the sandwich is still queued; the output is right, the stream still runs torch
    work and the device reports no error."""
    torch, aw = E.torch, E.aw
    env, channels, taps, S, calls, _ = FAMILIES["ols8192"]
    h, lt, rt, x, truth = family_case(E.oracle, "ols8192")
    ctx_r, _ = context(E, monkeypatch, env, "ref")                  # (sets the knobs)
    ref = reference_run(E, ctx_r, split(x, calls), [f32_like(S, n, 2) for n in calls], process_script(calls), spatializer(E, ctx_r, h, lt, rt, S, max(calls)), {})
    s = torch.cuda.Stream()
    held = {"ctx": aw.Context(0, stream=s.cuda_stream)}
    held["sp"] = spatializer(E, held["ctx"], h, lt, rt, S, max(calls))
    sw = Sandwich(E, s, "teardown with work pending")
    X = [sw.input(a) for a in split(x, calls)]
    Y = [sw.output(f32_like(S, n, 2)) for n in calls]
    script = [(f"aw_spatializer_process, {n} frames", (lambda i=i, n=n: held["sp"].process_device(X[i].data_ptr(), Y[i].data_ptr(), n)), True) for i, n in enumerate(calls)]

    def teardown():
        sp = held.pop("sp")
        sp._lib.aw_spatializer_destroy(sp._h)                   # the handle first, then its context
        sp._h = None
        held.pop("ctx").close()
    got = sw.run(script, teardown)
    assert sw.pending
    for g, r in zip(got, ref):
        assert poison_left(g, r) == 0 and same_bits(g, r)
    assert worst(E.oracle, np.concatenate(got, axis=1), truth) < TOL
    with torch.cuda.stream(s):                                      # the borrowed stream was not destroyed
        t = torch.zeros(64, device="cuda").add_(3.0)
    s.synchronize()
    assert bool((t == 3.0).all())
    torch.cuda.synchronize()
