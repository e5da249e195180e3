"""The batch sample-rate converter on the device (aw_rateconv_*, airwave_amd.RateConverter): bit-for-bit parity with the sequential rule of
airwave_amd/csrc/device/rateconv.hpp (its g++ build in tests/emu) and the float64 bound of tests/rateconv_ref.py, the invariances the rule
promises (splitting calls in time, sharding streams over handles, buffer alignment), the contract of the entries, stream order on a busy
caller-owned stream, MixedRateBatch(output_rate=...) and the C example.  Shapes are tile-sized."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402
import rateconv_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 48000), (96000, 44100), (48000, 96000)]
SENTINEL = 12345.0
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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def device(G, x, shift=0):
    """x on the device, `shift` floats past the allocation's (at least 16-byte) boundary."""
    t = G.torch.full((x.size + shift,), float("nan"), dtype=G.torch.float32, device="cuda")
    t[shift:].copy_(G.torch.from_numpy(np.array(x, np.float32).reshape(-1)))          # (a copy: the shared cases are read-only)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * shift


def output(G, S, frames, C, extra=0, shift=0):
    """A sentinel-filled device buffer for [S][frames][C] and `extra` frames of capacity beyond."""
    t = G.torch.full((S * (frames + extra) * C + shift + 4,), SENTINEL, dtype=G.torch.float32, device="cuda")
    return t, t.data_ptr() + 4 * shift


def fetch(G, t, S, frames, C, shift=0):
    """([S][frames][C], everything behind it) of an output buffer."""
    G.torch.cuda.synchronize()
    h = t.cpu().numpy()
    assert np.all(h[:shift] == SENTINEL)
    return h[shift:shift + S * frames * C].reshape(S, frames, C).copy(), h[shift + S * frames * C:]


def process(G, rc, x, shift=0, extra=3):
    """One process call over the host array x -> the host output; the capacity beyond the count must stay untouched."""
    S, n, C = x.shape
    keep, p_in = device(G, x, shift)
    want = rc.output_frames(n)
    t, p_out = output(G, S, want, C, extra, shift)
    made = rc.process_device(p_in, n, p_out, want + extra)
    assert made == want
    y, rest = fetch(G, t, S, made, C, shift)
    assert np.all(rest == SENTINEL)
    del keep
    return y


def flush(G, rc, extra=3):
    S, C = rc.n_streams, rc.n_channels
    want = rc.flush_frames()
    t, p_out = output(G, S, want, C, extra)
    assert rc.flush_device(p_out, want + extra) == want
    y, rest = fetch(G, t, S, want, C)
    assert np.all(rest == SENTINEL)
    return y


def case(pair, C, S=3):
    """(two tiles plus three frames, then seven) of S streams and what the sequential rule makes of them; computed once, left unchanged."""
    key = (pair, C, S)
    if key not in _cases:
        L, M, T, D = emu.plan(*pair)
        n = emu.input_frames_for(2 * emu.tile(pair[0], pair[1], C), L, M, D) + 3
        rng = np.random.default_rng(pair[0] + C)
        x, x7 = rng.standard_normal((S, n, C)).astype(np.float32), rng.standard_normal((S, 7, C)).astype(np.float32)
        q = emu.Converter(pair[0], pair[1], S, C, kernel=False)
        want = [q.process(x), q.process(x7), q.flush()]
        for a in (x, x7, *want):
            a.setflags(write=False)
        _cases[key] = (x, x7, want)
    return _cases[key]


@pytest.mark.parametrize("C", [2, 7])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_device_equals_the_sequential_rule_bit_for_bit(G, pair, C):
    check_three_calls(G, pair, C)


def check_three_calls(G, pair, C, c=None, roundings=None):
    """process, process and flush of case(pair, C) against the sequential rule, bit for bit, and against the float64 evaluation with the
    coefficients c (default: the library's float32 table) within `roundings` (default: T) * 2^-24 * sum |c| |x| per sample.  Returns the
    largest |y - y64| / bound."""
    x, x7, want = case(pair, C)
    S = x.shape[0]
    rc = G.aw.RateConverter(pair[0], pair[1], S, C, ctx=G.ctx)
    info = rc.info()
    L, M, T, D = emu.plan(*pair)
    assert (info["L"], info["M"], info["taps"], info["latency"]) == (L, M, T, D) and info["tile"] == emu.tile(pair[0], pair[1], C)
    got = [process(G, rc, x), process(G, rc, x7), flush(G, rc)]
    assert 2 * info["tile"] <= got[0].shape[1] < 3 * info["tile"]                   # three workgroups per stream, the last ragged
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (pair, C, i, int((bits(g) != bits(w)).sum()))
    n_in = x.shape[1] + 7
    y = np.concatenate(got, axis=1)
    assert y.shape[1] == -(-n_in * L // M)
    assert rc.info()["frames_consumed"] == 0 and rc.info()["frames_produced"] == 0          # the flush reset them
    c = G.aw.rateconv_filter(*pair) if c is None else c
    worst = 0.0
    for s in range(S):
        y64, bound = ref.convert64(np.concatenate([x[s], x7[s]]), L, M, D, c, flushed=True, with_bound=True)          # (T roundings)
        if roundings is not None:
            bound = bound * (roundings / T)
        worst = max(worst, float((np.abs(y[s] - y64) / np.maximum(bound, 1e-300)).max()))
        assert np.all(np.abs(y[s] - y64) <= bound), (pair, C, s, worst)
    print(f"{pair} C={C}: largest |y - y64| / bound = {worst:.3f}")
    return worst


def test_cutting_calls_in_time_changes_no_bit(G):
    pair, C = (96000, 44100), 2
    x, _, want = case(pair, C)
    S, n, _ = x.shape
    L, M, T, D = emu.plan(*pair)
    tile = emu.tile(pair[0], pair[1], C)
    # 1 frame, D frames (the first output), as many as make one tile of outputs more, the rest
    cuts = [0, 1, 1 + D, emu.input_frames_for(1 + tile, L, M, D), n]
    rc = G.aw.RateConverter(pair[0], pair[1], S, C, ctx=G.ctx)
    parts = [process(G, rc, np.ascontiguousarray(x[:, a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    assert parts[0].shape[1] == 0 and parts[1].shape[1] == 1 and parts[2].shape[1] == tile
    assert rc.info()["frames_consumed"] == n and rc.info()["frames_produced"] == want[0].shape[1]
    assert same(np.concatenate(parts, axis=1), want[0])


def test_sharding_streams_over_handles_changes_no_bit(G):
    pair, C = (44100, 48000), 7
    x, x7, want = case(pair, C, S=5)
    whole = G.aw.RateConverter(pair[0], pair[1], 5, C, ctx=G.ctx)
    y = np.concatenate([process(G, whole, x), process(G, whole, x7), flush(G, whole)], axis=1)
    halves = []
    for a, b in ((0, 2), (2, 5)):
        rc = G.aw.RateConverter(pair[0], pair[1], b - a, C, ctx=G.ctx)
        halves.append(np.concatenate([process(G, rc, np.ascontiguousarray(x[a:b])), process(G, rc, np.ascontiguousarray(x7[a:b])), flush(G, rc)], axis=1))
    assert same(np.concatenate(halves, axis=0), y) and same(y, np.concatenate(want, axis=1))


def test_a_buffer_shifted_by_one_float_changes_no_bit(G):
    pair, C = (48000, 96000), 7
    x, _, want = case(pair, C)
    for shift in (0, 1):
        rc = G.aw.RateConverter(pair[0], pair[1], x.shape[0], C, ctx=G.ctx)
        assert same(process(G, rc, x, shift=shift), want[0]), shift


def test_contract_of_the_entries(G):
    torch, aw = G.torch, G.aw
    pair, C, S = (44100, 48000), 2, 2
    L, M, T, D = emu.plan(*pair)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((S, 3000, C)).astype(np.float32)
    # allocations: all of them in create, counted on the context, none afterwards
    meter = aw.Spatializer(aw.HRIR(np.ones((2, 8), np.float32), 48000.0, ctx=G.ctx), [0, 1], [1, 0], 1, ctx=G.ctx)
    a0 = meter.info()["device_allocs"]
    rc = aw.RateConverter(pair[0], pair[1], S, C, ctx=G.ctx)
    a1 = meter.info()["device_allocs"]
    assert a1 == a0 + 4                                                             # the table, two history slots, the counts
    # a zero-output call: AW_OK, *out_frames == 0, nothing written
    assert rc.output_frames(D) == 0
    t, p = output(G, S, 0, C, extra=2)
    keep, p_in = device(G, x[:, :D])
    assert rc.process_device(p_in, D, p, 2) == 0
    assert np.all(fetch(G, t, S, 0, C)[1] == SENTINEL)
    assert rc.info()["frames_consumed"] == D and rc.info()["frames_produced"] == 0
    # a short capacity is refused and changes nothing: the next call's output proves it
    n = 2000
    want = rc.output_frames(n)
    assert want == ref.output_count(D + n, L, M, D)
    keep2, p_in2 = device(G, np.ascontiguousarray(x[:, D:D + n]))
    t, p = output(G, S, want, C)
    with pytest.raises(aw.AirwaveError) as e:
        rc.process_device(p_in2, n, p, want - 1)
    assert e.value.name == "INVALID_ARGUMENT" and "capacity" in str(e.value)
    assert np.all(fetch(G, t, S, want, C)[0] == SENTINEL)
    assert rc.info()["frames_consumed"] == D and rc.output_frames(n) == want
    y = process(G, rc, np.ascontiguousarray(x[:, D:D + n]))
    q = emu.Converter(pair[0], pair[1], S, C, kernel=False)
    q.process(x[:, :D])
    assert same(y, q.process(x[:, D:D + n]))
    # flush totals ceil(N L / M); reset restarts from silence
    tail = flush(G, rc)
    assert same(tail, q.flush()) and y.shape[1] + tail.shape[1] == -(-(D + n) * L // M)
    first = process(G, rc, x)
    rc.reset()
    assert rc.info()["frames_consumed"] == 0
    assert same(process(G, rc, x), first)
    # refusals that need a live handle
    lib = aw._capi.load()
    n64 = ctypes.c_int64(-7)
    assert lib.aw_rateconv_process(rc._h, None, 5, None, 0, ctypes.byref(n64)) == 1 and n64.value == -7
    assert lib.aw_rateconv_process(rc._h, ctypes.c_void_p(p_in + 2), 5, None, 0, ctypes.byref(n64)) == 1          # off a float
    assert lib.aw_rateconv_process(rc._h, ctypes.c_void_p(p_in), -1, None, 0, ctypes.byref(n64)) == 1
    for bad in ((44100, 44100, 1, 2), (44100, 48000, 0, 2), (44100, 48000, 1, 0), (44100, 48000, 1, 17), (48000, 44101, 1, 2)):
        with pytest.raises(aw.AirwaveError) as e:
            aw.RateConverter(*bad, ctx=G.ctx)
        assert e.value.name == "INVALID_ARGUMENT"
    # no device allocation after create: the library's own count, then (every kernel loaded) the device's free memory
    assert meter.info()["device_allocs"] == a1
    rc.reset()
    keep3, p_all = device(G, x)
    t, p = output(G, S, rc.output_frames(x.shape[1]) + 100, C)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(2):
        rc.process_device(p_all, x.shape[1], p, rc.output_frames(x.shape[1]))
        rc.flush_device(p, 100)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0
    assert meter.info()["device_allocs"] == a1
    del keep, keep2, keep3


def test_one_shot_convert(G):
    pair, C = (48000, 96000), 2
    x, x7, want = case(pair, C)
    y = G.aw.convert(np.concatenate([x, x7], axis=1), pair[0], pair[1], ctx=G.ctx)
    assert same(y, np.concatenate(want, axis=1))
    assert G.aw.convert(x[0], pair[0], pair[1], ctx=G.ctx).shape == (2 * x.shape[1], C)


def test_stream_order_on_a_busy_caller_owned_stream(G):
    """Producer, converter and consumer on a caller's side stream behind a delay, no host synchronisation in between: the output is the
    synchronised run's, and the calls returned while the delay was still pending."""
    from test_gpu_stream_order import DELAY_MS, Delay, Sandwich, poison_left, same_bits, side_stream
    torch, aw = G.torch, G.aw
    E = Env()
    E.torch, E.aw = torch, aw
    E.delay = Delay(torch, DELAY_MS)
    E.probe = torch.zeros(64, device="cuda")
    pair, C = (44100, 48000), 2
    x, x7, want = case(pair, C)
    S, n, _ = x.shape
    s = side_stream(E, [torch.cuda.default_stream()])
    ctx = aw.Context(0, stream=s.cuda_stream)
    rc = aw.RateConverter(pair[0], pair[1], S, C, ctx=ctx)
    counts = {}
    sw = Sandwich(E, s, "aw_rateconv_process, _process, _flush")
    X = [sw.input(x), sw.input(x7)]
    Y = [sw.output(w) for w in want]

    def call(i, frames):
        return lambda: counts.__setitem__(i, rc.process_device(X[i].data_ptr(), frames, Y[i].data_ptr(), want[i].shape[1]))
    got = sw.run([("aw_rateconv_process, two tiles + 3", call(0, n), True), ("aw_rateconv_process, 7 frames", call(1, 7), True),
                  ("aw_rateconv_flush", lambda: counts.__setitem__(2, rc.flush_device(Y[2].data_ptr(), want[2].shape[1])), True)])
    print(f"{sw.what}: the delay held the stream {sw.delay_ms:.1f} ms; still pending when the last call returned: {sw.pending}")
    assert [counts[i] for i in range(3)] == [w.shape[1] for w in want]
    for g, w in zip(got, want):
        assert poison_left(g, w) == 0 and same_bits(g, np.asarray(w))
    assert sw.pending, "the calls returned only after the delay had run: they did not just enqueue"
    rc.close()
    ctx.close()


def test_mixed_rate_batch_with_an_output_rate(G, golden_dir):
    aw = G.aw
    from test_gpu_full_size import SPEAKERS7
    w = aw.WAVLoader.load(os.path.join(golden_dir, "hrtf", "StageSH1.0.wav"))
    layout = aw.InputLayout(SPEAKERS7, "7 speakers")
    rates = [44100.0, 48000.0, 96000.0, 44100.0, 48000.0, 96000.0]
    frames = {44100.0: 3001, 48000.0: 3000, 96000.0: 5003}
    rng = np.random.default_rng(4)
    streams = [(0.1 * rng.standard_normal((frames[r], 7))).astype(np.float32) for r in rates]
    tracks = np.asarray(w.audio_data)
    plain = aw.MixedRateBatch(tracks, w.sample_rate, layout, rates, ctx=G.ctx)
    assert plain.output_rate is None and all(b.converter is None for b in plain.buckets.values())
    y_plain = plain.process(streams, rates)
    batch = aw.MixedRateBatch(tracks, w.sample_rate, layout, rates, ctx=G.ctx, output_rate=48000)
    assert batch.buckets[48000.0].converter is None and batch.buckets[44100.0].converter.n_channels == 2
    y = batch.process(streams, rates)
    for i, r in enumerate(rates):
        assert y_plain[i].shape == (frames[r], 2)
        if r == 48000.0:
            assert same(y[i], y_plain[i])                                           # the bucket that is at the rate already: the same bits
            continue
        L, M, T, D = emu.plan(r, 48000)
        assert y[i].shape == (-(-frames[r] * L // M), 2)
        q = emu.Converter(r, 48000, 1, 2, kernel=False)
        want = np.concatenate([q.process(y_plain[i][None]), q.flush()], axis=1)[0]
        assert np.abs(want).max() > 1e-3 and same(y[i], want), (i, r)
    # the device entry: per-bucket capacities in, the counts out; the rest comes with the flush
    torch = G.torch
    ins = {r: torch.from_numpy(np.stack([streams[i] for i in batch.buckets[r].stream_ids])).cuda() for r in frames}
    cap = {r: y[batch.buckets[r].stream_ids[0]].shape[0] + 8 for r in frames}          # (frames at the output rate)
    outs = {r: torch.full((2, cap[r], 2), SENTINEL, dtype=torch.float32, device="cuda") for r in frames}
    batch.reset()
    counts = batch.process_device({r: t.data_ptr() for r, t in ins.items()}, {r: t.data_ptr() for r, t in outs.items()}, frames, cap)
    torch.cuda.synchronize()
    for r in frames:
        b = batch.buckets[r]
        if b.converter is None:
            assert counts[r] == frames[r]
        else:
            L, M, T, D = emu.plan(r, 48000)
            assert counts[r] == ref.output_count(frames[r], L, M, D)
        flat = outs[r].cpu().numpy().reshape(-1)                                    # dense in the count, whatever the capacity
        got = flat[:2 * counts[r] * 2].reshape(2, counts[r], 2)
        assert np.all(flat[2 * counts[r] * 2:] == SENTINEL)
        for k, i in enumerate(b.stream_ids):
            assert same(got[k], y[i][:counts[r]]), (r, k)
    tails = {r: torch.full((2, 64, 2), SENTINEL, dtype=torch.float32, device="cuda") for r in (44100.0, 96000.0)}
    rest = batch.flush_device({r: t.data_ptr() for r, t in tails.items()}, {r: 64 for r in tails})
    torch.cuda.synchronize()
    for r, t in tails.items():
        assert counts[r] + rest[r] == y[batch.buckets[r].stream_ids[0]].shape[0]
        got = t.cpu().numpy().reshape(-1)[:2 * rest[r] * 2].reshape(2, rest[r], 2)
        for k, i in enumerate(batch.buckets[r].stream_ids):
            assert same(got[k], y[i][counts[r]:]), (r, k)


def test_the_example_runs_and_prints_the_expected_counts(G, golden_dir):
    from test_example_resample import EXE, build
    build()
    S, seconds = 3, 0.05
    r = subprocess.run([EXE, os.path.join(golden_dir, "hrtf", "RoomSH1.0.wav"), str(S), str(seconds)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "bucket 44100 Hz -> 48000 Hz: L 160 M 147 taps 96 latency 48; 3 streams, 2205 frames in, 2348 + 52 = 2400 frames out" in r.stdout
    assert "bucket 96000 Hz -> 48000 Hz: L 1 M 2 taps 192 latency 96; 3 streams, 4800 frames in, 2352 + 48 = 2400 frames out" in r.stdout
    rows = re.findall(r"stream (\d+) at (\d+) Hz: (\d+) frames at 48000 Hz, peak ([\d.]+)", r.stdout)
    assert [(int(a), int(b), int(c)) for a, b, c, _ in rows] == [(i, rate, 2400) for rate in (44100, 96000) for i in range(S)]
    assert all(0.001 < float(p) < 10.0 for *_, p in rows), rows
