"""Target changes of the batch entries' equalizer stage on the MI355X (aw_spatializer_set_equalizer_target): a published target is faded
to over T = max(1, round(0.020 * rate)) frames on one clock per handle, as ParametricEqualizerProcessor.setTarget does.

References.  aw_eq (ParametricEqualizerProcessor on the device, n_streams = a group of streams with one target history) over the stage-off
output of the same calls, its targets set before the same calls and drained after each: bit for bit.  The oracle's processor over the same
float32 input in pieces of at most 4096 frames: within 2 ULP on the frames of a fade (each rendering is within ULP of the oracle's, a
convex mix of two such values is too, and the final float32 rounding adds at most ULP at |y| < 1) and ULP elsewhere, ULP = 6e-8 as in
tests/test_gpu_eq_stage.py.  A stream that is not part of a change (KEEP): the two-call path that file holds the stage to —
ParametricEqualizerState over the stage-off output — fed the pieces the clock cuts the calls into, bit for bit.  (A second handle cannot
be given the pieces as calls of its own: the convolution in front of the stage depends on how its calls are cut.)"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_eq_stage import A, B, LT, PRESETS, RT, TAPS, ULP, adef, bits, cut, ear_split_off_context, odef
from test_gpu_eq_stage import noise as stage_noise
from test_gpu_loudness import device_call, host_call
from test_gpu_pcm_dither import F32, S16, S24, context, encode

pytestmark = pytest.mark.gpu

KEEP = -2
S9 = 9
# Input level.  The bounds are absolute and stand on |y| < 1 (one float32 ulp is 2^-24 there): at tests/test_gpu_eq_stage.py's 0.15 the
# 64-filter preset reaches 1.06 on some of the longer noises used here, at 0.1 it stays under 0.75.  check_bounds asserts the premise.
LEVEL = 0.1


def noise(seed, streams, frames):
    return stage_noise(seed, streams, frames, LEVEL)


def fade_length(rate):
    return max(1, int(np.floor(rate * 0.020 + 0.5)))


def make(aw, ctx, oracle, streams, rate=48000.0, stream_map=None):
    sp = aw.Spatializer(aw.HRIR(oracle.synth_hrir(2, TAPS, seed=61), sample_rate=rate, ctx=ctx), LT, RT, n_streams=streams, ctx=ctx)
    if stream_map is not None:
        sp.set_equalizer([adef(aw, p) for p in PRESETS], stream_map)
    return sp


def target(aw, sp, entries):
    """entries: per stream an index into PRESETS, -1 or KEEP."""
    sp.set_equalizer_target([adef(aw, p) for p in PRESETS], entries)


class Clock:
    """The rule, written out: a published target begins with the next call or where the running fade ends; a call is cut there."""

    def __init__(self, T):
        self.T, self.t, self.fading, self.pending = T, 0, False, False

    def publish(self):
        self.pending = True

    def cuts(self, frames):
        """[(first, frames, t0 or None, begins, ends)] of one call."""
        out, pos = [], 0
        while pos < frames:
            begins = False
            if not self.fading and self.pending:
                self.fading, self.pending, self.t, begins = True, False, 0, True
            if not self.fading:
                out.append((pos, frames - pos, None, False, False))
                break
            n = min(self.T - self.t, frames - pos)
            ends = self.t + n == self.T
            out.append((pos, n, self.t, begins, ends))
            self.t, pos = self.t + n, pos + n
            if ends:
                self.fading, self.t = False, 0
        return out


def fma64(a, b, c):
    """a * b + c rounded once, element by element (exact rationals; numpy has no fused multiply-add)."""
    a, b, c = np.broadcast_arrays(a, b, c)
    out = np.empty(a.shape, np.float64)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def fading_mask(cuts, frames):
    m = np.zeros(frames, bool)
    for first, n, t0, _, _ in cuts:
        if t0 is not None:
            m[first:first + n] = True
    return m


def oracle_processor_run(oracle, rate, publications, ys):
    """One stream: publications {call index: oracle definition or None (unity)}; ys: its float32 input per call -> output per call."""
    proc = oracle.ParametricEqualizerProcessor(rate)
    outs = []
    for i, y in enumerate(ys):
        if i in publications:
            proc.set_target(publications[i])
        o = np.empty_like(y)
        for at in range(0, y.shape[0], 4096):
            o[at:at + 4096, 0], o[at:at + 4096, 1] = proc.process(y[at:at + 4096, 0], y[at:at + 4096, 1])
            proc.drain_retired_states()
        outs.append(o)
    return outs


def check_bounds(got, want, mask, what):
    err = np.max(np.abs(got.astype(np.float64) - want), axis=1)
    e_fade, e_rest = (err[mask].max() if mask.any() else 0.0), (err[~mask].max() if (~mask).any() else 0.0)
    print(f"{what}: fade frames {int(mask.sum())} max err {e_fade:.3e} (bound {2 * ULP:.1e}), other frames {e_rest:.3e} (bound {ULP:.1e}), peak {np.abs(got).max():.3f}")
    assert np.abs(got).max() < 1.0
    assert e_fade <= 2 * ULP and e_rest <= ULP, (what, e_fade, e_rest)


# ---- 1. aw_eq, bit for bit ---------------------------------------------------------------------------------------------------------------

FIRST = [0, 0, 0, 1, 1, 1, 2, 2, -1]
SECOND = [1, 1, 1, 2, 2, 2, -1, -1, 0]


@pytest.mark.parametrize("form", ["ear_per_workgroup", "both_ears"])
@pytest.mark.parametrize("calls", [[500, 500, 3000], [20000]])
@pytest.mark.parametrize("rate", [48000.0, 44100.0])
def test_stage_off_then_targets_equal_aw_eq_bit_for_bit(oracle, rate, calls, form):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch) if form == "ear_per_workgroup" else ear_split_off_context(aw, torch)
    T = fade_length(rate)
    xs = cut(noise(int(rate) + sum(calls), S9, sum(calls)), calls)
    plain, staged = make(aw, ctx, oracle, S9, rate), make(aw, ctx, oracle, S9, rate)
    publications = {0: FIRST, 1: SECOND} if len(calls) > 1 else {0: FIRST}      # the second one while the first fade runs
    ys, got = [], []
    clock, masks = Clock(T), []
    for i, x in enumerate(xs):
        if i in publications:
            target(aw, staged, publications[i])
            clock.publish()
            assert staged.info()["equalizer_pending"] == 1
        ys.append(plain.process(x))
        got.append(staged.process(x))
        masks.append(fading_mask(clock.cuts(x.shape[1]), x.shape[1]))
        assert staged.info()["equalizer_fade"] == (T - clock.t if clock.fading else 0) and staged.info()["equalizer_pending"] == int(clock.pending)
    assert plain.info()["equalizer"] == 0 and staged.info()["equalizer_fade"] == 0
    groups = {}
    for s in range(S9):
        groups.setdefault(tuple(p[s] for p in publications.values()), []).append(s)
    for history, idx in groups.items():
        proc = aw.ParametricEqualizerProcessor(rate, 0, n_streams=len(idx), ctx=ctx)
        assert proc.transitionLength == T
        for i, y in enumerate(ys):
            if i in publications:
                e = publications[i][idx[0]]
                proc.setTarget(None if e < 0 else adef(aw, PRESETS[e]))
            want = proc.process_batch(np.ascontiguousarray(y[idx]))
            proc.drainRetiredStates()
            assert np.array_equal(bits(got[i][idx]), bits(want)), (history, i)
        s = idx[0]
        ref = oracle_processor_run(oracle, rate, {i: (None if p[s] < 0 else odef(oracle, PRESETS[p[s]])) for i, p in publications.items()}, [y[s] for y in ys])
        for i in range(len(calls)):
            check_bounds(got[i][s], ref[i], masks[i], f"rate {rate} calls {calls} {form} stream {s} history {history} call {i}")


# ---- 2. an installed preset, then a target -------------------------------------------------------------------------------------------

def test_installed_presets_then_a_target(oracle):
    """set_equalizer, two calls, set_equalizer_target, two calls.  Bit for bit against ParametricEqualizerState.process_batch over the
    pieces (the installed preset's state going on, the target's from zero) mixed in float64 as aw_eq's blend kernel mixes (its old-side
    product is fused into the sum: fma64); within the bounds of the oracle's states composed the same way with the reference's mix."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    rate, T = 48000.0, 960
    installed = [0, 1, 2, -1, 0, 1, 2, -1, 0]
    to = [1, 2, 0, 0, -1, 1, 2, -1, 2]             # preset -> preset, -1 -> preset, preset -> -1, the same preset again, -1 -> -1
    calls = [700, 1300, 500, 2000]
    xs = cut(noise(91, S9, sum(calls)), calls)
    plain, staged = make(aw, ctx, oracle, S9, rate), make(aw, ctx, oracle, S9, rate, installed)
    ys, got, clock, pieces = [], [], Clock(T), []
    for i, x in enumerate(xs):
        if i == 2:
            target(aw, staged, to)
            clock.publish()
            assert staged.info()["equalizer"] == 6                # the installed presets and the targets': the table holds what some map names
        ys.append(plain.process(x))
        got.append(staged.process(x))
        pieces.append(clock.cuts(x.shape[1]))
    assert pieces[2] == [(0, 500, 0, True, False)] and pieces[3] == [(0, 460, 500, False, True), (460, 1540, None, False, False)]
    for s in range(S9):
        def device_states():
            a = None if installed[s] < 0 else aw.ParametricEqualizerState(adef(aw, PRESETS[installed[s]]), rate, n_streams=1, ctx=ctx)
            b = None if to[s] < 0 else aw.ParametricEqualizerState(adef(aw, PRESETS[to[s]]), rate, n_streams=1, ctx=ctx)
            run = lambda st, v: v if st is None else st.process_batch(np.ascontiguousarray(v[None]))[0]
            return a, b, run

        def oracle_states():
            a = None if installed[s] < 0 else oracle.eq_prepare(odef(oracle, PRESETS[installed[s]]), rate)
            b = None if to[s] < 0 else oracle.eq_prepare(odef(oracle, PRESETS[to[s]]), rate)
            run = lambda st, v: v if st is None else np.stack(st.process(v[:, 0], v[:, 1]), axis=1)
            return a, b, run

        for name, (a, b, run) in (("device", device_states()), ("oracle", oracle_states())):
            active = a
            for i, y in enumerate(ys):
                want, mask = np.empty_like(y[s]), fading_mask(pieces[i], y.shape[1])
                for first, n, t0, begins, ends in pieces[i]:
                    v = y[s, first:first + n]
                    if t0 is None:
                        want[first:first + n] = run(active, v)
                        continue
                    o, w = run(a, v).astype(np.float64), run(b, v).astype(np.float64)
                    g = ((t0 + np.arange(n) + 1).astype(np.float64) / float(T))[:, None]
                    # the device's mix is aw_eq's: the old side's product fused into the sum; the oracle's is the reference's, unfused
                    want[first:first + n] = (fma64(o, 1.0 - g, w * g) if name == "device" else o * (1.0 - g) + w * g).astype(np.float32)
                    if ends:
                        active = b
                if name == "device":
                    assert np.array_equal(bits(got[i][s]), bits(want)), (s, i)
                else:
                    check_bounds(got[i][s], want, mask, f"stream {s} ({installed[s]} -> {to[s]}) call {i}")


# ---- 3. KEEP and -1 ----------------------------------------------------------------------------------------------------------------------

def test_keep_streams_and_unity(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    rate, T = 48000.0, 960
    installed = [0, 1, 2, -1, 0, 1, 2, -1, 0]
    to = [KEEP, KEEP, KEEP, KEEP, 1, -1, KEEP, 0, KEEP]
    calls = [1000, 500, 1500, 64]
    xs = cut(noise(92, S9, sum(calls)), calls)
    plain, staged = make(aw, ctx, oracle, S9, rate), make(aw, ctx, oracle, S9, rate, installed)
    clock = Clock(T)
    keep_states = {s: aw.ParametricEqualizerState(adef(aw, PRESETS[installed[s]]), rate, n_streams=1, ctx=ctx) for s in range(S9) if to[s] == KEEP and installed[s] >= 0}
    for i, x in enumerate(xs):
        if i == 1:
            target(aw, staged, to)
            clock.publish()
        y, got = plain.process(x), staged.process(x)
        pieces = clock.cuts(x.shape[1])
        for s, st in keep_states.items():             # the pieces as calls of the two-call path
            want = np.concatenate([st.process_batch(np.ascontiguousarray(y[s:s + 1, first:first + n]))[0] for first, n, *_ in pieces])
            assert np.array_equal(bits(got[s]), bits(want)), (i, s)
        assert np.array_equal(bits(got[3]), bits(y[3])), i                      # -1 and KEEP: never touched
        if i == 0:
            assert np.array_equal(bits(got[7]), bits(y[7]))                      # -1 before its fade
        if i == 2:                                                               # the fade ends at frame 460 of this call
            assert pieces[0][:2] == (0, 460) and pieces[0][4]
            assert np.array_equal(bits(got[5][460:]), bits(y[5][460:])) and not np.array_equal(bits(got[5][:460]), bits(y[5][:460]))
        if i == 3:
            assert np.array_equal(bits(got[5]), bits(y[5]))                      # faded to -1: it keeps its samples
            assert not np.array_equal(bits(got[7]), bits(y[7]))                  # faded from -1 to a preset
    assert staged.info()["equalizer_fade"] == 0 and staged.info()["equalizer_pending"] == 0


# ---- 4. a fade longer than a span ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["ear_per_workgroup", "both_ears"])
def test_rate_441000_fade_crosses_the_span_carry(oracle, form):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch) if form == "ear_per_workgroup" else ear_split_off_context(aw, torch)
    rate, F = 441000.0, 12000
    T = fade_length(rate)
    assert T == 8820 == 8192 + 19 * 32 + 20
    x = noise(93, S9, F)
    plain, staged = make(aw, ctx, oracle, S9, rate), make(aw, ctx, oracle, S9, rate)
    target(aw, staged, FIRST)
    y, got = plain.process(x), staged.process(x)
    mask = np.arange(F) < T
    for s in (0, 3, 6, 8):
        ref = oracle_processor_run(oracle, rate, {0: None if FIRST[s] < 0 else odef(oracle, PRESETS[FIRST[s]])}, [y[s]])[0]
        check_bounds(got[s], ref, mask, f"rate 441000 {form} stream {s} -> {FIRST[s]}")
    assert staged.info()["equalizer_fade"] == 0


# ---- 5. chunking, formats, buffers, sharding -----------------------------------------------------------------------------------------

def test_chunking_formats_buffers_and_sharding_change_no_bit(oracle):
    import torch
    import airwave_amd as aw
    S, F = 9, 40003                                                  # AW_HOST_CHUNK_MB=1 takes three streams a chunk
    T = 960
    ctx, small = context(aw, torch, chunk_mb=64), context(aw, torch, chunk_mb=1)
    installed = [0, 1, 2, -1, 0, 1, 2, -1, 0]
    to = [1, KEEP, 0, 2, -1, KEEP, 1, KEEP, 2]
    warm, x, x2 = noise(94, S, 300), noise(95, S, F), noise(96, S, 500)
    chunks = []

    def run(sp, call, fout=F32, first=0, k=S):
        """a short call, the target, a long call with the whole fade in it, a second target, a short call that ends inside its fade"""
        call(sp, warm[first:first + k])
        target(aw, sp, to[first:first + k])
        out = call(sp, x[first:first + k], fout)
        chunks.append(sp.info()["host_chunk_streams"])
        assert sp.info()["equalizer_fade"] == 0 and sp.info()["equalizer_pending"] == 0
        target(aw, sp, installed[first:first + k])
        out2 = call(sp, x2[first:first + k], fout)
        assert sp.info()["equalizer_fade"] == T - 500                # the clock moved once, however many chunks of streams ran
        return out, out2

    dev = lambda sp, v, fout=F32: device_call(torch, sp, v, fout)
    one, one2 = run(make(aw, ctx, oracle, S, stream_map=installed), dev)
    chunked, chunked2 = run(make(aw, small, oracle, S, stream_map=installed), host_call)
    assert 0 < chunks[-1] < S, chunks                                # the call with the whole fade in it ran in chunks of streams
    assert chunked.tobytes() == one.tobytes() and chunked2.tobytes() == one2.tobytes()
    for fmt in (S16, S24):
        enc, enc2 = run(make(aw, ctx, oracle, S, stream_map=installed), dev, fmt)
        assert enc.tobytes() == encode(fmt, one)[0].tobytes() and enc2.tobytes() == encode(fmt, one2)[0].tobytes()
        enc, enc2 = run(make(aw, small, oracle, S, stream_map=installed), host_call, fmt)
        assert enc.tobytes() == encode(fmt, one)[0].tobytes() and enc2.tobytes() == encode(fmt, one2)[0].tobytes()

    def pinned_call(sp, v, fout=F32):
        xin, y = sp.ctx.pinned_empty(v.shape, np.float32), sp.ctx.pinned_empty(v.shape, np.float32)
        xin[...] = v
        sp.process_host_into(xin, y, out_format="f32")
        return np.array(y)

    pinned, pinned2 = run(make(aw, small, oracle, S, stream_map=installed), pinned_call)
    assert pinned.tobytes() == one.tobytes() and pinned2.tobytes() == one2.tobytes()
    shards = [run(make(aw, ctx, oracle, k, stream_map=installed[first:first + k]), dev, F32, first, k) for first, k in ((0, 4), (4, 5))]
    assert np.concatenate([a for a, _ in shards]).tobytes() == one.tobytes() and np.concatenate([b for _, b in shards]).tobytes() == one2.tobytes()


def test_single_stream_callback_path_fades_like_a_batch(oracle):
    """One stream, callback-sized calls of the host entry: the fade's kernels run in place over the page-locked output.  Bit for bit aw_eq
    over that path's own stage-off output."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    rate, calls = 48000.0, [300, 500, 33, 4096, 100]
    xs = cut(noise(97, 1, sum(calls)), calls)
    plain, staged = make(aw, ctx, oracle, 1, rate), make(aw, ctx, oracle, 1, rate)
    for sp in (plain, staged):
        sp.reserve_host(4096)
    proc = aw.ParametricEqualizerProcessor(rate, 0, n_streams=1, ctx=ctx)
    for i, x in enumerate(xs):
        if i == 1:
            target(aw, staged, [1])
            proc.setTarget(adef(aw, B))
        if i == 2:                                                   # while the fade runs: begins 427 frames into the fourth call
            target(aw, staged, [0])
            proc.setTarget(adef(aw, A))
        y, got = host_call(plain, x), host_call(staged, x)
        assert staged.info()["host_chunk_streams"] == 0
        want = proc.process_batch(y)
        proc.drainRetiredStates()
        assert np.array_equal(bits(got), bits(want)), i
    assert staged.info()["equalizer_fade"] == 0 and staged.info()["equalizer_pending"] == 0


# ---- 6. later stages -----------------------------------------------------------------------------------------------------------------

def test_the_meter_sees_the_faded_signal(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, F = 5, 1500
    x = noise(99, S, F)
    sp = make(aw, ctx, oracle, S, stream_map=[0, 1, 2, -1, 0])
    sp.set_metering(True)
    target(aw, sp, [2, 2, 0, 2, KEEP])                               # +6 dB on most: the faded signal's peak is not the old one's
    out = device_call(torch, sp, x)
    lv = sp.levels()
    assert np.array_equal(lv["peak"], np.abs(out).max(axis=1)) and np.all(lv["frames"] == F)
    plain = make(aw, ctx, oracle, S, stream_map=[0, 1, 2, -1, 0])
    assert not np.array_equal(np.abs(device_call(torch, plain, x)).max(axis=1)[:4], lv["peak"][:4])


# ---- 7. lifecycle and refusals ---------------------------------------------------------------------------------------------------------

def test_lifecycle_and_refusals(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, F, T = 5, 4131, 960
    m = [0, -1, 1, 0, 2]
    x = noise(100, S, F)
    names = lambda sp: [n for n, _, _ in sp.stage_times()]
    fade_names = {"aw_eq_stage_fade_kernel", "aw_eq_stage_fade_tail_kernel", "aw_eq_stage_turn_kernel"}
    # nothing published: the stage's own kernels, the stage's own bits — before any target, and again once a fade is over
    only, sp = make(aw, ctx, oracle, S, stream_map=m), make(aw, ctx, oracle, S, stream_map=m)
    for h in (only, sp):
        h.set_profiling(True)
    assert np.array_equal(bits(device_call(torch, sp, x)), bits(device_call(torch, only, x)))
    ctx.synchronize()
    assert names(sp) == names(only) and not fade_names & set(names(sp))
    target(aw, sp, [KEEP, KEEP, KEEP, 1, KEEP])
    assert (sp.info()["equalizer_fade"], sp.info()["equalizer_pending"]) == (0, 1)
    sp.set_profiling(True)
    device_call(torch, sp, x[:, :500])                               # 15 chunks and 20 frames of the fade
    device_call(torch, sp, x)                                        # its other 460 frames, then the stage alone
    ctx.synchronize()
    assert fade_names <= set(names(sp)), names(sp)
    for h in (only, sp):
        h.set_profiling(True)
    a, b = device_call(torch, sp, x), device_call(torch, only, x)
    ctx.synchronize()
    assert names(sp) == names(only) and not fade_names & set(names(sp))
    assert np.array_equal(bits(a[1]), bits(b[1])) and not np.array_equal(bits(a[3]), bits(b[3]))
    allocs = sp.info()["device_allocs"]
    target(aw, sp, [1, 1, 1, 1, 1])
    after_setter = sp.info()["device_allocs"]
    assert after_setter > allocs                                     # the setter allocates ...
    device_call(torch, sp, x[:, :500])
    device_call(torch, sp, x)
    assert sp.info()["device_allocs"] == after_setter                # ... the process path does not

    # set_equalizer ends a fade and a published target
    sp = make(aw, ctx, oracle, S, stream_map=m)
    target(aw, sp, [1, 1, 1, 1, 1])
    device_call(torch, sp, x[:, :100])
    target(aw, sp, [2, 2, 2, 2, 2])
    assert (sp.info()["equalizer_fade"], sp.info()["equalizer_pending"]) == (T - 100, 1)
    sp.set_equalizer([adef(aw, p) for p in PRESETS], m)
    assert (sp.info()["equalizer_fade"], sp.info()["equalizer_pending"], sp.info()["equalizer"]) == (0, 0, 3)
    fresh = make(aw, ctx, oracle, S, stream_map=m)
    device_call(torch, fresh, x[:, :100])
    fresh.set_equalizer([adef(aw, p) for p in PRESETS], m)
    sp.set_profiling(True)
    assert np.array_equal(bits(device_call(torch, sp, x)), bits(device_call(torch, fresh, x)))
    ctx.synchronize()
    assert not fade_names & set(names(sp))

    # reset: every state from zero, the clock where it was
    sp, twin = make(aw, ctx, oracle, S, stream_map=m), make(aw, ctx, oracle, S, stream_map=m)
    target(aw, sp, [1, 2, 0, KEEP, -1])
    device_call(torch, sp, x[:, :300])
    sp.reset()
    assert (sp.info()["equalizer_fade"], sp.info()["equalizer_pending"]) == (T - 300, 0)
    # the twin reaches the same clock with silence: all of its states are zero there too, and its convolution history as well
    target(aw, twin, [1, 2, 0, KEEP, -1])
    device_call(torch, twin, np.zeros((S, 300, 2), np.float32))
    assert np.array_equal(bits(device_call(torch, sp, x)), bits(device_call(torch, twin, x)))

    # refusals: the status, and the stage, the clock, the published target and the next call's bits as they were
    sp, twin = make(aw, ctx, oracle, S, stream_map=m), make(aw, ctx, oracle, S, stream_map=m)
    for h in (sp, twin):
        target(aw, h, [1, 1, KEEP, 2, -1])
        device_call(torch, h, x[:, :200])
        target(aw, h, [KEEP, 0, 0, KEEP, 2])
    lib = sp._lib
    fn = lib.aw_spatializer_set_equalizer_target
    handles = [adef(aw, p)._handle() for p in PRESETS]
    bad_filter = aw.EqualizerDefinition(0.0, [aw.EqualizerFilter(7, None, True, 0, 1000.0, 1.0, 1.0), aw.EqualizerFilter(9, None, True, 0, 30000.0, 1.0, 1.0)])._handle()
    too_many = aw.EqualizerDefinition(0.0, [aw.EqualizerFilter(1, None, True, 0, 500.0 + i, 1.0, 1.0) for i in range(65)])._handle()
    huge = aw.EqualizerDefinition(1e9, [])._handle()
    try:
        arr = lambda hs: ctypes.cast((ctypes.c_void_p * len(hs))(*hs), ctypes.POINTER(ctypes.c_void_p))
        imap = lambda v: (ctypes.c_int32 * len(v))(*v)
        before = [sp.info()[k] for k in ("equalizer", "equalizer_filters", "equalizer_fade", "equalizer_pending")]
        assert before[2:] == [T - 200, 1]
        assert fn(None, arr(handles), 3, None) == 1
        assert fn(sp._h, arr(handles), -1, None) == 1
        assert fn(sp._h, None, 2, None) == 1
        assert fn(sp._h, arr([handles[0], None]), 2, None) == 1
        for bad in ([0, 1, 2, 3, 0], [0, 1, -3, 0, 0]):
            assert fn(sp._h, arr(handles), 3, imap(bad)) == 1
        assert fn(sp._h, None, 0, imap([-1, KEEP, 0, -1, KEEP])) == 1                    # definition 0 of none
        assert fn(sp._h, None, 0, None) == 1
        assert fn(sp._h, arr([handles[0], bad_filter]), 2, None) == 16                   # AW_ERR_EQ_INVALID_FILTER
        assert b"(definition 1)" in lib.aw_last_error_message()
        assert fn(sp._h, arr([too_many]), 1, None) == 15                                 # AW_ERR_EQ_TOO_MANY_FILTERS
        assert fn(sp._h, arr([handles[0], handles[1], huge]), 3, None) == 14             # AW_ERR_EQ_NON_FINITE_PREAMP
        with pytest.raises(ValueError):
            sp.set_equalizer_target([adef(aw, A)], [0, 0])                                # one entry per stream
        assert [sp.info()[k] for k in ("equalizer", "equalizer_filters", "equalizer_fade", "equalizer_pending")] == before
        assert np.array_equal(bits(device_call(torch, sp, x)), bits(device_call(torch, twin, x)))
        # no definitions at all is fine when nobody needs one
        assert fn(sp._h, None, 0, imap([-1, KEEP, -1, -1, KEEP])) == 0
        assert sp.info()["equalizer_pending"] == 1
    finally:
        for h in handles + [bad_filter, too_many, huge]:
            lib.aw_eq_definition_destroy(h)


# ---- 8. mixed-rate batches -------------------------------------------------------------------------------------------------------------

def test_mixed_rate_batch_retargets_each_bucket_at_its_own_rate(oracle):
    import airwave_amd as aw
    rates = [48000.0, 44100.0, 48000.0, 44100.0]
    da, db = adef(aw, A), adef(aw, B)
    h7 = oracle.synth_hrir(7, TAPS, seed=62)
    layout = aw.InputLayout.detect(2)
    batch, plain = aw.MixedRateBatch(h7, 48000.0, layout, rates), aw.MixedRateBatch(h7, 48000.0, layout, rates)
    with pytest.raises(ValueError):
        batch.retarget_equalizers([da])
    to = [da, db, None, aw.MixedRateBatch.KEEP]
    batch.retarget_equalizers(to)
    assert [batch.buckets[r].spatializer.info()["equalizer_pending"] for r in (48000.0, 44100.0)] == [1, 1]
    F = {48000.0: 500, 44100.0: 500}
    rng = np.random.default_rng(101)
    first = [rng.uniform(-LEVEL, LEVEL, (F[r], 2)).astype(np.float32) for r in rates]
    second = [rng.uniform(-LEVEL, LEVEL, (2000, 2)).astype(np.float32) for r in rates]
    procs = [None if d == aw.MixedRateBatch.KEEP else aw.ParametricEqualizerProcessor(r, 0, n_streams=1) for r, d in zip(rates, to)]
    for p, d in zip(procs, to):
        if p is not None:
            p.setTarget(d)
    for k, streams in enumerate((first, second)):
        got, ys = batch.process(streams, rates), plain.process(streams, rates)
        if k == 0:                                                   # each bucket on its own clock
            assert [batch.buckets[r].spatializer.info()["equalizer_fade"] for r in (48000.0, 44100.0)] == [960 - 500, 882 - 500]
        for i, p in enumerate(procs):
            want = ys[i] if p is None else p.process_batch(ys[i][None])[0]
            if p is not None:
                p.drainRetiredStates()
            assert np.array_equal(bits(got[i]), bits(want)), (k, i)
    assert [batch.buckets[r].spatializer.info()["equalizer_fade"] for r in (48000.0, 44100.0)] == [0, 0]
