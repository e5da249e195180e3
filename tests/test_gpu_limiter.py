"""The look-ahead true-peak limiter of the batch entries on the MI355X (aw_spatializer_set_limiter / _get_limiter).  The reference is
the header's sequential rule compiled by g++ (tests/emu/emu_limiter.cpp) over the float32 output y that the same handle wrote in an
unlimited twin run of the same calls: the device must equal it bit for bit in z and in the records.  Chunking, sample formats, sharding,
the page-locked single-stream path and splitting calls in time must change no bit; the convolution kernels themselves may round
differently when a call is cut (tests/test_gpu_true_peak.py), so a cut run is held to the rule over the y IT wrote, and to the uncut
run wherever the two y are the same bits."""
import ctypes
import os
import sys

import numpy as np
import pytest

from test_gpu_loudness import delta_spatializer, device_call, host_call, real_spatializer
from test_gpu_pcm_dither import F32, S16, TPDF, context, encode_dithered

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_limiter as emu  # noqa: E402

pytestmark = pytest.mark.gpu

C, L, H = 0.5, 64, 128
D = L + 11
SEED = 77


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rule(y_calls, gains, attack=L, hold=H, c=C):
    """The sequential rule over the calls [S][F][2] of a run: (z [S][sum F][2], records)."""
    lim = emu.Limiter(y_calls[0].shape[0], attack, hold, c, gains)
    z = np.concatenate([lim.process(y) for y in y_calls], axis=1)
    return z, lim


def check_records(rec, lim, frames, what):
    assert np.array_equal(rec["min_gain"].view(np.uint32), lim.min_gain), what
    assert np.array_equal(rec["limited_frames"], lim.limited) and np.array_equal(rec["nonfinite"], lim.nonfinite), what
    assert np.all(rec["frames"] == frames) and not rec["reserved"].any(), what


def gains_to_twice_the_ceiling(y):
    """One fixed gain per stream that brings the stream's sample peak to about 2 c."""
    return (2.0 * C / np.abs(y).max(axis=(1, 2))).astype(np.float32)


def twin_runs(sp, run, calls_x, gains_from=None):
    """The calls with the limiter off (y), a reset, the calls with it on behind fixed gains (z).  Returns (y calls, z calls, gains)."""
    ys = [run(sp, x) for x in calls_x]
    g = gains_to_twice_the_ceiling(np.concatenate(ys, axis=1)) if gains_from is None else gains_from
    sp.reset()
    sp.set_gain("fixed", g)
    sp.set_limiter(True, C, L, H)
    zs = [run(sp, x) for x in calls_x]
    return ys, zs, g


# ---- 1. the sequential rule ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["delta", "real"])
def test_device_equals_the_sequential_rule_bit_for_bit(kind, oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, F = 3, 4099
    rng = np.random.default_rng(71)
    if kind == "delta":
        sp, x = delta_spatializer(aw, ctx, 48000, S), rng.uniform(-0.9, 0.9, (S, F, 2)).astype(np.float32)
    else:
        sp, x = real_spatializer(aw, ctx, oracle, S), rng.uniform(-0.5, 0.5, (S, F, 7)).astype(np.float32)
    sp.set_metering(True)
    ys, zs, g = twin_runs(sp, lambda h, xs: device_call(torch, h, xs), [x])
    assert sp.info()["limiter"] == 1 and sp.info()["limiter_latency"] == D
    want, lim = rule(ys, g)
    rec = sp.limiter()
    print(f"{kind}: gains {g}, min gain {rec['min_gain']}, limited frames {rec['limited_frames']}, peak of z {np.abs(zs[0]).max(axis=(1, 2))}")
    assert np.array_equal(bits(zs[0]), bits(want))
    check_records(rec, lim, F, kind)
    assert np.all(rec["min_gain"] < 0.75) and np.all(rec["limited_frames"] > F // 2)
    assert np.abs(zs[0].astype(np.float64)).max() <= C * (1 + 2.0 ** -23)
    lv = sp.levels()
    assert np.array_equal(bits(lv["gain"]), bits(g))                    # the fixed gain, as without the limiter
    assert np.all(lv["frames"] == F) and np.array_equal(lv["peak"], np.abs(ys[0]).max(axis=1))          # the meter still taps y


# ---- 2. invariances --------------------------------------------------------------------------------------------------------------------

def test_chunking_formats_and_sharding_change_no_bit(oracle):
    import torch
    import airwave_amd as aw
    S, F = 5, 16411                                                   # (enough input bytes for AW_HOST_CHUNK_MB=1 to chunk 5 streams)
    x = np.random.default_rng(72).uniform(-0.5, 0.5, (S, F, 7)).astype(np.float32)
    x[2] *= np.float32(0.01)                                          # one stream stays under the ceiling
    ctx, small = context(aw, torch, chunk_mb=64), context(aw, torch, chunk_mb=1)
    y = device_call(torch, real_spatializer(aw, ctx, oracle, S), x)
    g = gains_to_twice_the_ceiling(y)
    g[2] = 1.0

    def limited(c, streams, first, run):
        sp = real_spatializer(aw, c, oracle, streams)
        sp.set_gain("fixed", g[first:first + streams])
        sp.set_dither("tpdf", SEED, first)
        sp.set_limiter(True, C, L, H)
        out = run(sp, x[first:first + streams])
        return out, sp.limiter(), sp

    z, one, _ = limited(ctx, S, 0, lambda sp, xs: device_call(torch, sp, xs))
    want, lim = rule([y], g)
    assert np.array_equal(bits(z), bits(want))
    check_records(one, lim, F, "device entry")
    assert one["min_gain"][2] == 1.0 and one["limited_frames"][2] == 0 and np.all(one["min_gain"][[0, 1, 3, 4]] < 0.75)
    zc, chunked, sp_c = limited(small, S, 0, lambda sp, xs: host_call(sp, xs))
    assert 0 < sp_c.info()["host_chunk_streams"] < S
    assert zc.tobytes() == z.tobytes() and chunked.tobytes() == one.tobytes()
    z16 = encode_dithered(S16, TPDF, z, SEED)[0]
    for run in (lambda sp, xs: host_call(sp, xs, S16), lambda sp, xs: device_call(torch, sp, xs, S16)):
        for c in (ctx, small):
            out, rec, _ = limited(c, S, 0, run)
            assert np.array_equal(out, z16) and rec.tobytes() == one.tobytes()
    shards = [limited(ctx, k, first, lambda sp, xs: device_call(torch, sp, xs)) for first, k in ((0, 2), (2, 3))]
    assert np.concatenate([s[0] for s in shards]).tobytes() == z.tobytes()
    assert np.concatenate([s[1] for s in shards]).tobytes() == one.tobytes()
    shards16 = [limited(small, k, first, lambda sp, xs: host_call(sp, xs, S16))[0] for first, k in ((0, 2), (2, 3))]
    assert np.array_equal(np.concatenate(shards16), z16)


# ---- 3. the single-stream page-locked path -----------------------------------------------------------------------------------------------

def test_single_stream_callback_path_equals_the_stream_inside_a_batch():
    """One stream, callback-sized calls of the host entry: the CPU runs the rule itself over the page-locked output."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    calls = [4096, 3, D + 1]
    x = np.random.default_rng(73).uniform(-0.9, 0.9, (3, sum(calls), 2)).astype(np.float32)
    at = np.concatenate([[0], np.cumsum(calls)])
    g = np.array([1.3, 1.1, 0.9], np.float32)
    for fout in (F32, S16):
        got = {}
        for name, streams, first in (("callback", 1, 1), ("batch", 3, 0)):
            sp = delta_spatializer(aw, ctx, 44100, streams)
            if name == "callback":
                sp.reserve_host(4096)
            xs = [x[first:first + streams, a:b] for a, b in zip(at[:-1], at[1:])]
            ys = [host_call(sp, c) for c in xs]
            sp.reset()
            sp.set_gain("fixed", g[first:first + streams])
            sp.set_dither("tpdf", SEED, first)
            sp.set_metering(True)
            sp.set_limiter(True, C, L, H)
            zs = np.concatenate([host_call(sp, c, fout) for c in xs], axis=1)
            want, lim = rule(ys, g[first:first + streams])
            if fout == F32:
                assert np.array_equal(bits(zs), bits(want)), name
            else:
                assert np.array_equal(zs, encode_dithered(S16, TPDF, want, SEED, first)[0]), name
            check_records(sp.limiter(), lim, sum(calls), name)
            got[name] = (np.concatenate(ys, axis=1), zs, sp.limiter(), sp.levels())
            if name == "callback":
                assert sp.info()["host_chunk_streams"] == 0
        if np.array_equal(bits(got["callback"][0]), bits(got["batch"][0][1:2])):
            assert got["callback"][1].tobytes() == got["batch"][1][1:2].tobytes()
            assert got["callback"][2].tobytes() == got["batch"][2][1:2].tobytes()
            assert got["callback"][3]["clipped"][0] == got["batch"][3]["clipped"][1]


# ---- 4. cutting in time ----------------------------------------------------------------------------------------------------------------

def test_cutting_calls_in_time_changes_no_bit(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, F = 3, 4099
    x = np.random.default_rng(74).uniform(-0.5, 0.5, (S, F, 7)).astype(np.float32)
    runs = {}
    g = None
    for cuts in ((F,), (1000, F - 1000), (D - 1, F - (D - 1))):
        sp = real_spatializer(aw, ctx, oracle, S)
        at = np.concatenate([[0], np.cumsum(cuts)])
        ys, zs, g = twin_runs(sp, lambda h, xs: device_call(torch, h, xs), [x[:, a:b] for a, b in zip(at[:-1], at[1:])], g)
        want, lim = rule(ys, g)
        z = np.concatenate(zs, axis=1)
        assert np.array_equal(bits(z), bits(want)), cuts
        check_records(sp.limiter(), lim, F, cuts)
        runs[cuts] = (np.concatenate(ys, axis=1), z, sp.limiter())
    whole = runs[(F,)]
    for cuts, (y, z, rec) in runs.items():
        same = np.array_equal(bits(y), bits(whole[0]))
        print(f"calls of {cuts}: y identical to the uncut run's: {same}")
        if same:
            assert z.tobytes() == whole[1].tobytes() and rec.tobytes() == whole[2].tobytes()
    # through a unit impulse the outputs do not depend on the cut on any kernel path that reproduces its input exactly: checked, then held
    xd = np.random.default_rng(75).uniform(-0.9, 0.9, (S, F, 2)).astype(np.float32)
    gd = np.array([1.2, 1.0, 0.7], np.float32)
    outs = []
    for cuts in ((F,), (1000, F - 1000), (D - 1, F - (D - 1))):
        sp = delta_spatializer(aw, ctx, 48000, S)
        at = np.concatenate([[0], np.cumsum(cuts)])
        ys, zs, _ = twin_runs(sp, lambda h, xs: host_call(h, xs), [xd[:, a:b] for a, b in zip(at[:-1], at[1:])], gd)
        outs.append((np.concatenate(ys, axis=1), np.concatenate(zs, axis=1), sp.limiter()))
        assert np.array_equal(bits(outs[-1][1]), bits(rule(ys, gd)[0])), cuts
    for y, z, rec in outs[1:]:
        if np.array_equal(bits(y), bits(outs[0][0])):
            assert z.tobytes() == outs[0][1].tobytes() and rec.tobytes() == outs[0][2].tobytes()


# ---- 5. default behaviour, the setter's rules -------------------------------------------------------------------------------------------

def test_off_means_off_and_the_refusals(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    x = np.random.default_rng(76).uniform(-0.5, 0.5, (3, 5003, 7)).astype(np.float32)
    for fout in (F32, S16):
        plain, switched = real_spatializer(aw, ctx, oracle, 3), real_spatializer(aw, ctx, oracle, 3)
        switched.set_limiter(True, C, L, H)
        switched.set_limiter(False)
        assert switched.info()["limiter"] == 0 and switched.info()["limiter_latency"] == 0
        for sp in (plain, switched):
            sp.set_gain("fixed", [0.5])
            sp.set_profiling(True)
        for run in (lambda sp: device_call(torch, sp, x, fout), lambda sp: host_call(sp, x, fout)):
            assert run(plain).tobytes() == run(switched).tobytes()
        ctx.synchronize()
        assert [n for n, _, _ in plain.stage_times()] == [n for n, _, _ in switched.stage_times()]
        assert "aw_limiter_kernel" not in [n for n, _, _ in switched.stage_times()]
        assert not switched.limiter()["frames"].any() and np.all(switched.limiter()["min_gain"] == 1.0)
        # on: the kernel runs, the scale kernel does not, and a reserved process path does not allocate
        switched.set_limiter(True, C, L, H)
        switched.reserve_pcm(5003, "f32", "s16")
        switched.set_profiling(True)
        device_call(torch, switched, x, fout)
        host_call(switched, x, fout)
        allocs = switched.info()["device_allocs"]
        device_call(torch, switched, x, fout)
        host_call(switched, x, fout)
        ctx.synchronize()
        assert switched.info()["device_allocs"] == allocs
        names = [n for n, _, _ in switched.stage_times()]
        assert "aw_limiter_kernel" in names and "aw_scale_kernel" not in names
    sp = delta_spatializer(aw, ctx, 48000, 2)
    with pytest.raises(aw.AirwaveError):
        sp.limiter()                                                  # never switched on
    lib, f = sp._lib, ctypes.c_float
    assert lib.aw_spatializer_set_limiter(None, 1, f(C), L, H) == 1
    sp.set_limiter(True, 0.25, 32, 7)
    for bad in ((0.0, L, H), (-0.5, L, H), (1.5, L, H), (float("nan"), L, H), (float("inf"), L, H), (C, 15, H), (C, 513, H), (C, L, -1), (C, L, 1025)):
        assert lib.aw_spatializer_set_limiter(sp._h, 1, f(bad[0]), bad[1], bad[2]) == 1
        assert sp.info()["limiter"] == 1 and sp.info()["limiter_latency"] == 32 + 11
    for mode in ("peak_ceiling", "true_peak_ceiling"):
        with pytest.raises(aw.AirwaveError):
            sp.set_gain(mode, ceiling=0.5)                            # per-call gains would break "splitting calls changes no bit"
        assert sp.info()["gain_mode"] == 0
    sp.set_limiter(False)
    for mode in ("peak_ceiling", "true_peak_ceiling"):
        sp.set_gain(mode, ceiling=0.5)
        assert lib.aw_spatializer_set_limiter(sp._h, 1, f(C), L, H) == 1 and sp.info()["limiter"] == 0
    sp.set_gain("none")
    # the previous setting is what runs: L = 32, H = 7, c = 0.25.  y1 / y2: what the convolution writes from silence and behind `a` (a
    # twin handle without limiter; a unit impulse through the FFT is exact only up to rounding)
    a = np.random.default_rng(78).uniform(-0.9, 0.9, (2, 700, 2)).astype(np.float32)
    twin = delta_spatializer(aw, ctx, 48000, 2)
    (want1, lim1), (want2, lim2) = (rule([host_call(twin, a)], None, 32, 7, 0.25) for _ in range(2))

    def zeroed():
        r = sp.limiter()
        return not r["frames"].any() and not r["limited_frames"].any() and not r["nonfinite"].any() and np.all(r["min_gain"] == 1.0)

    sp.set_limiter(True, 0.25, 32, 7)
    assert zeroed()
    assert np.array_equal(bits(host_call(sp, a)), bits(want1))
    check_records(sp.limiter(), lim1, 700, "the first call")
    sp.reset_levels()                                                 # records and the limiter's history; the convolution's history stays
    assert zeroed()
    assert np.array_equal(bits(host_call(sp, a)), bits(want2))
    check_records(sp.limiter(), lim2, 700, "after reset_levels")
    sp.reset()
    assert zeroed()
    assert np.array_equal(bits(host_call(sp, a)), bits(want1))
    sp.set_limiter(False)                                             # off -> on: empty history again, the records stay
    sp.set_limiter(True, 0.25, 32, 7)
    assert np.array_equal(bits(host_call(sp, a)), bits(want2))
    r = sp.limiter()
    assert np.all(r["frames"] == 1400) and np.array_equal(r["limited_frames"], lim1.limited + lim2.limited)
    assert np.array_equal(r["min_gain"].view(np.uint32), np.minimum(lim1.min_gain, lim2.min_gain))


# ---- 6. another attack on a live handle ---------------------------------------------------------------------------------------------------

def test_another_attack_on_a_live_handle_makes_new_records(oracle):
    """aw_spatializer_set_limiter with another attack and hold on a handle whose limiter has run: new records and history are made first,
    then the stream goes idle and the old ones are freed; the records start over and the history is silence."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    h = oracle.synth_hrir(2, 64, seed=79)
    lt, rt = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    sp, twin = (aw.Spatializer(aw.HRIR(h, sample_rate=48000.0, ctx=ctx), lt, rt, n_streams=2, ctx=ctx) for _ in range(2))
    x = np.random.default_rng(79).uniform(-0.9, 0.9, (2, 4000, 2)).astype(np.float32)
    y1, y2 = host_call(twin, x[:, :1000]), host_call(twin, x[:, 1000:])          # what the convolution writes, call by call
    y = np.concatenate([y1, y2], axis=1)
    for s in range(2):
        assert oracle.peak_rel_error(y[s], oracle.spatialize_f64(x[s], h, lt, rt)) < 1e-5
    allocs = sp.info()["device_allocs"]
    sp.set_limiter(True, C, 32, 7)
    z1 = host_call(sp, x[:, :1000])
    want1, lim1 = rule([y1], None, 32, 7)
    assert np.array_equal(bits(z1), bits(want1))
    check_records(sp.limiter(), lim1, 1000, "attack 32, hold 7")
    assert np.all(lim1.limited > 0)
    sp.set_limiter(True, C, L, H)
    assert sp.info()["limiter"] == 1 and sp.info()["limiter_latency"] == D
    r = sp.limiter()
    assert not r["frames"].any() and not r["limited_frames"].any() and np.all(r["min_gain"] == 1.0)
    z2 = host_call(sp, x[:, 1000:])
    want2, lim2 = rule([y2], None)                                    # (behind silence: the history started over with the records)
    assert np.array_equal(bits(z2), bits(want2))
    check_records(sp.limiter(), lim2, 3000, "attack 64, hold 128")
    assert np.all(lim2.limited > 0)
    delta = sp.info()["device_allocs"] - allocs
    print(f"device allocations of the sequence: {delta}")
    # Measured once on the library as it was before the buffers got an owning type (not derived from the new code): the records twice,
    # and for 1000 frames and again for 3000 the float staging in and out and the staging in front of the limiter.
    assert delta == 8
