"""Per-stream levels and gain of the batch entries on the MI355X (aw_spatializer_set_metering / _get_levels / _set_gain).  The float
entry's output y on an identical handle that never touched the new entries is the truth: the records must be numpy's peak, count and
(within the summation bound) energy of y, the per-stream clip counts numpy's, every gained output numpy's encode of float32(y * g) bit for
bit, and chunking, pinning, alignment, sharding and (NONE / FIXED) splitting in time invisible.  With meter and gain off a handle launches
what it always has."""
import ctypes

import numpy as np
import pytest

from test_gpu_pcm_dither import (F32, MODE, NAME, NONE, S16, S24, S32, TPDF, TPDF_HP, U64, context, from_dev, layout, np_dither, out_host,
                                 pack_s24, to_dev)

pytestmark = pytest.mark.gpu

TAPS = 4320
ENTRIES = ("process", "process_pcm", "process_host", "process_host_pcm")


# ---- numpy restatement of the documented rules -------------------------------------------------------------------------------------------

def np_levels(y):
    """peak [S, 2] float32, energy [S, 2] float64, nonfinite [S] of y [S, F, 2]."""
    fin = np.isfinite(y)
    z = np.where(fin, y, np.float32(0))
    return np.abs(z).max(axis=1), (z.astype(np.float64) ** 2).sum(axis=1), (~fin).sum(axis=(1, 2))


def np_auto_gain(y, c):
    p = np_levels(y)[0].max(axis=1)
    c = np.float32(c)
    with np.errstate(divide="ignore"):
        return np.where(p > c, c / p, np.float32(1)).astype(np.float32)


def np_encode(fmt, mode, x, seed=0, first_stream=0, pos0=0):
    """The documented encode of float32 x [S, F, 2] -> (array in fmt's host layout, clipped mask [S, F, 2])."""
    if fmt == F32:
        return x.copy(), np.zeros(x.shape, bool)
    S, F, _ = x.shape
    with np.errstate(over="ignore", invalid="ignore"):
        if fmt == S32:
            v, lo, hi = np.rint(x.astype(np.float64) * 2147483648.0), -2.0 ** 31, 2.0 ** 31 - 1
        else:
            scale = np.float32(32768 if fmt == S16 else 8388608)
            d = np.float32(0)
            if mode != NONE:
                g = (U64(first_stream) + np.arange(S, dtype=U64))[:, None, None]
                p = (U64(pos0) + np.arange(F, dtype=U64))[None, :, None]
                d = np_dither(mode, seed, g, p, np.arange(2, dtype=U64)[None, None, :])
            v = np.rint(x * scale + d).astype(np.float64)
            lo, hi = (-32768.0, 32767.0) if fmt == S16 else (-8388608.0, 8388607.0)
        clipped = ~((v >= lo) & (v <= hi))
        r = np.where(np.isnan(v), 0.0, np.clip(v, lo, hi)).astype(np.int64)
    return {S16: lambda: r.astype(np.int16), S24: lambda: pack_s24(r), S32: lambda: r.astype(np.int32)}[fmt](), clipped


def expected(y, splits, fout, dither=NONE, seed=0, first_stream=0, gain="none", gains=None, ceiling=None):
    """What a metered handle must report and write for truth y [S, sum(splits), 2] over consecutive calls of `splits` frames:
    (output, peak, energy, nonfinite, clipped per stream, gain per stream of the last call)."""
    S = y.shape[0]
    outs, clipped, at = [], np.zeros(S, np.int64), 0
    g = np.ones(S, np.float32)
    for n in splits:
        ys = y[:, at:at + n]
        if gain == "fixed":
            g = np.broadcast_to(np.asarray(gains, np.float32), (S,))
        elif gain == "peak_ceiling":
            g = np_auto_gain(ys, ceiling)
        with np.errstate(invalid="ignore", over="ignore"):
            yg = (ys * g[:, None, None]).astype(np.float32) if gain != "none" else ys
        o, cm = np_encode(fout, dither, yg, seed, first_stream, at)
        outs.append(o)
        clipped += cm.sum(axis=(1, 2))
        at += n
    peak, energy, nonfinite = np_levels(y)
    return np.concatenate(outs, axis=1), peak, energy, nonfinite, clipped, g


def check_levels(lv, want, frames, what=""):
    _, peak, energy, nonfinite, clipped, g = want
    assert np.array_equal(lv["peak"].view(np.uint32), peak.view(np.uint32)), what
    assert np.array_equal(lv["frames"], np.full(len(lv), frames, np.uint64)), what
    assert np.array_equal(lv["nonfinite"].astype(np.int64), nonfinite), what
    assert np.array_equal(lv["clipped"].astype(np.int64), clipped), (what, lv["clipped"], clipped)
    assert np.array_equal(lv["gain"].view(np.uint32), g.view(np.uint32)), (what, lv["gain"], g)
    assert not lv["reserved"].any()
    # N non-negative exact terms summed in any order: relative error at most N * 2^-53 (N: samples per ear)
    bound = frames * 2.0 ** -53 * energy
    err = np.abs(lv["energy"] - energy)
    print(f"{what}: max energy error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert np.all(err <= bound), (what, err, bound)


# ---- running the entries -----------------------------------------------------------------------------------------------------------------

def make_sp(aw, ctx, h, channels, S, dither=NONE, seed=0, first_stream=0):
    lt, rt = layout(channels)
    sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    if dither != NONE:
        sp.set_dither(MODE[dither], seed=seed, first_stream=first_stream)
    return sp


def run(torch, ctx, sp, entry, x, fout, splits, pinned=False, misalign=0):
    """x float32 [S, F, C] through consecutive calls of one entry -> (output in fout's layout, summed clipped count or None)."""
    S = x.shape[0]
    outs, at, clips = [], 0, 0
    clip_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    for n in splits:
        xs = np.ascontiguousarray(x[:, at:at + n])
        yo = out_host(fout, S, n)
        if entry in ("process", "process_pcm"):
            xd = torch.empty(xs.nbytes + 64, dtype=torch.uint8, device="cuda")
            yd = torch.empty(yo.nbytes + 64, dtype=torch.uint8, device="cuda")
            assert not (misalign and fout == F32)                    # float32 buffers go to the kernels as they are: aligned
            ox, oy = 0, misalign * {S16: 2, S24: 1, S32: 4}.get(fout, 0)   # an integer output at an odd 16-byte offset
            xd[ox:ox + xs.nbytes] = to_dev(torch, xs)
            if entry == "process":
                assert fout == F32
                sp.process_device(xd.data_ptr() + ox, yd.data_ptr() + oy, n)
            else:
                sp.process_pcm_device(xd.data_ptr() + ox, "f32", yd.data_ptr() + oy, NAME[fout], n, clip_t.data_ptr())
            torch.cuda.synchronize()
            outs.append(from_dev(yd[oy:oy + yo.nbytes], yo))
        else:
            if pinned:
                xh, yh = ctx.pinned_empty(xs.shape, xs.dtype), ctx.pinned_empty(yo.shape, yo.dtype)
                xh[...] = xs
            else:
                xh, yh = xs, yo
            if entry == "process_host":
                assert fout == F32
                sp.process_host_into(xh, yh)
            else:
                clips += sp.process_host_into(xh, yh, out_format=NAME[fout])
            outs.append(np.array(yh))
        at += n
    if entry == "process_pcm":
        clips = int(clip_t.item())
    return np.concatenate(outs, axis=1), clips


def truth(aw, torch, ctx, h, channels, x, splits):
    """The float entry's output on a handle that never touched the new entries."""
    sp = make_sp(aw, ctx, h, channels, x.shape[0])
    return run(torch, ctx, sp, "process", x, F32, splits)[0]


def loud_input(rng, S, F, C, lo=0.02, hi=1.5):
    """Ordinary noise whose level rises from stream to stream, so that some streams' output clips and some stays far below full scale."""
    x = rng.standard_normal((S, F, C)).astype(np.float32)
    return x * np.geomspace(lo, hi, S).astype(np.float32)[:, None, None]


@pytest.fixture(scope="module")
def hrir(oracle):
    return oracle.synth_hrir(14, TAPS, seed=41)


# ---- 1: levels against numpy -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels,S,splits", [(2, 5, (1001, 777)), (8, 7, (2003, 1)), (14, 3, (999, 1502)), (8, 6, (3, 5, 7))])
def test_levels_equal_numpy_on_every_entry(hrir, channels, S, splits):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    rng = np.random.default_rng(channels * 100 + S)
    x = loud_input(rng, S, sum(splits), channels)
    y = truth(aw, torch, ctx, hrir, channels, x, splits)
    for entry in ENTRIES:
        fout = S16 if entry.endswith("pcm") else F32
        sp = make_sp(aw, ctx, hrir, channels, S)
        sp.set_metering(True)
        assert sp.info()["metering"] == 1 and sp.info()["gain_mode"] == 0
        got, clips = run(torch, ctx, sp, entry, x, fout, splits)
        want = expected(y, splits, fout)
        assert np.array_equal(got.view(np.uint8), want[0].view(np.uint8)), entry
        lv = sp.levels()
        check_levels(lv, want, sum(splits), f"{entry} C={channels} splits={splits}")
        if fout != F32:
            assert clips == int(want[4].sum())
        sp.reset_levels()
        assert not sp.levels()["frames"].any() and not sp.levels()["peak"].any()


def test_single_stream_page_locked_path(hrir):
    """One stream, reserved: the host entries take the page-locked path, whose levels and gain are computed on the CPU by the same rules."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    rng = np.random.default_rng(5)
    splits = (1000, 333)
    x = (rng.standard_normal((1, sum(splits), 8)) * 0.9).astype(np.float32)
    y = truth(aw, torch, ctx, hrir, 8, x, splits)
    for entry, fout in (("process_host", F32), ("process_host_pcm", S16), ("process_host_pcm", S24)):
        for gain, kw in (("none", {}), ("fixed", {"gains": [0.25]}), ("peak_ceiling", {"ceiling": 0.5})):
            sp = make_sp(aw, ctx, hrir, 8, 1, TPDF, seed=3)
            sp.reserve(max(splits))
            sp.set_metering(True)
            sp.set_gain(gain, **kw)
            got, clips = run(torch, ctx, sp, entry, x, fout, splits)
            want = expected(y, splits, fout, TPDF, 3, 0, gain, **kw)
            assert np.array_equal(got.view(np.uint8), want[0].view(np.uint8)), (entry, NAME[fout], gain)
            check_levels(sp.levels(), want, sum(splits), f"one stream {entry} {NAME[fout]} {gain}")


# ---- 2: per-stream clipped ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dither", [NONE, TPDF, TPDF_HP])
def test_clipped_per_stream(hrir, dither):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, splits = 9, (1501, 6)
    x = loud_input(np.random.default_rng(11), S, sum(splits), 8)
    y = truth(aw, torch, ctx, hrir, 8, x, splits)
    for fout in (S16, S24, S32):
        for entry in ("process_pcm", "process_host_pcm"):
            sp = make_sp(aw, ctx, hrir, 8, S, dither, seed=21, first_stream=40)
            sp.set_metering(True)
            got, clips = run(torch, ctx, sp, entry, x, fout, splits)
            want = expected(y, splits, fout, dither, 21, 40)
            assert 0 < np.count_nonzero(want[4]) < S                  # some streams clip, not all
            assert np.array_equal(got.view(np.uint8), want[0].view(np.uint8))
            lv = sp.levels()
            check_levels(lv, want, sum(splits), f"clipped {entry} {NAME[fout]} {MODE[dither]}")
            assert int(lv["clipped"].sum()) == clips == int(want[4].sum())


# ---- 3: fixed gains -----------------------------------------------------------------------------------------------------------------------

def test_fixed_gains(hrir):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, splits = 6, (1203, 502)
    rng = np.random.default_rng(12)
    x = loud_input(rng, S, sum(splits), 8)
    y = truth(aw, torch, ctx, hrir, 8, x, splits)
    gains = rng.uniform(0.05, 1.7, S).astype(np.float32)
    gains[2] = -0.5
    for g in (gains, gains[:1]):
        for entry, fout, dither in (("process", F32, NONE), ("process_host", F32, NONE), ("process_pcm", S16, TPDF), ("process_pcm", S24, TPDF_HP),
                                    ("process_pcm", S32, NONE), ("process_host_pcm", S16, NONE), ("process_host_pcm", S24, TPDF)):
            sp = make_sp(aw, ctx, hrir, 8, S, dither, seed=8)
            sp.set_metering(True)
            sp.set_gain("fixed", gains=g)
            assert sp.info()["gain_mode"] == 1
            got, clips = run(torch, ctx, sp, entry, x, fout, splits)
            want = expected(y, splits, fout, dither, 8, 0, "fixed", gains=g)
            assert np.array_equal(got.view(np.uint8), want[0].view(np.uint8)), (entry, NAME[fout], g.size)
            check_levels(sp.levels(), want, sum(splits), f"fixed {entry} {NAME[fout]} n={g.size}")
    # without the meter the gain still applies, and the records stay empty
    sp = make_sp(aw, ctx, hrir, 8, S)
    sp.set_gain("fixed", gains=gains)
    got, _ = run(torch, ctx, sp, "process_pcm", x, S16, splits)
    assert np.array_equal(got, expected(y, splits, S16, gain="fixed", gains=gains)[0])
    lv = sp.levels()
    assert not lv["frames"].any() and not lv["clipped"].any() and np.array_equal(lv["gain"], gains)


# ---- 4: peak ceiling ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["process_pcm", "process_host_pcm"])
def test_peak_ceiling_stops_the_clipping(hrir, entry):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, splits, c = 10, (2501,), 0.98
    x = loud_input(np.random.default_rng(13), S, sum(splits), 14)
    y = truth(aw, torch, ctx, hrir, 14, x, splits)
    plain_sp = make_sp(aw, ctx, hrir, 14, S)
    plain, plain_clips = run(torch, ctx, plain_sp, entry, x, S16, splits)
    assert plain_clips > 0
    sp = make_sp(aw, ctx, hrir, 14, S)
    sp.set_metering(True)
    sp.set_gain("peak_ceiling", ceiling=c)
    assert sp.info()["gain_mode"] == 2
    got, clips = run(torch, ctx, sp, entry, x, S16, splits)
    assert clips == 0
    want = expected(y, splits, S16, gain="peak_ceiling", ceiling=c)
    lv = sp.levels()
    check_levels(lv, want, sum(splits), f"peak ceiling {entry}")
    assert np.array_equal(lv["gain"].view(np.uint32), np_auto_gain(y, c).view(np.uint32))
    assert np.array_equal(got, want[0])
    quiet = lv["gain"] == 1
    assert quiet.any() and not quiet.all()
    assert np.array_equal(got[quiet], plain[quiet])                   # streams under the ceiling: a gain of 1 and today's bytes
    # float32 output and the other formats under the same rule, dither included
    for entry2, fout, dither in (("process", F32, NONE), ("process_host", F32, NONE), (entry, S24, TPDF), (entry, S32, NONE), (entry, S16, TPDF_HP)):
        sp = make_sp(aw, ctx, hrir, 14, S, dither, seed=4)
        sp.set_gain("peak_ceiling", ceiling=c)
        got, _ = run(torch, ctx, sp, entry2, x, fout, splits)
        want = expected(y, splits, fout, dither, 4, 0, "peak_ceiling", ceiling=c)
        assert np.array_equal(got.view(np.uint8), want[0].view(np.uint8)), (entry2, NAME[fout])


# ---- 5: invariance ------------------------------------------------------------------------------------------------------------------------

GAINS = [("none", {}), ("fixed", {"gains": None}), ("peak_ceiling", {"ceiling": 0.7})]


@pytest.mark.parametrize("gain,kw", GAINS, ids=[g for g, _ in GAINS])
def test_chunks_pinning_alignment_and_shards_are_invisible(hrir, gain, kw):
    import torch
    import airwave_amd as aw
    S, splits, C = 24, (9001,), 8                                     # 24 x 9001 x 8 floats = 6.9 MB: chunks of 1 MB
    rng = np.random.default_rng(14)
    x = loud_input(rng, S, sum(splits), C)
    if gain == "fixed":
        kw = {"gains": rng.uniform(0.1, 1.2, S).astype(np.float32)}
    big, small = context(aw, torch), context(aw, torch, chunk_mb=1)
    y = truth(aw, torch, big, hrir, C, x, splits)

    def handle(ctx, n=S, first=0, g0=0):
        sp = make_sp(aw, ctx, hrir, C, n, TPDF, seed=6, first_stream=first)
        sp.set_metering(True)
        k = dict(kw)
        if gain == "fixed":
            k["gains"] = kw["gains"][g0:g0 + n]
        sp.set_gain(gain, **k)
        return sp

    for fout in (S16, F32):
        want = expected(y, splits, fout, TPDF, 6, 0, gain, **kw)
        host, dev = ("process_host_pcm", "process_pcm") if fout != F32 else ("process_host", "process")
        variants = {}
        sp = handle(small)
        variants["chunked pageable"] = (run(torch, small, sp, host, x, fout, splits)[0], sp.levels())
        assert sp.info()["host_chunk_streams"] > 0
        sp = handle(small)
        variants["chunked pinned"] = (run(torch, small, sp, host, x, fout, splits, pinned=True)[0], sp.levels())
        sp = handle(big)
        variants["one piece"] = (run(torch, big, sp, host, x, fout, splits)[0], sp.levels())
        assert sp.info()["host_chunk_streams"] == 0
        sp = handle(small)
        variants["device chunked"] = (run(torch, small, sp, dev, x, fout, splits)[0], sp.levels())
        if fout != F32:
            sp = handle(big)
            variants["device unaligned"] = (run(torch, big, sp, dev, x, fout, splits, misalign=3)[0], sp.levels())
        a, b = handle(big, S // 2, 0, 0), handle(big, S - S // 2, S // 2, S // 2)
        ya, yb = run(torch, big, a, dev, x[:S // 2], fout, splits)[0], run(torch, big, b, dev, x[S // 2:], fout, splits)[0]
        variants["two shards"] = (np.concatenate([ya, yb]), np.concatenate([a.levels(), b.levels()]))
        for name, (got, lv) in variants.items():
            assert np.array_equal(got.view(np.uint8), want[0].view(np.uint8)), (name, NAME[fout])
            check_levels(lv, want, sum(splits), f"{gain} {NAME[fout]} {name}")


@pytest.mark.parametrize("gain", ["none", "fixed"])
def test_splitting_calls_in_time_is_invisible(hrir, gain):
    """The kernels' float output is the truth per split; on it, NONE and FIXED give the same records and bytes however the frames are cut."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, C, F = 5, 8, 3000
    rng = np.random.default_rng(15)
    x = loud_input(rng, S, F, C)
    kw = {"gains": rng.uniform(0.1, 1.2, S).astype(np.float32)} if gain == "fixed" else {}
    results = []
    for splits in ((F,), (1700, 1300), (7, 2048, 945)):
        y = truth(aw, torch, ctx, hrir, C, x, splits)
        sp = make_sp(aw, ctx, hrir, C, S, TPDF_HP, seed=2)
        sp.set_metering(True)
        sp.set_gain(gain, **kw)
        got, _ = run(torch, ctx, sp, "process_pcm", x, S16, splits)
        want = expected(y, splits, S16, TPDF_HP, 2, 0, gain, **kw)
        assert np.array_equal(got, want[0]), splits
        check_levels(sp.levels(), want, F, f"time split {splits} {gain}")
        results.append((y, got, sp.levels()))
    for y, got, lv in results[1:]:
        if np.array_equal(y.view(np.uint32), results[0][0].view(np.uint32)):      # where the kernels' float output does not depend on the cut
            assert np.array_equal(got, results[0][1])
            for f in ("peak", "frames", "clipped", "nonfinite", "gain"):
                assert np.array_equal(lv[f], results[0][2][f]), f


# ---- 6: off means today -------------------------------------------------------------------------------------------------------------------

def test_off_is_todays_launch_sequence_and_bytes(hrir):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, splits = 6, (1777,)
    x = loud_input(np.random.default_rng(16), S, sum(splits), 8)

    def profiled(sp, entry, fout):
        sp.set_profiling(True)
        got, clips = run(torch, ctx, sp, entry, x, fout, splits)
        ctx.synchronize()
        return got, clips, [(n, k) for n, _, k in sp.stage_times()]

    for entry, fout in (("process_pcm", S16), ("process_host_pcm", S24), ("process", F32), ("process_host", F32)):
        fresh = profiled(make_sp(aw, ctx, hrir, 8, S, TPDF, seed=1), entry, fout)
        names = [n for n, _ in fresh[2]]
        assert "aw_levels_kernel" not in names and "aw_scale_kernel" not in names
        sp = make_sp(aw, ctx, hrir, 8, S, TPDF, seed=1)
        sp.set_metering(True)
        sp.set_gain("fixed", gains=[0.5])
        on = profiled(sp, entry, fout)
        on_names = [n for n, _ in on[2]]
        assert "aw_levels_kernel" in on_names and ("aw_scale_kernel" in on_names) == (fout == F32), on_names
        assert ("aw_pcm_encode_kernel" in on_names) == (fout != F32)
        sp.set_metering(False)
        sp.set_gain("none")
        sp.reset()
        assert sp.info()["metering"] == 0 and sp.info()["gain_mode"] == 0
        off = profiled(sp, entry, fout)
        assert off[2] == fresh[2], (off[2], fresh[2])
        assert np.array_equal(off[0].view(np.uint8), fresh[0].view(np.uint8)) and off[1] == fresh[1]


# ---- 7: allocation contract ---------------------------------------------------------------------------------------------------------------

def test_metered_gained_calls_allocate_nothing(hrir):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch, chunk_mb=1)
    S, F = 24, 9001
    x = loud_input(np.random.default_rng(17), S, F, 8)
    sp = make_sp(aw, ctx, hrir, 8, S, TPDF)
    before = sp.info()["device_allocs"]
    sp.set_metering(True)
    assert sp.info()["device_allocs"] == before + 1                   # the records, at once
    sp.reserve_pcm(F, "f32", "s16")
    sp.set_gain("peak_ceiling", ceiling=0.9)
    sp.set_gain("fixed", gains=np.full(S, 0.5, np.float32))
    allocs = sp.info()["device_allocs"]
    for gain, kw in (("fixed", {"gains": [0.5]}), ("peak_ceiling", {"ceiling": 0.9}), ("none", {})):
        sp.set_gain(gain, **kw)
        run(torch, ctx, sp, "process_host_pcm", x, S16, (F,))
        run(torch, ctx, sp, "process_pcm", x, S16, (F,))
        sp.levels()
        assert sp.info()["device_allocs"] == allocs, gain


# ---- 8: a non-finite input sample ---------------------------------------------------------------------------------------------------------

def test_nonfinite_sample_stays_in_its_stream(hrir):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    S, splits, bad = 6, (2001,), 3
    x = loud_input(np.random.default_rng(18), S, sum(splits), 8, lo=0.05, hi=0.3)
    xn = x.copy()
    xn[bad, 700, 2] = np.nan
    y, yn = truth(aw, torch, ctx, hrir, 8, x, splits), truth(aw, torch, ctx, hrir, 8, xn, splits)
    assert not np.isfinite(yn[bad]).all() and np.isfinite(np.delete(yn, bad, axis=0)).all()
    for gain, kw in (("none", {}), ("peak_ceiling", {"ceiling": 0.5})):
        res = []
        for xin, yy in ((x, y), (xn, yn)):
            sp = make_sp(aw, ctx, hrir, 8, S, TPDF, seed=9)
            sp.set_metering(True)
            sp.set_gain(gain, **kw)
            got, _ = run(torch, ctx, sp, "process_pcm", xin, S16, splits)
            want = expected(yy, splits, S16, TPDF, 9, 0, gain, **kw)
            assert np.array_equal(got, want[0])
            lv = sp.levels()
            check_levels(lv, want, sum(splits), f"nonfinite {gain}")
            res.append((got, lv))
        assert res[1][1]["nonfinite"][bad] == np.count_nonzero(~np.isfinite(yn[bad])) > 0
        others = np.arange(S) != bad
        assert np.array_equal(res[0][0][others], res[1][0][others])
        for f in ("peak", "gain", "frames", "clipped", "nonfinite"):
            assert np.array_equal(res[0][1][f][others], res[1][1][f][others]), f


def test_get_levels_argument_checks(hrir):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    sp = make_sp(aw, ctx, hrir, 8, 4)
    with pytest.raises(aw.AirwaveError):
        sp.levels()                                                   # neither metering nor a gain was ever set
    sp.set_metering(True)
    assert len(sp.levels(1, 2)) == 2 and len(sp.levels(4, 0)) == 0
    buf = np.zeros(8, aw.LEVELS_DTYPE)
    for first, n in ((-1, 1), (0, 5), (3, 2), (0, -1)):
        assert sp._lib.aw_spatializer_get_levels(sp._h, first, n, buf.ctypes.data) == 1
    sp.set_gain("peak_ceiling", ceiling=0.5)
    g3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    assert sp._lib.aw_spatializer_set_gain(sp._h, 1, g3, 3, 0.0) == 1          # 3 gains for 4 streams: refused, the setting stays
    assert sp.info()["gain_mode"] == 2
