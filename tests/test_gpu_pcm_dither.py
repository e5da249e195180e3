"""TPDF dither of the s16 / s24 encode on the MI355X (aw_spatializer_set_dither).  The dither is a pure function of (seed, global stream,
absolute frame position, ear), so every PCM entry must give numpy's dithered encode of the float entry's output at the known positions, bit
for bit, with the clip counter equal to numpy's count; chunking, split calls, reset, sharding over handles and unaligned buffers must be
invisible; NONE must be today's encode.  A sine below half an s16 LSB must survive the dithered encode."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, S16, S24, S32 = 0, 1, 2, 3
NAME = {F32: "f32", S16: "s16", S24: "s24", S32: "s32"}
NONE, TPDF, TPDF_HP = 0, 1, 2
MODE = {NONE: "none", TPDF: "tpdf", TPDF_HP: "tpdf_hp"}
U64 = np.uint64


def pack_s24(s):
    u = (s.astype(np.int64) & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)


def make_pcm(rng, fmt, shape, level=0.3):
    """PCM input (numpy, in the format's host layout) at about `level` of full scale; float32 for F32."""
    if fmt == F32:
        return (rng.standard_normal(shape) * level).astype(np.float32)
    bits = {S16: 16, S24: 24, S32: 32}[fmt]
    top = 2 ** (bits - 1)
    s = np.clip(np.rint(rng.standard_normal(shape) * level * top), -top, top - 1).astype(np.int64)
    return {S16: lambda: s.astype(np.int16), S24: lambda: pack_s24(s), S32: lambda: s.astype(np.int32)}[fmt]()


def encode(fmt, x):
    with np.errstate(over="ignore", invalid="ignore"):
        if fmt == S32:
            v, lo, hi = np.rint(x.astype(np.float64) * 2147483648.0), -2.0 ** 31, 2.0 ** 31 - 1
        else:
            v = np.rint(x * np.float32(32768 if fmt == S16 else 8388608)).astype(np.float64)
            lo, hi = (-32768.0, 32767.0) if fmt == S16 else (-8388608.0, 8388607.0)
        clipped = ~((v >= lo) & (v <= hi))
        r = np.where(np.isnan(v), 0.0, np.clip(v, lo, hi)).astype(np.int64)
    out = {S16: lambda: r.astype(np.int16), S24: lambda: pack_s24(r), S32: lambda: r.astype(np.int32)}[fmt]()
    return out, int(clipped.sum())


def np_splitmix64(z):
    z = np.asarray(z, U64) + U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def np_dither(mode, seed, g, p, ear):
    """The documented dither in LSB (float32), broadcast over global stream g, frame position p and ear (uint64 arrays)."""
    k = ((U64(seed) ^ U64(0xD1B54A32D192ED03)) + g) * U64(0x9E3779B97F4A7C15)
    if mode == TPDF:
        h = np_splitmix64(k + U64(2) * p + ear)
        return ((h >> U64(40)).astype(np.int64) - ((h >> U64(16)) & U64(0xFFFFFF)).astype(np.int64)).astype(np.float32) * np.float32(2.0 ** -24)
    sh = np.where(ear != 0, U64(16), U64(40))
    r = lambda h: ((h >> sh) & U64(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)
    return r(np_splitmix64(k + p)) - r(np_splitmix64(k + p - U64(1)))


def encode_dithered(fmt, mode, y, seed, first_stream=0, pos0=0):
    """numpy's encode of float output y [S, F, 2] whose streams are global first_stream.. and whose frames sit at positions pos0..;
    returns (array in fmt's host layout, clipped count).  NONE, s32 and f32 are the plain encode."""
    if mode == NONE or fmt not in (S16, S24):
        return encode(fmt, y)
    S, F, _ = y.shape
    g = (U64(first_stream) + np.arange(S, dtype=U64))[:, None, None]
    p = (U64(pos0) + np.arange(F, dtype=U64))[None, :, None]
    d = np_dither(mode, seed, g, p, np.arange(2, dtype=U64)[None, None, :])
    scale = np.float32(32768.0 if fmt == S16 else 8388608.0)
    lo, hi = (-32768.0, 32767.0) if fmt == S16 else (-8388608.0, 8388607.0)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(y * scale + d).astype(np.float64)
        clipped = ~((v >= lo) & (v <= hi))
        r = np.where(np.isnan(v), 0.0, np.clip(v, lo, hi)).astype(np.int64)
    return (r.astype(np.int16) if fmt == S16 else pack_s24(r)), int(clipped.sum())


def out_host(fmt, S, F):
    return {F32: lambda: np.full((S, F, 2), np.nan, np.float32), S16: lambda: np.zeros((S, F, 2), np.int16),
            S24: lambda: np.zeros((S, F, 2, 3), np.uint8), S32: lambda: np.zeros((S, F, 2), np.int32)}[fmt]()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()


def from_dev(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def context(aw, torch, chunk_mb=None, ola_min_blocks=None):
    env = {"AW_HOST_CHUNK_MB": chunk_mb, "AW_OLA_MIN_BLOCKS": ola_min_blocks}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = str(v)                     # knobs are read once, at context creation
        return aw.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def layout(channels):
    return (np.arange(channels) % 14).astype(np.int32), ((np.arange(channels) * 3 + 7) % 14).astype(np.int32)


def run_pcm_device(aw, torch, sp, x_pcm, fin, fout, splits, clip_t=None):
    """process_pcm over consecutive calls; returns the concatenated host output in fout's layout."""
    S = x_pcm.shape[0]
    outs, at = [], 0
    for n in splits:
        xs = x_pcm[:, at:at + n]
        yo = out_host(fout, S, n)
        xd, yd = to_dev(torch, xs), torch.empty(yo.nbytes, dtype=torch.uint8, device="cuda")
        sp.process_pcm_device(xd.data_ptr(), NAME[fin], yd.data_ptr(), NAME[fout], n, 0 if clip_t is None else clip_t.data_ptr())
        torch.cuda.synchronize()
        outs.append(from_dev(yd, yo))
        at += n
    return np.concatenate(outs, axis=1)


def spatializer(aw, ctx, h, lt, rt, S, mode=NONE, seed=0, first_stream=0):
    sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    if mode != NONE:
        sp.set_dither(MODE[mode], seed=seed, first_stream=first_stream)
    return sp


# (taps, channels, streams, two call lengths, the info() key that shows the expected kernel family)
LAYOUTS = [
    pytest.param(4320, 8, 48, (20001, 18999), "overlap_add_rows", id="ola8"),
    pytest.param(32768, 7, 6, (200001, 220003), "long_window_rows", id="longwin7"),
]


@pytest.mark.parametrize("taps,channels,streams,splits,path_key", LAYOUTS)
def test_dithered_device_entry_equals_numpy(oracle, taps, channels, streams, splits, path_key):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch, chunk_mb=8, ola_min_blocks=0 if path_key == "overlap_add_rows" else None)
    h = oracle.synth_hrir(14, taps, seed=31)
    lt, rt = layout(channels)
    rng = np.random.default_rng(taps + channels)
    for fin in (F32, S16):
        x = make_pcm(rng, fin, (streams, sum(splits), channels), level=0.5)
        ref_sp = spatializer(aw, ctx, h, lt, rt, streams)
        yf = run_pcm_device(aw, torch, ref_sp, x, fin, F32, splits)
        assert ref_sp.info()[path_key] > 0, ref_sp.info()
        for fout in (S16, S24):
            for mode in (TPDF, TPDF_HP):
                seed, first = 0xD17 + 16 * fout + mode, 1000 * mode
                sp = spatializer(aw, ctx, h, lt, rt, streams, mode, seed, first)
                clip_t = torch.zeros(1, dtype=torch.int64, device="cuda")
                got = run_pcm_device(aw, torch, sp, x, fin, fout, splits, clip_t)
                want, n_clip = encode_dithered(fout, mode, yf, seed, first)
                assert np.array_equal(got, want), (NAME[fin], NAME[fout], MODE[mode])
                assert int(clip_t.item()) == n_clip, (NAME[fin], NAME[fout], MODE[mode], int(clip_t.item()), n_clip)
                assert sp.info()["position_frames"] == sum(splits)
                if fout == S16:
                    plain, _ = encode(S16, yf)
                    assert np.mean(got != plain) > 0.05                    # the dither changed a real share of the samples


@pytest.mark.parametrize("pinned", [True, False])
def test_dithered_host_entry_chunked_equals_numpy(oracle, pinned):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch, chunk_mb=2)
    h = oracle.synth_hrir(14, 4320, seed=32)
    lt, rt = layout(8)
    S, splits = 24, (60001, 40003)
    rng = np.random.default_rng(33)
    x_all = make_pcm(rng, S16, (S, sum(splits), 8), level=0.5)
    yf = run_pcm_device(aw, torch, spatializer(aw, ctx, h, lt, rt, S), x_all, S16, F32, splits)
    for fout, mode in ((S16, TPDF), (S16, TPDF_HP), (S24, TPDF)):
        sp = spatializer(aw, ctx, h, lt, rt, S, mode, seed=77, first_stream=5)
        sp.reserve_pcm(max(splits), "s16", NAME[fout])
        allocs = sp.info()["device_allocs"]
        got, at, clips = [], 0, 0
        for n in splits:
            xs = np.ascontiguousarray(x_all[:, at:at + n])
            yo = out_host(fout, S, n)
            if pinned:
                x, y = ctx.pinned_empty(xs.shape, xs.dtype), ctx.pinned_empty(yo.shape, yo.dtype)
                x[...] = xs
                allocs += 2
            else:
                x, y = xs, yo
            clips += sp.process_host_into(x, y, out_format=NAME[fout])
            assert sp.info()["device_allocs"] == allocs                # reserve_pcm sized everything: dither allocates nothing
            got.append(np.array(y))
            at += n
        assert 0 < sp.info()["host_chunk_streams"] < S
        want, n_clip = encode_dithered(fout, mode, yf, 77, 5)
        assert np.array_equal(np.concatenate(got, axis=1), want), (NAME[fout], MODE[mode])
        assert clips == n_clip


def test_dithered_single_stream_callback_path_equals_numpy(oracle):
    """One stream, callback-sized calls: the zero-copy path encodes on the CPU with the same rule (pcm.hpp)."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    h = oracle.synth_hrir(14, 4320, seed=34)
    lt, rt = layout(2)
    calls = [4096, 4096, 1023, 4096]
    x_all = make_pcm(np.random.default_rng(35), S16, (1, sum(calls), 2), level=0.9)
    yf = run_pcm_device(aw, torch, spatializer(aw, ctx, h, lt, rt, 1), x_all, S16, F32, calls)
    for fout, mode in ((S16, TPDF), (S16, TPDF_HP), (S24, TPDF_HP)):
        sp = spatializer(aw, ctx, h, lt, rt, 1, mode, seed=3, first_stream=41)
        sp.reserve_pcm(4096, "s16", NAME[fout])
        allocs = sp.info()["device_allocs"]
        got, at, clips = [], 0, 0
        for n in calls:
            y = out_host(fout, 1, n)
            clips += sp.process_host_into(np.ascontiguousarray(x_all[:, at:at + n]), y, out_format=NAME[fout])
            got.append(y)
            at += n
        assert sp.info()["device_allocs"] == allocs and sp.info()["host_chunk_streams"] == 0
        want, n_clip = encode_dithered(fout, mode, yf, 3, 41)
        assert np.array_equal(np.concatenate(got, axis=1), want), (NAME[fout], MODE[mode])
        assert clips == n_clip


def test_tiny_calls_and_unaligned_buffers_equal_numpy(oracle):
    """Calls of 1, 3 and 7 frames (a 16-element group of the encode spans several streams) and device buffers at odd byte offsets
    (the kernels' heads and tails)."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    h = oracle.synth_hrir(14, 4320, seed=36)
    lt, rt = layout(3)
    S = 5
    rng = np.random.default_rng(37)
    calls = [1, 3, 7, 1, 2, 7, 3, 64]
    x = make_pcm(rng, S16, (S, sum(calls), 3), level=0.7)
    yf = run_pcm_device(aw, torch, spatializer(aw, ctx, h, lt, rt, S), x, S16, F32, calls)
    for fout in (S16, S24):
        for mode in (TPDF, TPDF_HP):
            sp = spatializer(aw, ctx, h, lt, rt, S, mode, seed=mode, first_stream=9)
            got = run_pcm_device(aw, torch, sp, x, S16, fout, calls)
            assert np.array_equal(got, encode_dithered(fout, mode, yf, mode, 9)[0]), (NAME[fout], MODE[mode])
    F = 3001
    x = make_pcm(rng, S16, (S, F, 3), level=0.9)
    yf = run_pcm_device(aw, torch, spatializer(aw, ctx, h, lt, rt, S), x, S16, F32, [F])
    for fout, mode in ((S16, TPDF), (S24, TPDF_HP), (S16, TPDF_HP), (S24, TPDF)):
        want, n_clip = encode_dithered(fout, mode, yf, 8, 2)
        for off_in, off_out in ((1, 0), (0, 3), (5, 7), (14, 13), (2, 6)):
            sp = spatializer(aw, ctx, h, lt, rt, S, mode, seed=8, first_stream=2)
            xb = torch.zeros(x.nbytes + 32, dtype=torch.uint8, device="cuda")
            xb[off_in:off_in + x.nbytes] = to_dev(torch, x)
            yo = out_host(fout, S, F)
            yb = torch.full((yo.nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
            clip_t = torch.zeros(1, dtype=torch.int64, device="cuda")
            sp.process_pcm_device(xb.data_ptr() + off_in, "s16", yb.data_ptr() + off_out, NAME[fout], F, clip_t.data_ptr())
            torch.cuda.synchronize()
            yh = yb.cpu().numpy()
            assert np.array_equal(yh[off_out:off_out + yo.nbytes].view(yo.dtype).reshape(yo.shape), want), (NAME[fout], MODE[mode], off_in, off_out)
            assert (yh[:off_out] == 0xA5).all() and (yh[off_out + yo.nbytes:] == 0xA5).all()     # nothing written outside
            assert int(clip_t.item()) == n_clip


def test_split_calls_reset_and_sharding_change_no_bit(oracle):
    """On silent input the output is the dither alone, a function of (stream, position, ear): one call of F frames, calls of F1 + F2,
    the same after reset, and two handles of S / 2 streams (first_stream 0 and S / 2) must all give the same bytes."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch, chunk_mb=1)
    h = oracle.synth_hrir(14, 4320, seed=38)
    lt, rt = layout(4)
    S, F, F1 = 8, 100007, 40013
    x = np.zeros((S, F, 4), np.int16)
    for mode in (TPDF, TPDF_HP):
        one = spatializer(aw, ctx, h, lt, rt, S, mode, seed=21)
        a = run_pcm_device(aw, torch, one, x, S16, S16, [F])
        assert set(np.unique(a).tolist()) == {-1, 0, 1} and 0.2 < np.mean(a != 0) < 0.3
        assert np.array_equal(a, encode_dithered(S16, mode, np.zeros((S, F, 2), np.float32), 21)[0])
        two = spatializer(aw, ctx, h, lt, rt, S, mode, seed=21)
        assert np.array_equal(run_pcm_device(aw, torch, two, x, S16, S16, [F1, F - F1]), a)
        assert one.info()["position_frames"] == two.info()["position_frames"] == F
        b = run_pcm_device(aw, torch, one, x, S16, S16, [F])
        assert not np.array_equal(b, a)                            # the position moved on
        one.reset()
        assert one.info()["position_frames"] == 0
        assert np.array_equal(run_pcm_device(aw, torch, one, x, S16, S16, [F]), a)
        halves = [spatializer(aw, ctx, h, lt, rt, S // 2, mode, seed=21, first_stream=k * S // 2) for k in (0, 1)]
        sh = [run_pcm_device(aw, torch, halves[k], x[k * S // 2:(k + 1) * S // 2], S16, S16, [F1, F - F1]) for k in (0, 1)]
        assert np.array_equal(np.concatenate(sh, axis=0), a)
        # the host entry, chunked by streams, and a float call that advances the position in between
        host = spatializer(aw, ctx, h, lt, rt, S, mode, seed=21)
        y1 = np.zeros((S, F1, 2), np.int16)
        host.process_host_into(np.ascontiguousarray(x[:, :F1]), y1)
        assert host.info()["host_chunk_streams"] > 0
        xf, yf = torch.zeros((S, F - F1, 4), device="cuda"), torch.empty((S, F - F1, 2), device="cuda")
        host.process_device(xf.data_ptr(), yf.data_ptr(), F - F1)
        assert host.info()["position_frames"] == F
        y2 = np.zeros((S, F, 2), np.int16)
        host.process_host_into(x, y2)
        assert np.array_equal(y1, a[:, :F1]) and np.array_equal(y2, b)


def test_sine_below_half_an_lsb_survives_dither():
    """A -100 dBFS sine (0.33 LSB of s16) through a delta HRIR: undithered s16 output is digital silence; with TPDF (and the high-pass
    form) correlating the output with the sine recovers the amplitude, and the noise power is 1/4 LSB^2 (1/12 of the rounding + 1/6 of
    the dither).  Full-scale input: samples that the dither pushes past full scale are counted as clipped."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    h = np.zeros((2, 256), np.float32)
    h[:, 0] = 1.0
    lt, rt = np.array([0], np.int32), np.array([1], np.int32)
    F = 1 << 20
    amp = 10.0 ** (-100 / 20)
    w = 2 * np.pi * 997.0 / 48000.0
    s = np.sin(w * np.arange(F))
    x = (amp * s).astype(np.float32).reshape(1, F, 1)
    ref = run_pcm_device(aw, torch, spatializer(aw, ctx, h, lt, rt, 1), x, F32, F32, [F])
    assert np.abs(ref[0, :, 0] - x[0, :, 0]).max() < 1e-9                 # the delta HRIR passes the sine through
    plain = run_pcm_device(aw, torch, spatializer(aw, ctx, h, lt, rt, 1), x, F32, S16, [F])
    assert not plain.any()                                                 # below half an LSB: silence without dither
    a_lsb = amp * 32768.0
    for mode in (TPDF, TPDF_HP):
        y = run_pcm_device(aw, torch, spatializer(aw, ctx, h, lt, rt, 1, mode, seed=1), x, F32, S16, [F]).astype(np.float64)
        for ear in (0, 1):
            ye = y[0, :, ear]
            got = 2.0 * np.mean(ye * s)
            assert abs(got / a_lsb - 1.0) < 0.1, (MODE[mode], ear, got, a_lsb)
            noise = np.mean((ye - a_lsb * s) ** 2)
            assert 0.22 < noise < 0.28, (MODE[mode], ear, noise)
    # full scale: the dither pushes about 1/8 of the samples at 32767 / 32768 past it
    xf = np.full((1, 65536, 1), 32767, np.int16)
    yf = run_pcm_device(aw, torch, spatializer(aw, ctx, h, lt, rt, 1), xf, S16, F32, [65536])
    for mode in (TPDF, TPDF_HP):
        clip_t = torch.zeros(1, dtype=torch.int64, device="cuda")
        got = run_pcm_device(aw, torch, spatializer(aw, ctx, h, lt, rt, 1, mode, seed=2), xf, S16, S16, [65536], clip_t)
        want, n_clip = encode_dithered(S16, mode, yf, 2)
        assert np.array_equal(got, want) and int(clip_t.item()) == n_clip
        assert 0.1 < n_clip / yf.size < 0.15, n_clip / yf.size


def test_none_after_dither_is_the_undithered_encode(oracle):
    """set_dither(NONE) after dithered calls gives the bytes of a handle that was never set; s32 output is never dithered; a reserved
    device entry allocates nothing with dither on."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    h = oracle.synth_hrir(14, 4320, seed=39)
    lt, rt = layout(6)
    S, splits = 12, (30011, 20021)
    x = make_pcm(np.random.default_rng(40), S16, (S, sum(splits), 6), level=0.5)
    for fout in (S16, S24, S32):
        never = spatializer(aw, ctx, h, lt, rt, S)
        a = [run_pcm_device(aw, torch, never, x[:, :splits[0]], S16, fout, [splits[0]]),
             run_pcm_device(aw, torch, never, x[:, splits[0]:], S16, fout, [splits[1]])]
        sp = spatializer(aw, ctx, h, lt, rt, S, TPDF, seed=4)
        sp.reserve_pcm(max(splits), "s16", NAME[fout])
        allocs = sp.info()["device_allocs"]
        b0 = run_pcm_device(aw, torch, sp, x[:, :splits[0]], S16, fout, [splits[0]])
        assert sp.info()["device_allocs"] == allocs
        assert np.array_equal(b0, a[0]) == (fout == S32)                  # s32 is never dithered
        sp.set_dither("none")
        assert np.array_equal(run_pcm_device(aw, torch, sp, x[:, splits[0]:], S16, fout, [splits[1]]), a[1]), NAME[fout]
