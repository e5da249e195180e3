"""Integer PCM sample formats on the MI355X (aw_spatializer_process_pcm / _process_host_pcm / _reserve_pcm).  Every PCM input decodes to
an exact float32 input of the same kernels, so the PCM entries must give the float32 device entry's bits on the host-decoded input; integer
output must be the documented encode (round half to even, saturate) of those bits, with the clip counter equal to numpy's count.  Chunking,
unaligned slices and the single-stream path must be invisible."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, S16, S24, S32 = 0, 1, 2, 3
NAME = {F32: "f32", S16: "s16", S24: "s24", S32: "s32"}


def pack_s24(s):
    u = (s.astype(np.int64) & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)


def unpack_s24(b):
    u = b[..., 0].astype(np.int32) | (b[..., 1].astype(np.int32) << 8) | (b[..., 2].astype(np.int32) << 16)
    return np.where(u & 0x800000, u - 0x1000000, u).astype(np.int32)


def make_pcm(rng, fmt, shape, level=0.3):
    """PCM input (numpy, in the format's host layout) at about `level` of full scale."""
    bits = {S16: 16, S24: 24, S32: 32}[fmt]
    top = 2 ** (bits - 1)
    s = np.clip(np.rint(rng.standard_normal(shape) * level * top), -top, top - 1).astype(np.int64)
    return {S16: lambda: s.astype(np.int16), S24: lambda: pack_s24(s), S32: lambda: s.astype(np.int32)}[fmt]()


def decode(fmt, a):
    if fmt == S16:
        return a.astype(np.float32) / np.float32(32768)
    if fmt == S24:
        return (unpack_s24(a).astype(np.float64) / 8388608.0).astype(np.float32)
    return (a.astype(np.float64) / 2147483648.0).astype(np.float32)


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


def run_f32_device(aw, torch, sp, x, splits):
    S, _, C = x.shape
    outs, at = [], 0
    for n in splits:
        xd = torch.from_numpy(np.ascontiguousarray(x[:, at:at + n])).cuda()
        yd = torch.empty((S, n, 2), dtype=torch.float32, device="cuda")
        sp.process_device(xd.data_ptr(), yd.data_ptr(), n)
        torch.cuda.synchronize()
        outs.append(yd.cpu().numpy())
        at += n
    return np.concatenate(outs, axis=1)


# (taps, channels, streams, two call lengths, the info() key that shows the expected kernel family)
LAYOUTS = [
    pytest.param(4320, 8, 128, (20001, 18999), "overlap_add_rows", id="ola8"),
    pytest.param(4320, 14, 16, (20011, 17003), "overlap_add_rows", id="ola14"),
    pytest.param(32768, 7, 6, (200001, 220003), "long_window_rows", id="longwin7"),
]


@pytest.mark.parametrize("taps,channels,streams,splits,path_key", LAYOUTS)
def test_pcm_device_entry_equals_float_entry_on_decoded_input(oracle, taps, channels, streams, splits, path_key):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch, chunk_mb=8, ola_min_blocks=0 if path_key == "overlap_add_rows" else None)
    h = oracle.synth_hrir(14, taps, seed=21)
    lt, rt = layout(channels)
    rng = np.random.default_rng(taps + channels)
    for fin in (S16, S24, S32):
        x_pcm = make_pcm(rng, fin, (streams, sum(splits), channels))
        ref_sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=streams, ctx=ctx)
        ref = run_f32_device(aw, torch, ref_sp, decode(fin, x_pcm), splits)
        assert ref_sp.info()[path_key] > 0, ref_sp.info()
        sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=streams, ctx=ctx)
        got = run_pcm_device(aw, torch, sp, x_pcm, fin, F32, splits)
        assert sp.info()[path_key] > 0, sp.info()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), NAME[fin]
    assert oracle.peak_rel_error(got[0, :6000], oracle.spatialize_f64(decode(fin, x_pcm[0, :6000]), h, lt, rt)) < 1e-5


def test_pcm_encode_equals_numpy_rule_and_counts_clips(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch, chunk_mb=8, ola_min_blocks=0)
    h = oracle.synth_hrir(14, 4320, seed=22)
    lt, rt = layout(8)
    S, splits = 40, (15001, 13001)
    # an input level at which about 10 % of the output samples clip: measured on a quiet run first (the system is linear)
    probe = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    y0 = run_pcm_device(aw, torch, probe, make_pcm(np.random.default_rng(5), S16, (S, sum(splits), 8), level=0.01), S16, F32, splits)
    level = 0.01 / float(np.quantile(np.abs(y0), 0.9))
    x_pcm = make_pcm(np.random.default_rng(5), S16, (S, sum(splits), 8), level=level)
    ref_sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    yf = run_pcm_device(aw, torch, ref_sp, x_pcm, S16, F32, splits)
    for fout in (S16, S24, S32):
        sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
        clip_t = torch.zeros(1, dtype=torch.int64, device="cuda")
        got = run_pcm_device(aw, torch, sp, x_pcm, S16, fout, splits, clip_t)
        want, n_clip = encode(fout, yf)
        assert np.array_equal(got, want), NAME[fout]
        assert int(clip_t.item()) == n_clip, (NAME[fout], int(clip_t.item()), n_clip)
        assert 0.02 < n_clip / yf.size < 0.3, n_clip / yf.size           # a real share of the samples clips
    # unknown formats are refused on a live handle, before anything runs
    lib = sp._lib
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    n = ctypes.c_uint64(0)
    hb = np.zeros(4096, np.uint8)
    assert lib.aw_spatializer_process_pcm(sp._h, ctypes.c_void_p(buf.data_ptr()), 7, ctypes.c_void_p(buf.data_ptr()), S16, 8, None) == 1
    assert lib.aw_spatializer_process_pcm(sp._h, ctypes.c_void_p(buf.data_ptr()), S16, ctypes.c_void_p(buf.data_ptr()), -1, 8, None) == 1
    assert lib.aw_spatializer_process_host_pcm(sp._h, ctypes.c_void_p(hb.ctypes.data), 4, ctypes.c_void_p(hb.ctypes.data), S16, 8,
                                               ctypes.byref(n)) == 1
    assert lib.aw_spatializer_reserve_pcm(sp._h, 1024, S16, 9) == 1


def test_device_entry_at_any_byte_offset(oracle):
    """Unaligned device buffers: the kernels' heads and tails (16-byte alignment on either side) for every format pair used here."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    h = oracle.synth_hrir(14, 4320, seed=23)
    lt, rt = layout(7)
    S, F = 3, 3001
    rng = np.random.default_rng(9)
    for fin, fout in ((S24, S24), (S16, S16), (S32, S32), (S24, S16)):
        x_pcm = make_pcm(rng, fin, (S, F, 7), level=0.8)
        ref_sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
        yf = run_f32_device(aw, torch, ref_sp, decode(fin, x_pcm), [F])
        want, n_clip = encode(fout, yf)
        for off_in, off_out in ((1, 0), (0, 3), (5, 7), (14, 13), (2, 6)):
            sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
            xb = torch.zeros(x_pcm.nbytes + 32, dtype=torch.uint8, device="cuda")
            xb[off_in:off_in + x_pcm.nbytes] = to_dev(torch, x_pcm)
            yo = out_host(fout, S, F)
            yb = torch.full((yo.nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
            clip_t = torch.zeros(1, dtype=torch.int64, device="cuda")
            sp.process_pcm_device(xb.data_ptr() + off_in, NAME[fin], yb.data_ptr() + off_out, NAME[fout], F, clip_t.data_ptr())
            torch.cuda.synchronize()
            yh = yb.cpu().numpy()
            got = yh[off_out:off_out + yo.nbytes].view(yo.dtype).reshape(yo.shape)
            assert np.array_equal(got, want), (NAME[fin], NAME[fout], off_in, off_out)
            assert (yh[:off_out] == 0xA5).all() and (yh[off_out + yo.nbytes:] == 0xA5).all()     # nothing written outside
            assert int(clip_t.item()) == n_clip


@pytest.mark.parametrize("pinned", [True, False])
def test_chunked_host_pcm_entry_equals_device_pcm_entry(oracle, pinned):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch, chunk_mb=8)
    h = oracle.synth_hrir(14, 4320, seed=24)
    lt, rt = layout(8)
    S, splits = 37, (100001, 60003)
    rng = np.random.default_rng(13)
    for fin, fout in ((S16, S16), (S24, S24), (S16, F32), (F32, S16)):
        if fin == F32:
            x_all = (rng.standard_normal((S, sum(splits), 8)) * 0.4).astype(np.float32)
        else:
            x_all = make_pcm(rng, fin, (S, sum(splits), 8), level=0.5)
        ref_sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
        clip_t = torch.zeros(1, dtype=torch.int64, device="cuda")
        ref = run_pcm_device(aw, torch, ref_sp, x_all, fin, fout, splits, clip_t)
        sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
        sp.reserve_pcm(max(splits), NAME[fin], NAME[fout])
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
            clips += sp.process_host_into(x, y, in_format=NAME[fin], out_format=NAME[fout])
            assert sp.info()["device_allocs"] == allocs                # reserve_pcm sized the staging: the entry allocates nothing
            got.append(np.array(y))
            at += n
        chunk = sp.info()["host_chunk_streams"]
        assert 0 < chunk < S, chunk
        got = np.concatenate(got, axis=1)
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (NAME[fin], NAME[fout])
        assert clips == int(clip_t.item())


def test_single_stream_callback_path_equals_batch_rule(oracle):
    """One stream, callback-sized calls: the zero-copy path converts on the CPU with the same element rules (pcm.hpp)."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    h = oracle.synth_hrir(14, 4320, seed=25)
    lt, rt = layout(2)
    rng = np.random.default_rng(17)
    calls = [4096, 4096, 1023, 4096]
    for fin, fout in ((S16, S16), (S24, S24), (S32, F32), (S16, S32)):
        x_all = make_pcm(rng, fin, (1, sum(calls), 2), level=0.9)
        ref_sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=1, ctx=ctx)
        clip_t = torch.zeros(1, dtype=torch.int64, device="cuda")
        ref = run_pcm_device(aw, torch, ref_sp, x_all, fin, fout, calls, clip_t)
        sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=1, ctx=ctx)
        sp.reserve_pcm(4096, NAME[fin], NAME[fout])
        allocs = sp.info()["device_allocs"]
        got, at, clips = [], 0, 0
        for n in calls:
            y = out_host(fout, 1, n)
            clips += sp.process_host_into(np.ascontiguousarray(x_all[:, at:at + n]), y, in_format=NAME[fin], out_format=NAME[fout])
            got.append(y)
            at += n
        assert sp.info()["device_allocs"] == allocs and sp.info()["host_chunk_streams"] == 0
        got = np.concatenate(got, axis=1)
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (NAME[fin], NAME[fout])
        assert clips == int(clip_t.item())


def test_f32_through_pcm_entries_equals_the_float_entries(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch, chunk_mb=8)
    h = oracle.synth_hrir(14, 4320, seed=26)
    lt, rt = layout(8)
    S, F = 24, 90001
    xd = torch.empty((S, F, 8), dtype=torch.float32, device="cuda")
    ctx.synth_fill(xd.data_ptr(), S, F, 8, seed=31)
    torch.cuda.synchronize()
    x = xd.cpu().numpy()
    a = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    b = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    for _ in range(2):
        ya = torch.empty((S, F, 2), dtype=torch.float32, device="cuda")
        yb = torch.empty((S, F, 2), dtype=torch.float32, device="cuda")
        a.process_device(xd.data_ptr(), ya.data_ptr(), F)
        b.process_pcm_device(xd.data_ptr(), "f32", yb.data_ptr(), "f32", F)
        torch.cuda.synchronize()
        assert torch.equal(ya, yb)
    c = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    d = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    for _ in range(2):
        yc, yd = np.full((S, F, 2), np.nan, np.float32), np.full((S, F, 2), np.nan, np.float32)
        c.process_host_into(x, yc)
        n = ctypes.c_uint64(7)
        assert d._lib.aw_spatializer_process_host_pcm(d._h, ctypes.c_void_p(x.ctypes.data), F32, ctypes.c_void_p(yd.ctypes.data), F32, F,
                                                      ctypes.byref(n)) == 0
        assert n.value == 0
        assert np.array_equal(yc.view(np.uint32), yd.view(np.uint32))
        assert c.info()["host_chunk_streams"] == d.info()["host_chunk_streams"] > 0


def test_s16_host_entry_at_cfg2_size_against_the_oracle(oracle, golden_dir):
    """BASELINE cfg 2's shape (128 streams x 10 s of 7.1 -> RoomSH1.0) as s16 in / f32 out through the host entry, page-locked."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    wav = oracle.wav_load(os.path.join(golden_dir, "hrtf", "RoomSH1.0.wav"))
    tracks, lt, rt = oracle.assemble_tracks(wav, oracle.layout_detect(8))
    S, F, C = 128, 480000, 8
    rng = np.random.default_rng(0xA17AE)
    x = ctx.pinned_empty((S, F, C), np.int16)
    for s in range(S):
        x[s] = rng.integers(-8192, 8192, size=(F, C), dtype=np.int16)
    y = ctx.pinned_empty((S, F, 2), np.float32)
    sp = aw.Spatializer(aw.HRIR(tracks, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    sp.reserve_pcm(F, "s16", "f32")
    y[...] = np.nan
    assert sp.process_host_into(x, y) == 0
    assert sp.info()["host_chunk_streams"] > 0
    L = tracks.shape[1]
    for s in (0, 63, 127):
        xs = decode(S16, x[s])
        assert oracle.peak_rel_error(y[s, :8192], oracle.spatialize_f64(xs[:8192], tracks, lt, rt)) < 1e-5
        assert oracle.peak_rel_error(y[s, -4096:], oracle.spatialize_f64(xs[F - 4096 - (L - 1):], tracks, lt, rt)[-4096:]) < 1e-5
