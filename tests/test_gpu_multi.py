"""The multi-device handle on the MI355X (aw_multi_*, include/airwave_hip.h "multi-device batch spatializer").  Only ordinal 0 is opened,
listed several times: several contexts on one device, which is how a one-GPU box runs this code.

Reference.  Separately created single handles, one per non-empty shard, each with the shard's stream count on a context of its own on that
ordinal, given the same slices, the same sequence of calls and the same settings (the dither's first_stream offset by the shard's first
stream), driven one after the other on this thread.  Output bytes, the clipped total and the records must equal theirs bit for bit.  One
field is held to a bound instead: aw_stream_levels.energy, which include/airwave_hip.h documents as exact up to the ORDER of its float64
additions ("may differ between runs ... at most N * 2^-53 relative over N samples") — the meter adds one partial sum per wave with an
atomic, so two runs of ONE handle already differ there; the bound is that figure, as in tests/test_gpu_levels.py.  Against the float64
oracle the project's 1e-5 of peak holds (tests/test_gpu_parity.py).  No test compares with one handle of all the streams: its kernels are
chosen from its own stream count."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from airwave_amd import sharding
from test_gpu_eq_stage import A, C, adef
from test_multi_host import EXE, build_example

pytestmark = pytest.mark.gpu

KEEP = -2
AW_ERR_INVALID_ARGUMENT = 1
LT8 = (np.arange(8) % 14).astype(np.int32)
RT8 = ((np.arange(8) + 7) % 14).astype(np.int32)


@pytest.fixture(scope="module")
def aw():
    import airwave_amd
    return airwave_amd


@pytest.fixture(scope="module")
def hrir8(oracle):
    return oracle.synth_hrir(14, 4320, seed=23)


class Reference:
    """The separately driven handles of a device list: the methods of MultiSpatializer that the tests use, slice by slice."""

    def __init__(self, aw, devices, tracks, rate, lt, rt, streams):
        self.parts = []
        for i, ordinal in enumerate(devices):
            first, count = sharding.shard_streams(streams, len(devices), i)
            if count:
                ctx = aw.Context(ordinal)
                self.parts.append((first, count, aw.Spatializer(aw.HRIR(tracks, rate, ctx=ctx), lt, rt, n_streams=count, ctx=ctx)))

    def each(self, call):
        for first, count, sp in self.parts:
            call(sp, first, count)

    def process_into(self, x, out):
        return sum(sp.process_host_into(x[first:first + count], out[first:first + count]) for first, count, sp in self.parts)

    def gather(self, getter):
        return np.concatenate([getattr(sp, getter)() for _, _, sp in self.parts])


def f32_calls(x, lengths, into):
    """Consecutive calls over x [S, sum(lengths), C] into `into(x_call, out_call)`; returns the outputs side by side."""
    outs, at = [], 0
    for n in lengths:
        xc = np.ascontiguousarray(x[:, at:at + n])
        out = np.full((x.shape[0], n, 2), np.nan, np.float32)
        into(xc, out)
        outs.append(out)
        at += n
    return np.concatenate(outs, axis=1)


def test_float_path_pageable_and_pinned(aw, oracle, hrir8):
    S, lengths = 5, (17000, 13000)
    x = oracle.synth_input(S, sum(lengths), 8, seed=31)
    ref = Reference(aw, [0, 0], hrir8, 48000.0, LT8, RT8, S)
    assert [(f, c) for f, c, _ in ref.parts] == [(0, 3), (3, 2)]
    want = f32_calls(x, lengths, ref.process_into)
    m = aw.MultiSpatializer([0, 0], hrir8, 48000.0, LT8, RT8, S)
    assert m.shards() == [{"ordinal": 0, "first_stream": 0, "count": 3}, {"ordinal": 0, "first_stream": 3, "count": 2}]
    got = np.concatenate([m.process(np.ascontiguousarray(x[:, :lengths[0]])), m.process(np.ascontiguousarray(x[:, lengths[0]:]))], axis=1)      # pageable
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    m.reset()

    def pinned(xc, out):
        px, po = m.pinned_empty(xc.shape, np.float32), m.pinned_empty(out.shape, np.float32)
        px[...] = xc
        po[...] = np.nan
        assert m.process_host_into(px, po) == 0
        out[...] = po
    got = f32_calls(x, lengths, pinned)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for s in (0, 4):
        err = oracle.peak_rel_error(got[s], oracle.spatialize_f64(x[s], hrir8, LT8, RT8))
        print(f"stream {s}: {err:.3g} of peak against the float64 oracle")
        assert err < 1e-5


@pytest.mark.parametrize("streams,shards", [(2, [(0, 1), (1, 1), (2, 0)]), (4, [(0, 2), (2, 1), (3, 1)])])
def test_small_shards(aw, oracle, hrir8, streams, shards):
    """More shards than streams leave an empty shard that owns nothing; one-stream shards take the host entry's single-stream path
    (calls of 9000 frames: under its 16384-frame limit)."""
    lengths = (9000, 9000)
    x = oracle.synth_input(streams, sum(lengths), 8, seed=37)
    m = aw.MultiSpatializer([0, 0, 0], hrir8, 48000.0, LT8, RT8, streams)
    assert [(s["first_stream"], s["count"]) for s in m.shards()] == shards and all(s["ordinal"] == 0 for s in m.shards())
    for i, (_, count) in enumerate(shards):
        assert (m._lib.aw_multi_spatializer(m._h, i) is None) == (count == 0) == (m._lib.aw_multi_context(m._h, i) is None) == (m.shard_info(i) is None)
    ref = Reference(aw, [0, 0, 0], hrir8, 48000.0, LT8, RT8, streams)
    assert len(ref.parts) == sum(1 for _, c in shards if c)
    want = f32_calls(x, lengths, ref.process_into)
    got = f32_calls(x, lengths, m.process_host_into)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert oracle.peak_rel_error(got[streams - 1], oracle.spatialize_f64(x[streams - 1], hrir8, LT8, RT8)) < 1e-5


def test_long_hrir_on_the_long_window_kernels(aw, oracle):
    """7 channels x 32768 taps, 3 streams as 2 + 1.  tests/policy_points.py pins layouts, not call lengths; 200001 frames is the length
    tests/test_gpu_pcm_dither.py runs this layout's long-window rows at, and the planner picks them for one and for two streams too: the
    test asserts it of every shard."""
    S, C, L, F = 3, 7, 32768, 200001
    h = oracle.synth_hrir(14, L, seed=41)
    lt, rt = (np.arange(C) % 14).astype(np.int32), ((np.arange(C) + 7) % 14).astype(np.int32)
    x = oracle.synth_input(S, F, C, seed=43)
    ref = Reference(aw, [0, 0], h, 48000.0, lt, rt, S)
    want = np.full((S, F, 2), np.nan, np.float32)
    ref.process_into(x, want)
    m = aw.MultiSpatializer([0, 0], h, 48000.0, lt, rt, S)
    got = m.process(x)
    for i in range(2):
        assert m.shard_info(i)["long_window_rows"] != 0, m.shard_info(i)
    assert all(sp.info()["long_window_rows"] != 0 for _, _, sp in ref.parts)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for s in (0, S - 1):
        assert oracle.peak_rel_error(got[s], oracle.spatialize_f64(x[s], h, lt, rt)) < 1e-5


def s16_input(oracle, streams, frames, channels, seed, level=0.6):
    return np.clip(np.rint(oracle.synth_input(streams, frames, channels, seed=seed) * (level * 32768.0)), -32768, 32767).astype(np.int16)


def chain_settings(aw, target, first_stream, count, gains, dither_first):
    """Everything the whole-chain test switches on, for the multi handle (first_stream 0, every stream) or for one reference handle."""
    sl = slice(first_stream, first_stream + count)
    target.set_equalizer([adef(aw, A), adef(aw, C)], np.array([0, 1, 0, 1, -1], np.int32)[sl])
    target.set_loudness(True, 2.0)
    target.set_true_peak(True)
    target.set_metering(True)
    target.set_gain("fixed", gains[sl])
    target.set_limiter(True, 0.9, 64, 128)
    target.set_dither("tpdf_hp", 0xC0FFEE, dither_first)
    target.reserve_pcm(24000, "s16", "s16")


def test_whole_chain_s16_with_every_stage_and_a_target_change_across_the_boundary(aw, oracle, hrir8):
    S, F = 5, 24000
    x = s16_input(oracle, S, 2 * F, 8, seed=47)
    gains = np.array([0.9, 0.5, 1.3, 0.7, 1.1], np.float32)
    change = np.array([1, 0, KEEP, KEEP, 0], np.int32)          # streams 2 and 3 — the last of shard 0, the first of shard 1 — keep theirs
    ref = Reference(aw, [0, 0], hrir8, 48000.0, LT8, RT8, S)
    ref.each(lambda sp, first, count: chain_settings(aw, sp, first, count, gains, 1000 + first))
    m = aw.MultiSpatializer([0, 0], hrir8, 48000.0, LT8, RT8, S)
    chain_settings(aw, m, 0, S, gains, 1000)
    want, got, want_clip, got_clip = [], [], 0, 0
    for call in range(2):
        xc = np.ascontiguousarray(x[:, call * F:(call + 1) * F])
        if call == 1:
            ref.each(lambda sp, first, count: sp.set_equalizer_target([adef(aw, A), adef(aw, C)], change[first:first + count]))
            m.set_equalizer_target([adef(aw, A), adef(aw, C)], change)
        w, g = np.zeros((S, F, 2), np.int16), np.zeros((S, F, 2), np.int16)
        want_clip += ref.process_into(xc, w)
        got_clip += m.process_host_into(xc, g)
        want.append(w)
        got.append(g)
    assert np.array_equal(np.concatenate(got, axis=1), np.concatenate(want, axis=1)) and got_clip == want_clip
    assert np.abs(np.concatenate(got, axis=1).astype(np.int32)).max() > 8000          # (a live signal)
    lv, wlv = m.levels(), ref.gather("levels")
    for field in ("peak", "gain", "reserved", "frames", "clipped", "nonfinite"):
        assert np.array_equal(lv[field], wlv[field]), field
    assert int(lv["clipped"].sum()) == got_clip and np.array_equal(lv["gain"], gains)
    # energy: exact products, float64 additions in an order the meter leaves open (header: at most N * 2^-53 relative over N samples)
    rel = np.abs(lv["energy"] - wlv["energy"]) / wlv["energy"]
    print("energy, multi against separately driven, relative:", rel.max(), "bound", 2 * F * 2.0 ** -53)
    assert np.all(wlv["energy"] > 0) and rel.max() <= 2 * F * 2.0 ** -53
    for getter in ("loudness", "true_peak", "limiter"):
        a, b = getattr(m, getter)(), ref.gather(getter)
        assert a.tobytes() == b.tobytes(), getter
    assert np.all(np.isfinite(m.loudness()["integrated_lufs"])) and np.all(m.limiter()["frames"] == 2 * F)
    # ranges that cross the shard boundary (streams 2 | 3) and ranges inside one shard
    for getter in ("levels", "loudness", "true_peak", "limiter"):
        whole = getattr(m, getter)()
        for first, n in ((1, 3), (2, 2), (0, 5), (0, 2), (3, 2), (4, 1), (2, 1), (3, 0)):
            part = getattr(m, getter)(first, n)
            assert part.tobytes() == whole[first:first + n].tobytes(), (getter, first, n)
    # the raw hops of a stream in shard 1, against the handle that owns it
    hops = m.loudness_hops(4, 0, 10)
    assert hops.tobytes() == ref.parts[1][2].loudness_hops(1, 0, 10).tobytes() and np.all(hops > 0)
    buf = np.zeros(3, aw.LEVELS_DTYPE)
    assert m._lib.aw_multi_get_levels(m._h, 3, 3, ctypes.c_void_p(buf.ctypes.data)) == AW_ERR_INVALID_ARGUMENT          # past the last stream


def threads_now():
    return int(re.search(r"^Threads:\s+(\d+)", open("/proc/self/status").read(), re.M).group(1))


def test_no_allocation_and_no_new_thread_after_reserve(aw, oracle, hrir8):
    S, F = 5, 20000
    x = s16_input(oracle, S, F, 8, seed=53)
    out = np.zeros((S, F, 2), np.int16)
    m = aw.MultiSpatializer([0, 0], hrir8, 48000.0, LT8, RT8, S)
    m.set_dither("tpdf", 5)
    m.reserve_pcm(F, "s16", "s16")
    allocs = lambda: sum(m.shard_info(i)["device_allocs"] for i in range(2))
    a0, t0 = allocs(), threads_now()
    for _ in range(2):
        m.process_host_into(x, out)                              # pageable buffers: the bounce chunks and the copy threads were made by the reserve
        assert (allocs(), threads_now()) == (a0, t0)
    px, po = m.pinned_empty(x.shape, np.int16), m.pinned_empty(out.shape, np.int16)
    px[...] = x
    a1 = allocs()
    assert a1 == a0 + 2                                          # (the two page-locked buffers count, on the first shard's context)
    m.reset()
    m.process_host_into(px, po)
    m.reset()
    m.process_host_into(x, out)
    assert (allocs(), threads_now()) == (a1, t0) and np.array_equal(po, out)


def test_rejected_setters_change_no_shard(aw, oracle, hrir8):
    S, F = 5, 9000
    x = s16_input(oracle, S, 2 * F, 8, seed=59)
    gains = np.array([0.5, 0.6, 0.7, 0.8, 0.9], np.float32)
    ref = Reference(aw, [0, 0], hrir8, 48000.0, LT8, RT8, S)
    ref.each(lambda sp, first, count: sp.set_gain("fixed", gains[first:first + count]))
    m = aw.MultiSpatializer([0, 0], hrir8, 48000.0, LT8, RT8, S)
    m.set_gain("fixed", gains)
    want, got = np.zeros((S, 2 * F, 2), np.int16), np.zeros((S, 2 * F, 2), np.int16)
    for call in range(2):
        sl = slice(call * F, (call + 1) * F)
        xc, w, g = np.ascontiguousarray(x[:, sl]), np.zeros((S, F, 2), np.int16), np.zeros((S, F, 2), np.int16)
        if call == 1:
            # a gain array of the wrong length; a good array with one non-finite entry in the LAST shard's slice; an equalizer map whose
            # bad entry lies in the last shard's slice: shard 0's part of each is valid, and must not have been applied
            three = np.array([3.0, 3.0, 3.0], np.float32)
            assert m._lib.aw_multi_set_gain(m._h, aw.GAIN_MODES["fixed"], three.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 3, 0.0) == AW_ERR_INVALID_ARGUMENT
            bad = np.array([3.0, 3.0, 3.0, 3.0, np.inf], np.float32)
            assert m._lib.aw_multi_set_gain(m._h, aw.GAIN_MODES["fixed"], bad.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 5, 0.0) == AW_ERR_INVALID_ARGUMENT
            # (no `as excinfo` here: the traceback it holds would tie this frame, and with it the reference's contexts and handles, into a
            # reference cycle, which the collector finalizes in no particular order — a context before the handles made on it)
            for setter in (m.set_equalizer, m.set_equalizer_target):
                with pytest.raises(aw.AirwaveError, match=r"INVALID_ARGUMENT.*stream_definition\[4\]"):
                    setter([adef(aw, A)], np.array([0, 0, 0, 0, 7], np.int32))
            assert all(m.shard_info(i)["equalizer"] == 0 and m.shard_info(i)["equalizer_pending"] == 0 for i in range(2))
        ref.process_into(xc, w)
        m.process_host_into(xc, g)
        want[:, sl], got[:, sl] = w, g
    assert np.array_equal(got, want) and np.abs(got.astype(np.int32)).max() > 4000


def lcg_s16(seed, n):
    """examples/offline_batch_multi.c's input: s = s * 1664525 + 1013904223 (mod 2^32) per sample, (s >> 18) - 8192; by doubling."""
    a, c, mask = np.uint64(1664525), np.uint64(1013904223), np.uint64(0xFFFFFFFF)
    seq = np.array([(np.uint64(seed) * a + c) & mask], np.uint64)
    A_k, C_k = a, c                                              # x[i + k] = A_k x[i] + C_k with k = len(seq)
    while seq.size < n:
        seq = np.concatenate([seq, (seq * A_k + C_k) & mask])
        A_k, C_k = (A_k * A_k) & mask, (A_k * C_k + C_k) & mask
    return ((seq[:n] >> np.uint64(18)).astype(np.int64) - 8192).astype(np.int16)


def test_multi_example_writes_what_the_python_mirror_writes(aw, golden_dir, tmp_path):
    build_example()
    wav = os.path.join(golden_dir, "hrtf", "RoomSH1.0.wav")
    S, F, C = 5, 48000, 8
    out = str(tmp_path / "out.s16")
    r = subprocess.run([EXE, wav, "0,0", str(S), "1", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert re.findall(r"^shard (\d+): device (\d+) first stream (\d+) count (\d+)$", r.stdout, re.M) == [("0", "0", "0", "3"), ("1", "0", "3", "2")]
    assert re.search(r"^device 0: .+ compute units", r.stdout, re.M)
    rate = re.search(r"^streams 5 frames 48000: ([\d.]+) M stereo frames/s \([\d.]+ ms\), clipped (\d+)$", r.stdout, re.M)
    assert rate, r.stdout
    w = aw.WAVLoader.load(wav)
    layout = aw.InputLayout.detect(C)
    cmap = aw.HRIRChannelMap.hesuvi7Channel(layout) if w.channel_count == 7 else aw.HRIRChannelMap.hesuvi14Channel(layout)
    lt, rt = cmap.resolve(layout, w.channel_count)
    m = aw.MultiSpatializer([0, 0], w.audio_data, w.sample_rate, lt, rt, S)
    m.set_gain("fixed", np.float32(0.25) + np.float32(0.5) * np.arange(S, dtype=np.float32) / np.float32(S))
    m.set_dither("tpdf", 7, 0)
    x = lcg_s16(20240, S * F * C).reshape(S, F, C)
    y = np.zeros((S, F, 2), np.int16)
    clipped = m.process_host_into(x, y)
    assert np.fromfile(out, np.int16).tobytes() == y.tobytes() and int(rate.group(2)) == clipped
    assert np.abs(y.astype(np.int32)).max() > 2000
