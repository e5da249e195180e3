"""CPU-side checks of the integer PCM sample formats (include/airwave_hip.h, aw_sample_format): the element rules of
airwave_amd/csrc/device/pcm.hpp, compiled by plain g++ into a test-only library, against the numpy restatement of the documented
rule and against aw_wav_load's decoder; the format table of the C ABI; and the argument checks that run before any HIP call."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import airwave_amd as aw
from airwave_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCM_HPP = os.path.join(ROOT, "airwave_amd", "csrc", "device", "pcm.hpp")
F32, S16, S24, S32 = 0, 1, 2, 3
AW_ERR_INVALID_ARGUMENT = 1

SHIM = r"""
#include "pcm.hpp"
extern "C" {
int pcm_format_bytes(int f) { return awp::format_bytes(f); }
void pcm_decode(int fmt, const unsigned char *src, float *dst, long n) {
    const int b = awp::format_bytes(fmt);
    for (long i = 0; i < n; ++i) dst[i] = awp::decode_at(fmt, src + i * b);
}
void pcm_encode(int fmt, const float *src, unsigned char *dst, unsigned char *clip, long n) {
    const int b = awp::format_bytes(fmt);
    for (long i = 0; i < n; ++i) { unsigned k = 0; awp::encode_at(fmt, src[i], dst + i * b, &k); clip[i] = (unsigned char)k; }
}
}
"""


@pytest.fixture(scope="module")
def pcm(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcm_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libpcm_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + os.path.dirname(PCM_HPP), str(src), "-o", str(so)],
                   check=True)
    lib = ctypes.CDLL(str(so))
    lib.pcm_format_bytes.restype = ctypes.c_int
    lib.pcm_format_bytes.argtypes = [ctypes.c_int]
    lib.pcm_decode.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    lib.pcm_encode.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    return lib


def pack_s24(s: np.ndarray) -> np.ndarray:
    u = (s.astype(np.int64) & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)


def unpack_s24(b: np.ndarray) -> np.ndarray:
    u = b[..., 0].astype(np.int32) | (b[..., 1].astype(np.int32) << 8) | (b[..., 2].astype(np.int32) << 16)
    return np.where(u & 0x800000, u - 0x1000000, u).astype(np.int32)


def np_decode(fmt, s):
    """aw_wav_load's rule (host/host_api.cpp), restated."""
    if fmt == S16:
        return s.astype(np.float32) / np.float32(32768.0)
    if fmt == S24:
        return (s.astype(np.float64) / 8388608.0).astype(np.float32)
    return (s.astype(np.float64) / 2147483648.0).astype(np.float32)


def np_encode(fmt, x):
    """The documented encode rule: inverse scale, round half to even, saturate; s32 in double; NaN -> 0.  Returns (ints, clipped)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if fmt == S32:
            v, lo, hi = np.rint(x.astype(np.float64) * 2147483648.0), -2.0 ** 31, 2.0 ** 31 - 1
        else:
            scale = np.float32(32768.0 if fmt == S16 else 8388608.0)
            v = np.rint(x * scale).astype(np.float64)
            lo, hi = (-32768.0, 32767.0) if fmt == S16 else (-8388608.0, 8388607.0)
        clipped = ~((v >= lo) & (v <= hi))
        r = np.where(np.isnan(v), 0.0, np.clip(v, lo, hi))
    return r.astype(np.int64), clipped


def run_decode(lib, fmt, raw: np.ndarray, n: int) -> np.ndarray:
    raw = np.ascontiguousarray(raw)
    out = np.empty(n, np.float32)
    lib.pcm_decode(fmt, raw.ctypes.data, out.ctypes.data, n)
    return out


def run_encode(lib, fmt, x: np.ndarray):
    x = np.ascontiguousarray(x, np.float32)
    n = x.size
    raw = np.zeros(n * {S16: 2, S24: 3, S32: 4}[fmt], np.uint8)
    clip = np.zeros(n, np.uint8)
    lib.pcm_encode(fmt, x.ctypes.data, raw.ctypes.data, clip.ctypes.data, n)
    if fmt == S16:
        ints = raw.view(np.int16).astype(np.int64)
    elif fmt == S24:
        ints = unpack_s24(raw.reshape(n, 3)).astype(np.int64)
    else:
        ints = raw.view(np.int32).astype(np.int64)
    return ints, clip.astype(bool)


def test_format_bytes_table(pcm):
    lib = _capi.load()
    for f, b in ((F32, 4), (S16, 2), (S24, 3), (S32, 4), (4, 0), (-1, 0), (1 << 20, 0)):
        assert lib.aw_sample_format_bytes(f) == b
        assert pcm.pcm_format_bytes(f) == b
    assert [aw.sample_format_bytes(n) for n in ("f32", "s16", "s24", "s32", "u8")] == [4, 2, 3, 4, 0]


def test_decode_every_s16_value(pcm):
    s = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    got = run_decode(pcm, S16, s.view(np.uint8), s.size)
    assert np.array_equal(got.view(np.uint32), np_decode(S16, s).view(np.uint32))


def test_decode_every_s24_value(pcm):
    s = np.arange(-(1 << 23), 1 << 23, dtype=np.int32)
    got = run_decode(pcm, S24, pack_s24(s).reshape(-1), s.size)
    assert np.array_equal(got.view(np.uint32), np_decode(S24, s).view(np.uint32))


def test_decode_s32_dense_and_edges(pcm):
    rng = np.random.default_rng(7)
    edges = np.array([-2 ** 31, -2 ** 31 + 1, -2 ** 31 + 64, -2 ** 31 + 127, -2 ** 31 + 128, -2 ** 31 + 129, -1, 0, 1, 2 ** 24 - 1, 2 ** 24 + 1,
                      2 ** 31 - 129, 2 ** 31 - 128, 2 ** 31 - 127, 2 ** 31 - 64, 2 ** 31 - 1], np.int64)
    s = np.concatenate([edges, np.arange(-2 ** 31, 2 ** 31 - 1, 4099, dtype=np.int64), rng.integers(-2 ** 31, 2 ** 31, 1 << 18)]).astype(np.int32)
    got = run_decode(pcm, S32, s.view(np.uint8), s.size)
    assert np.array_equal(got.view(np.uint32), np_decode(S32, s).view(np.uint32))


def _write_wav(path, bits, data_ints, channels):
    if bits == 16:
        payload = data_ints.astype("<i2").tobytes()
    elif bits == 24:
        payload = pack_s24(data_ints).tobytes()
    else:
        payload = data_ints.astype("<i4").tobytes()
    bps = bits // 8
    fmt = struct.pack("<HHIIHH", 1, channels, 48000, 48000 * channels * bps, channels * bps, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload)) + payload
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)


@pytest.mark.parametrize("bits,fmt", [(16, S16), (24, S24), (32, S32)])
def test_decode_matches_wav_loader(pcm, tmp_path, bits, fmt):
    rng = np.random.default_rng(bits)
    ch, frames = 3, 4001
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1))
    s = rng.integers(lo, hi, size=(frames, ch), dtype=np.int64)
    s[:4] = [[lo, hi - 1, 0], [-1, 1, lo + 1], [hi - 2, lo, hi - 1], [0, 0, 0]]
    p = tmp_path / f"pcm{bits}.wav"
    _write_wav(p, bits, s.reshape(-1), ch)
    w = aw.WAVLoader.load(str(p))
    loaded = np.asarray(w.audio_data, np.float32).reshape(ch, frames).T          # planar [ch][frames] -> interleaved
    raw = {S16: lambda: s.astype(np.int16).view(np.uint8), S24: lambda: pack_s24(s.reshape(-1)).reshape(-1),
           S32: lambda: s.astype(np.int32).view(np.uint8)}[fmt]()
    got = run_decode(pcm, fmt, raw.reshape(-1), s.size).reshape(frames, ch)
    assert np.array_equal(got.view(np.uint32), loaded.view(np.uint32))


def _edge_floats():
    f = np.float32
    vals = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 1e30, -1e30, np.inf, -np.inf, np.nan, -np.nan,
            np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny,
            1e-45, -1e-45, 1e-40, -1e-40, np.nextafter(f(1.0), f(0.0)), np.nextafter(f(-1.0), f(0.0)),
            np.nextafter(f(1.0), f(2.0)), np.nextafter(f(-1.0), f(-2.0))]
    for scale in (32768.0, 8388608.0, 2147483648.0):
        # just inside / outside full scale, exact .5 ties on both sides of zero, values next to the top tie
        tie = f((scale - 0.5) / scale)
        vals += [f((scale - 1) / scale), f(-(scale - 1) / scale), tie, f(-(scale + 0.5) / scale),
                 f((scale + 0.5) / scale), f(0.5 / scale), f(-0.5 / scale), f(1.5 / scale), f(-1.5 / scale), f(2.5 / scale), f(-2.5 / scale),
                 f((scale - 1.5) / scale), f(-(scale - 1.5) / scale), f(3.5 / scale), np.nextafter(tie, f(0)), np.nextafter(tie, f(2))]
    # s32 near +-2^31: every float between 1 - 2^-20 and 1 + 2^-20 and their negatives
    one = np.float32(1.0)
    u = one.view(np.uint32)
    near = np.arange(u - 4096, u + 4096, dtype=np.uint32).view(np.float32)
    return np.concatenate([np.array(vals, np.float32), near, -near])


@pytest.mark.parametrize("fmt", [S16, S24, S32])
def test_encode_edge_cases(pcm, fmt):
    x = _edge_floats()
    got, clip = run_encode(pcm, fmt, x)
    ref, rclip = np_encode(fmt, x)
    assert np.array_equal(got, ref)
    assert np.array_equal(clip, rclip)
    # spot checks of the rule itself
    top = {S16: 32767, S24: 8388607, S32: 2 ** 31 - 1}[fmt]
    e, c = run_encode(pcm, fmt, np.array([1.0, -1.0, np.nan, np.inf, -np.inf, 0.0], np.float32))
    assert list(e) == [top, -top - 1, 0, top, -top - 1, 0]
    assert list(c) == [True, False, True, True, True, False]


@pytest.mark.parametrize("fmt", [S16, S24, S32])
def test_encode_random_and_round_trip(pcm, fmt):
    rng = np.random.default_rng(11 + fmt)
    x = (rng.standard_normal(1 << 18) * 0.6).astype(np.float32)          # about 10 % past full scale
    got, clip = run_encode(pcm, fmt, x)
    ref, rclip = np_encode(fmt, x)
    assert np.array_equal(got, ref) and np.array_equal(clip, rclip)
    assert 0.05 < clip.mean() < 0.2
    # decode(encode(decode(s))) == decode(s): every PCM value survives the round trip unclipped
    s = rng.integers({S16: -32768, S24: -(1 << 23), S32: -2 ** 31}[fmt], {S16: 32768, S24: 1 << 23, S32: 2 ** 31}[fmt], 1 << 16)
    xs = np_decode(fmt, s)
    back, bclip = run_encode(pcm, fmt, xs)
    if fmt != S32:                                                         # (s32 decodes through float32's 24-bit mantissa)
        assert np.array_equal(back, s)
    assert not bclip.any()


# ---- the C ABI's argument checks: they return before any HIP call (no device here; a HIP call would fail otherwise) ----------------

def test_pcm_entries_reject_null_arguments():
    lib = _capi.load()
    buf = (ctypes.c_ubyte * 64)()
    dummy = (ctypes.c_ubyte * 4096)()                       # a non-NULL handle that the checks never read
    p, h = ctypes.addressof(buf), ctypes.addressof(dummy)
    n = ctypes.c_uint64(0)
    assert lib.aw_spatializer_process_pcm(None, p, S16, p, S16, 8, None) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_process_pcm(h, None, S16, p, S16, 8, None) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_process_pcm(h, p, S16, None, S16, 8, None) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_process_host_pcm(None, p, S16, p, S16, 8, ctypes.byref(n)) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_process_host_pcm(h, None, S24, p, S16, 8, ctypes.byref(n)) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_process_host_pcm(h, p, S24, None, S16, 8, None) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_reserve_pcm(None, 1024, S16, S16) == AW_ERR_INVALID_ARGUMENT
    assert b"NULL" in lib.aw_last_error_message()


def _fake_spatializer(n_streams=3, n_channels=5):
    """A Spatializer whose library is a recorder: a wrapper that checks its arguments never reaches it."""
    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def f(*a):
                self.calls.append(name)
                return 0
            return f
    sp = object.__new__(aw.Spatializer)
    sp._lib, sp._h, sp.n_streams, sp.n_channels = Recorder(), None, n_streams, n_channels
    return sp


def test_python_wrapper_rejects_wrong_dtypes_and_shapes():
    sp = _fake_spatializer()
    S, F, C = 3, 10, 5
    bad = [
        (np.zeros((S, F, C), np.float64), np.zeros((S, F, 2), np.int16), None, None, TypeError),     # float64 has no format
        (np.zeros((S, F, C), np.uint8), np.zeros((S, F, 2), np.int16), None, None, TypeError),       # packed s24 must be named
        (np.zeros((S, F, C), np.int16), np.zeros((S, F, 2), np.int16), "s32", None, TypeError),      # format / dtype disagree
        (np.zeros((S, F, C), np.int16), np.zeros((S, F, 2), np.int16), "s8", None, ValueError),      # unknown format
        (np.zeros((S, F, C + 1), np.int16), np.zeros((S, F, 2), np.int16), None, None, ValueError),  # wrong channel count
        (np.zeros((S + 1, F, C), np.int16), np.zeros((S + 1, F, 2), np.int16), None, None, ValueError),
        (np.zeros((S, F, C), np.int16), np.zeros((S, F + 1, 2), np.int16), None, None, ValueError),  # output frames differ
        (np.zeros((S, F, C, 2), np.uint8), np.zeros((S, F, 2), np.int16), "s24", None, ValueError),  # s24 needs [..., 3]
        (np.zeros((S, F, C), np.int16), np.zeros((S, F, 2, 3), np.uint8), None, None, TypeError),    # s24 output unnamed
        (np.zeros((S, F, C), np.int16), np.zeros((S, 2, F), np.int16).transpose(0, 2, 1), None, None, ValueError),   # not contiguous
    ]
    for x, y, fi, fo, exc in bad:
        with pytest.raises(exc):
            sp.process_host_into(x, y, in_format=fi, out_format=fo)
    with pytest.raises(ValueError):
        sp.process_pcm_device(0, "s12", 0, "s16", F)
    assert sp._lib.calls == []
    # well-formed calls do reach the library: int16 in / out, packed s24 in / float32 out, int32 in / packed s24 out
    assert sp.process_host_into(np.zeros((S, F, C), np.int16), np.zeros((S, F, 2), np.int16)) == 0
    sp.process_host_into(np.zeros((S, F, C, 3), np.uint8), np.zeros((S, F, 2), np.float32), in_format="s24")
    sp.process_host_into(np.zeros((S, F, C), np.int32), np.zeros((S, F, 2, 3), np.uint8), out_format="s24")
    assert sp._lib.calls == ["aw_spatializer_process_host_pcm"] * 3
