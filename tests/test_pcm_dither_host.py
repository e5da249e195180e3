"""CPU-side checks of the dither of the integer PCM encode (include/airwave_hip.h, aw_dither / aw_spatializer_set_dither): the rules of
airwave_amd/csrc/device/pcm.hpp, compiled by plain g++ into a test-only library, against a numpy restatement of the documented rule; the
statistics of the noise; the setter's argument checks, which run before any HIP call; and the constants of the C header against Python's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import airwave_amd as aw
from airwave_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCM_HPP = os.path.join(ROOT, "airwave_amd", "csrc", "device", "pcm.hpp")
F32, S16, S24, S32 = 0, 1, 2, 3
NONE, TPDF, TPDF_HP = 0, 1, 2
AW_ERR_INVALID_ARGUMENT = 1
U64 = np.uint64

SHIM = r"""
#include "pcm.hpp"
extern "C" {
unsigned long long mix(unsigned long long z) { return awp::splitmix64(z); }
void dither_values(int mode, unsigned long long seed, const unsigned long long *g, const unsigned long long *p, const int *ear, float *d, long n) {
    for (long i = 0; i < n; ++i) d[i] = awp::dither_value(mode, awp::dither_key(seed, g[i]), p[i], ear[i]);
}
void dither_encode(int fmt, int mode, unsigned long long seed, const unsigned long long *g, const unsigned long long *p, const int *ear,
                   const float *x, unsigned char *dst, unsigned char *clip, long n) {
    const int b = awp::format_bytes(fmt);
    for (long i = 0; i < n; ++i) {
        unsigned k = 0;
        awp::encode_dithered_at(fmt, mode, x[i], awp::dither_key(seed, g[i]), p[i], ear[i], dst + i * b, &k);
        clip[i] = (unsigned char)k;
    }
}
void plain_encode(int fmt, const float *x, unsigned char *dst, unsigned char *clip, long n) {
    const int b = awp::format_bytes(fmt);
    for (long i = 0; i < n; ++i) { unsigned k = 0; awp::encode_at(fmt, x[i], dst + i * b, &k); clip[i] = (unsigned char)k; }
}
}
"""


@pytest.fixture(scope="module")
def pcm(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcm_dither_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libpcm_dither_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + os.path.dirname(PCM_HPP), str(src), "-o", str(so)],
                   check=True)
    lib = ctypes.CDLL(str(so))
    lib.mix.restype = ctypes.c_ulonglong
    lib.mix.argtypes = [ctypes.c_ulonglong]
    lib.dither_values.argtypes = [ctypes.c_int, ctypes.c_ulonglong] + [ctypes.c_void_p] * 4 + [ctypes.c_long]
    lib.dither_encode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong] + [ctypes.c_void_p] * 6 + [ctypes.c_long]
    lib.plain_encode.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_long]
    return lib


# ---- numpy restatement of the documented rule (uint64 arithmetic wraps mod 2^64) ---------------------------------------------------------

def np_splitmix64(z):
    z = np.asarray(z, U64) + U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def np_key(seed, g):
    return ((U64(seed) ^ U64(0xD1B54A32D192ED03)) + np.asarray(g, U64)) * U64(0x9E3779B97F4A7C15)


def np_dither(mode, seed, g, p, ear):
    """d in LSB, float32, broadcast over g / p / ear (uint64 arrays; ear 0 or 1)."""
    k, p, ear = np_key(seed, g), np.asarray(p, U64), np.asarray(ear, U64)
    if mode == TPDF:
        h = np_splitmix64(k + U64(2) * p + ear)
        a = (h >> U64(40)).astype(np.int64)
        b = ((h >> U64(16)) & U64(0xFFFFFF)).astype(np.int64)
        return (a - b).astype(np.float32) * np.float32(2.0 ** -24)
    sh = np.where(ear != 0, U64(16), U64(40))
    r = lambda h: ((h >> sh) & U64(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)
    return r(np_splitmix64(k + p)) - r(np_splitmix64(k + p - U64(1)))


def np_encode_dithered(fmt, x, d):
    """s16 / s24: rint(x * scale + d) in float32, saturated; returns (ints, clipped)."""
    scale = np.float32(32768.0 if fmt == S16 else 8388608.0)
    lo, hi = (-32768.0, 32767.0) if fmt == S16 else (-8388608.0, 8388607.0)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(np.asarray(x, np.float32) * scale + np.asarray(d, np.float32)).astype(np.float64)
        clipped = ~((v >= lo) & (v <= hi))
        r = np.where(np.isnan(v), 0.0, np.clip(v, lo, hi))
    return r.astype(np.int64), clipped


def unpack(fmt, raw, n):
    if fmt == S16:
        return raw.view(np.int16).astype(np.int64)
    if fmt == S24:
        b = raw.reshape(n, 3)
        u = b[:, 0].astype(np.int32) | (b[:, 1].astype(np.int32) << 8) | (b[:, 2].astype(np.int32) << 16)
        return np.where(u & 0x800000, u - 0x1000000, u).astype(np.int64)
    if fmt == S32:
        return raw.view(np.int32).astype(np.int64)
    return raw.view(np.float32)


def run_values(lib, mode, seed, g, p, ear):
    g, p = np.ascontiguousarray(g, U64), np.ascontiguousarray(p, U64)
    ear = np.ascontiguousarray(ear, np.int32)
    d = np.empty(g.size, np.float32)
    lib.dither_values(mode, seed, g.ctypes.data, p.ctypes.data, ear.ctypes.data, d.ctypes.data, g.size)
    return d


def run_encode(lib, fmt, mode, seed, g, p, ear, x):
    g, p = np.ascontiguousarray(g, U64), np.ascontiguousarray(p, U64)
    ear, x = np.ascontiguousarray(ear, np.int32), np.ascontiguousarray(x, np.float32)
    n = x.size
    raw = np.zeros(n * {F32: 4, S16: 2, S24: 3, S32: 4}[fmt], np.uint8)
    clip = np.zeros(n, np.uint8)
    lib.dither_encode(fmt, mode, seed, g.ctypes.data, p.ctypes.data, ear.ctypes.data, x.ctypes.data, raw.ctypes.data, clip.ctypes.data, n)
    return raw, clip.astype(bool)


def run_plain(lib, fmt, x):
    x = np.ascontiguousarray(x, np.float32)
    raw = np.zeros(x.size * {F32: 4, S16: 2, S24: 3, S32: 4}[fmt], np.uint8)
    clip = np.zeros(x.size, np.uint8)
    lib.plain_encode(fmt, x.ctypes.data, raw.ctypes.data, clip.ctypes.data, x.size)
    return raw, clip.astype(bool)


def coordinates(rng, n):
    """(g, p, ear) over many streams and positions: random, p = 0 (the high-pass rule's wrap) and just past it, p near 2^64, g near
    2^64, p spread over the whole range."""
    top = U64(np.iinfo(np.uint64).max)
    g = rng.integers(0, 1 << 20, n, dtype=np.uint64)
    p = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    p[: n // 8] = 0
    p[n // 8: n // 4] = rng.integers(0, 4, n // 4 - n // 8, dtype=np.uint64)
    p[n // 4: n // 3] = top - rng.integers(0, 3, n // 3 - n // 4, dtype=np.uint64)
    g[n // 3: n // 2] = top - rng.integers(0, 1000, n // 2 - n // 3, dtype=np.uint64)
    p[n // 2: 2 * n // 3] = rng.integers(0, np.iinfo(np.int64).max, 2 * n // 3 - n // 2, dtype=np.int64).astype(np.uint64) * U64(2)
    ear = rng.integers(0, 2, n).astype(np.uint64)
    return g, p, ear


def test_splitmix64_is_the_synth_generator(pcm):
    z = np.array([0, 1, 2, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, (1 << 64) - 1, 123456789123456789], np.uint64)
    want = np_splitmix64(z)
    assert [pcm.mix(int(v)) for v in z] == [int(v) for v in want]
    assert int(want[0]) == 0xE220A8397B1DCDAF          # splitmix64's published first output for state 0


@pytest.mark.parametrize("mode", [TPDF, TPDF_HP])
def test_dither_values_match_numpy(pcm, mode):
    rng = np.random.default_rng(40 + mode)
    for seed in (0, 1, 0xA17AE, 0xD1B54A32D192ED03, (1 << 64) - 1):
        g, p, ear = coordinates(rng, 1 << 15)
        got = run_values(pcm, mode, seed, g, p, ear)
        want = np_dither(mode, seed, g, p, ear)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), seed
        assert np.all(np.abs(got) < 1.0)


def _encode_inputs(rng, fmt, n):
    scale = 32768.0 if fmt == S16 else 8388608.0
    x = (rng.standard_normal(n) * 0.3).astype(np.float32)
    # full scale and just inside / outside it, where the dither decides whether a sample clips; values around +-0.5 LSB; the specials
    edge = np.array([1.0, -1.0, (scale - 1) / scale, -(scale - 1) / scale, (scale - 0.5) / scale, -(scale + 0.5) / scale,
                     (scale - 0.25) / scale, -(scale - 0.75) / scale, (scale - 1.5) / scale, 0.5 / scale, -0.5 / scale, 0.25 / scale,
                     0.0, -0.0, np.nan, np.inf, -np.inf, 2.0, -2.0, 1e30, 1e-40], np.float32)
    x[: n // 4] = np.resize(edge, n // 4)
    near = rng.uniform(-2.0, 2.0, n // 4) / scale
    x[n // 4: n // 2] = (np.sign(near) * (1.0 - np.abs(near))).astype(np.float32)
    return x


@pytest.mark.parametrize("fmt", [S16, S24])
@pytest.mark.parametrize("mode", [TPDF, TPDF_HP])
def test_dithered_encode_matches_numpy_and_counts_clips(pcm, fmt, mode):
    rng = np.random.default_rng(7 * fmt + mode)
    n = 1 << 16
    g, p, ear = coordinates(rng, n)
    x = _encode_inputs(rng, fmt, n)
    seed = 0x5EED + fmt
    raw, clip = run_encode(pcm, fmt, mode, seed, g, p, ear, x)
    want, wclip = np_encode_dithered(fmt, x, np_dither(mode, seed, g, p, ear))
    assert np.array_equal(unpack(fmt, raw, n), want)
    assert np.array_equal(clip, wclip)
    # near full scale the dither pushes some samples that would not clip past it, and pulls some that would back inside
    _, pclip = run_plain(pcm, fmt, x)
    near = slice(n // 4, n // 2)
    assert (clip[near] & ~pclip[near]).any() and (~clip[near] & pclip[near]).any()


@pytest.mark.parametrize("fmt", [F32, S16, S24, S32])
def test_none_and_wide_formats_are_the_plain_encode(pcm, fmt):
    """NONE is encode_at byte for byte; s32 and f32 are never dithered, whatever the mode."""
    rng = np.random.default_rng(90 + fmt)
    n = 1 << 14
    g, p, ear = coordinates(rng, n)
    x = _encode_inputs(rng, S16, n)
    plain, pclip = run_plain(pcm, fmt, x)
    for mode in (NONE, TPDF, TPDF_HP) if fmt in (F32, S32) else (NONE,):
        raw, clip = run_encode(pcm, fmt, mode, 3, g, p, ear, x)
        assert np.array_equal(raw, plain) and np.array_equal(clip, pclip), mode


def test_zero_input_statistics(pcm):
    """Zero input: the rounded output is -1, 0 or 1 with P(+-1) = 1/8 each (triangular noise of (-1, 1) LSB); TPDF is white,
    the high-pass form's d has lag-1 autocorrelation -1/2 along each ear."""
    n = 1 << 20
    p = np.repeat(np.arange(n // 2, dtype=np.uint64) + U64(1000), 2)
    ear = np.tile(np.array([0, 1], np.uint64), n // 2)
    g = np.full(n, 5, np.uint64)
    x = np.zeros(n, np.float32)
    for mode in (TPDF, TPDF_HP):
        raw, clip = run_encode(pcm, S16, mode, 11, g, p, ear, x)
        v = unpack(S16, raw, n)
        assert not clip.any()
        assert set(np.unique(v).tolist()) == {-1, 0, 1}
        for s in (-1, 1):
            assert abs(np.mean(v == s) - 0.125) < 0.003, (mode, s, np.mean(v == s))
        d = run_values(pcm, mode, 11, g, p, ear).astype(np.float64)
        assert abs(d.mean()) < 0.003 and abs(d.var() - 1 / 6) < 0.003, (mode, d.mean(), d.var())
        for e in (0, 1):
            de = d[e::2]
            rho = np.corrcoef(de[:-1], de[1:])[0, 1]
            assert abs(rho - (-0.5 if mode == TPDF_HP else 0.0)) < 0.01, (mode, e, rho)
        assert abs(np.corrcoef(d[0::2], d[1::2])[0, 1]) < 0.01          # the two ears are independent
    # another stream or another seed gives other noise
    a = run_values(pcm, TPDF, 11, g, p, ear)
    assert not np.array_equal(a, run_values(pcm, TPDF, 11, g + U64(1), p, ear))
    assert not np.array_equal(a, run_values(pcm, TPDF, 12, g, p, ear))


def test_set_dither_rejects_null_handle_and_unknown_mode():
    """Argument checks return before any HIP call (no device here) and before the handle is touched."""
    lib = _capi.load()
    dummy = (ctypes.c_ubyte * 4096)()                       # a non-NULL handle that the checks never read
    h = ctypes.addressof(dummy)
    assert lib.aw_spatializer_set_dither(None, TPDF, 1, 0) == AW_ERR_INVALID_ARGUMENT
    assert b"NULL" in lib.aw_last_error_message()
    for mode in (3, -1, 1 << 20):
        assert lib.aw_spatializer_set_dither(h, mode, 1, 0) == AW_ERR_INVALID_ARGUMENT
    assert bytes(dummy) == bytes(4096)
    assert lib.aw_spatializer_info(None, 18) == -1


def test_header_constants_match_python():
    text = open(os.path.join(ROOT, "include", "airwave_hip.h")).read()
    consts = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bAW_DITHER_([A-Z_]+)\s*=\s*(\d+)", text)}
    assert consts == aw.DITHER_MODES == {"none": 0, "tpdf": 1, "tpdf_hp": 2}
    assert re.search(r"typedef\s+int32_t\s+aw_dither\s*;", text)
    assert re.search(r"aw_status\s+aw_spatializer_set_dither\s*\(\s*aw_spatializer\s*\*\s*sp\s*,\s*aw_dither\s+mode\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*uint64_t\s+first_stream\s*\)", text)


def test_python_wrapper_checks_the_mode_before_the_library():
    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def f(*a):
                self.calls.append((name, a[1:]))
                return 0
            return f
    sp = object.__new__(aw.Spatializer)
    sp._lib, sp._h, sp.n_streams, sp.n_channels = Recorder(), None, 2, 2
    with pytest.raises(ValueError):
        sp.set_dither("rectangular")
    assert sp._lib.calls == []
    sp.set_dither("tpdf", seed=9, first_stream=64)
    sp.set_dither("tpdf_hp")
    sp.set_dither(0)
    assert sp._lib.calls == [("aw_spatializer_set_dither", (1, 9, 64)), ("aw_spatializer_set_dither", (2, 0, 0)),
                             ("aw_spatializer_set_dither", (0, 0, 0))]
    assert "position_frames" in sp.info()
