"""CPU-side checks of the per-stream level meter and output gain (include/airwave_hip.h, aw_stream_levels / aw_spatializer_set_metering /
_get_levels / _reset_levels / _set_gain): the rules of airwave_amd/csrc/device/levels.hpp, compiled by plain g++ into a test-only library,
against numpy; the struct, the constants and the entry points of the C header against Python's; and the argument checks, which run
before any HIP call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import airwave_amd as aw
from airwave_amd import _capi
from test_pcm_dither_host import NONE, S16, S24, S32, F32, TPDF, TPDF_HP, U64, _encode_inputs, coordinates, np_dither, np_encode_dithered, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "airwave_amd", "csrc", "device")
HEADER = os.path.join(ROOT, "include", "airwave_hip.h")
AW_ERR_INVALID_ARGUMENT = 1
NEW_ENTRIES = ("aw_spatializer_set_metering", "aw_spatializer_get_levels", "aw_spatializer_reset_levels", "aw_spatializer_set_gain")

SHIM = r"""
#include <cstddef>
#include "levels.hpp"
#include "../../../include/airwave_hip.h"
extern "C" {
void contribute(const float *y, long n, unsigned *peak_bits, double *energy, unsigned *nonfinite) {
    for (long i = 0; i < n; ++i) awl::contribute(y[i], *peak_bits, *energy, *nonfinite);
}
void auto_gain(const float *p, const float *c, float *g, long n) { for (long i = 0; i < n; ++i) g[i] = awl::auto_gain(p[i], c[i]); }
void apply_gain(const float *y, const float *g, float *o, long n) { for (long i = 0; i < n; ++i) o[i] = awl::apply_gain(y[i], g[i]); }
void gained_encode(int fmt, int mode, unsigned long long seed, const unsigned long long *s, const unsigned long long *p, const int *ear,
                   const float *y, const float *g, unsigned char *dst, unsigned char *clip, long n) {
    const int b = awp::format_bytes(fmt);
    for (long i = 0; i < n; ++i) {
        unsigned k = 0;
        awl::encode_gained_at(fmt, mode, y[i], g[i], awp::dither_key(seed, s[i]), p[i], ear[i], dst + i * b, &k);
        clip[i] = (unsigned char)k;
    }
}
void layout(long *o) {
    o[0] = sizeof(aw_stream_levels); o[1] = offsetof(aw_stream_levels, peak); o[2] = offsetof(aw_stream_levels, gain);
    o[3] = offsetof(aw_stream_levels, reserved); o[4] = offsetof(aw_stream_levels, energy); o[5] = offsetof(aw_stream_levels, frames);
    o[6] = offsetof(aw_stream_levels, clipped); o[7] = offsetof(aw_stream_levels, nonfinite);
    o[8] = AW_GAIN_NONE; o[9] = AW_GAIN_FIXED; o[10] = AW_GAIN_PEAK_CEILING; o[11] = sizeof(awl::Record);
    o[12] = awl::kGainNone; o[13] = awl::kGainFixed; o[14] = awl::kGainPeakCeiling;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("levels_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "liblevels_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + DEVICE, str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.contribute.argtypes = [ctypes.c_void_p, ctypes.c_long] + [ctypes.c_void_p] * 3
    lib.auto_gain.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_long]
    lib.apply_gain.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_long]
    lib.gained_encode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong] + [ctypes.c_void_p] * 7 + [ctypes.c_long]
    lib.layout.argtypes = [ctypes.c_void_p]
    return lib


def run_contribute(lib, y):
    y = np.ascontiguousarray(y, np.float32)
    pk, en, nf = ctypes.c_uint(0), ctypes.c_double(0.0), ctypes.c_uint(0)
    lib.contribute(y.ctypes.data, y.size, ctypes.addressof(pk), ctypes.addressof(en), ctypes.addressof(nf))
    return np.array([pk.value], np.uint32).view(np.float32)[0], en.value, nf.value


def test_contribution_rule_matches_numpy(shim):
    rng = np.random.default_rng(1)
    tiny = np.float32(1e-45)                                       # the smallest denormal
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, tiny, -tiny, 1e-40, -3e-39, 3.0e38, -3.4e38, 1.0, -1.0], np.float32)
    cases = [specials, np.array([-0.0], np.float32), np.array([np.nan, np.inf], np.float32), np.array([tiny, -2 * tiny], np.float32),
             (rng.standard_normal(4097) * 0.7).astype(np.float32), np.concatenate([specials, (rng.standard_normal(1000) * 3).astype(np.float32)])]
    for y in cases:
        peak, energy, nonfinite = run_contribute(shim, y)
        fin = np.isfinite(y)
        want_peak = np.abs(y[fin]).max() if fin.any() else np.float32(0)
        assert np.float32(peak).view(np.uint32) == np.float32(want_peak).view(np.uint32)      # |-0| is +0; a denormal peak survives
        assert nonfinite == np.count_nonzero(~fin)
        want = 0.0
        for v in y[fin].astype(np.float64):                        # the same order: the sums must agree exactly
            want += v * v
        assert energy == want
    assert run_contribute(shim, np.array([tiny], np.float32))[1] == float(tiny) ** 2 > 0      # exact in double, no underflow


def test_quotient_rule_is_the_correctly_rounded_float32_quotient(shim):
    rng = np.random.default_rng(2)
    n = 1 << 18
    c = rng.uniform(0.0, 1.0, n).astype(np.float32)
    c[c == 0] = 1.0
    p = (c * rng.uniform(0.5, 40.0, n).astype(np.float32)).astype(np.float32)
    # random mantissas at all exponents, operands one ulp apart, p == c, huge and denormal peaks, the ceilings a host would use
    bits = rng.integers(0x00000001, 0x7F7FFFFF, n // 4, dtype=np.uint32)
    p[: n // 4] = bits.view(np.float32)
    p[n // 4: n // 4 + 1000] = np.nextafter(c[n // 4: n // 4 + 1000], np.float32(2))
    p[n // 4 + 1000: n // 4 + 2000] = c[n // 4 + 1000: n // 4 + 2000]
    c[n // 2: n // 2 + 4000] = np.resize(np.array([1.0, 0.98, 0.5, 0.891, 2.0 ** -24, np.nextafter(np.float32(1), np.float32(0))], np.float32), 4000)
    edge_p = np.array([3.4e38, 1e-45, 1e-40, 1.0, 1.0000001, 0.0, 0.98, 0.98000004], np.float32)
    p[-8:] = edge_p
    g = np.empty(n, np.float32)
    shim.auto_gain(p.ctypes.data, c.ctypes.data, g.ctypes.data, n)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        want = np.where(p > c, c / p, np.float32(1)).astype(np.float32)
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32))
    assert np.all(g[p <= c] == 1) and np.all(g[p > c] <= 1) and (p > c).sum() > n // 4


@pytest.mark.parametrize("fmt", [S16, S24, S32, F32])
@pytest.mark.parametrize("mode", [NONE, TPDF, TPDF_HP])
def test_gained_encode_matches_numpy(shim, fmt, mode):
    rng = np.random.default_rng(10 * fmt + mode)
    n = 1 << 15
    s, p, ear = coordinates(rng, n)
    y = _encode_inputs(rng, S16 if fmt in (F32, S32) else fmt, n)
    g = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    g[::7] = 1.0
    seed = 0x6A1 + fmt
    y, g = np.ascontiguousarray(y), np.ascontiguousarray(g)
    s, p, ear32 = np.ascontiguousarray(s, U64), np.ascontiguousarray(p, U64), np.ascontiguousarray(ear, np.int32)
    raw = np.zeros(n * {F32: 4, S16: 2, S24: 3, S32: 4}[fmt], np.uint8)
    clip = np.zeros(n, np.uint8)
    shim.gained_encode(fmt, mode, seed, s.ctypes.data, p.ctypes.data, ear32.ctypes.data, y.ctypes.data, g.ctypes.data, raw.ctypes.data,
                       clip.ctypes.data, n)
    with np.errstate(invalid="ignore", over="ignore"):
        yg = (y * g).astype(np.float32)                            # one float32 rounding
    prod = np.empty(n, np.float32)
    shim.apply_gain(y.ctypes.data, g.ctypes.data, prod.ctypes.data, n)
    both_nan = np.isnan(prod) & np.isnan(yg)
    assert np.array_equal(prod.view(np.uint32)[~both_nan], yg.view(np.uint32)[~both_nan])
    if fmt == F32:
        got = raw.view(np.float32)
        assert np.array_equal(got.view(np.uint32)[~both_nan], yg.view(np.uint32)[~both_nan]) and not clip.any()
        return
    if fmt == S32:
        with np.errstate(invalid="ignore", over="ignore"):
            v = np.rint(yg.astype(np.float64) * 2147483648.0)
            wclip = ~((v >= -2.0 ** 31) & (v <= 2.0 ** 31 - 1))
            want = np.where(np.isnan(v), 0.0, np.clip(v, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
    else:
        d = np_dither(mode, seed, s, p, ear) if mode != NONE else np.zeros(n, np.float32)
        want, wclip = np_encode_dithered(fmt, yg, d)
    assert np.array_equal(unpack(fmt, raw, n), want)
    assert np.array_equal(clip.astype(bool), wclip)


def test_struct_layout_and_constants_match_python(shim):
    o = (ctypes.c_long * 15)()
    shim.layout(ctypes.addressof(o))
    size, offs, consts = o[0], list(o[1:8]), list(o[8:11])
    names = ["peak", "gain", "reserved", "energy", "frames", "clipped", "nonfinite"]
    assert size == 56 == ctypes.sizeof(_capi.StreamLevels) == aw.LEVELS_DTYPE.itemsize
    assert offs == [getattr(_capi.StreamLevels, f).offset for f in names] == [aw.LEVELS_DTYPE.fields[f][1] for f in names]
    assert list(aw.LEVELS_DTYPE.names) == names == [f for f, _ in _capi.StreamLevels._fields_]
    assert consts == [aw.GAIN_MODES["none"], aw.GAIN_MODES["fixed"], aw.GAIN_MODES["peak_ceiling"]] == [0, 1, 2] == list(o[12:15])
    assert o[11] == 40
    text = open(HEADER).read()
    found = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bAW_GAIN_([A-Z_]+)\s*=\s*(\d+)", text)}
    assert found == aw.GAIN_MODES
    assert re.search(r"typedef\s+int32_t\s+aw_gain_mode\s*;", text)


def test_new_entries_are_declared_exported_and_typed():
    text = open(HEADER).read()
    declared = set(re.findall(r"AW_API\s+[\w\s\*]+?\b(aw_\w+)\s*\(", text))
    lib = _capi.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert declared == set(_capi.SIGNATURES)                        # every AW_API name is in the ctypes table, and nothing else is
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(NEW_ENTRIES) <= exported


def test_argument_checks_come_before_any_hip_call():
    lib = _capi.load()
    dummy = (ctypes.c_ubyte * 4096)()                              # a non-NULL handle of zero streams that the failing checks never write
    h = ctypes.addressof(dummy)
    one = (ctypes.c_float * 2)(0.5, 0.5)
    rec = (ctypes.c_ubyte * 112)()
    assert lib.aw_spatializer_set_metering(None, 1) == AW_ERR_INVALID_ARGUMENT
    assert b"NULL" in lib.aw_last_error_message()
    assert lib.aw_spatializer_reset_levels(None) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_get_levels(None, 0, 1, ctypes.addressof(rec)) == AW_ERR_INVALID_ARGUMENT
    for first, n in ((-1, 1), (0, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):      # no stream of a zero-stream handle is in range
        assert lib.aw_spatializer_get_levels(h, first, n, ctypes.addressof(rec)) == AW_ERR_INVALID_ARGUMENT, (first, n)
    assert lib.aw_spatializer_set_gain(None, 0, None, 0, 0.0) == AW_ERR_INVALID_ARGUMENT
    for mode in (3, -1, 1 << 20):
        assert lib.aw_spatializer_set_gain(h, mode, one, 1, 0.5) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_set_gain(h, 1, None, 1, 0.0) == AW_ERR_INVALID_ARGUMENT           # FIXED without gains
    for n in (-1, 2, 7):                                                        # neither 1 nor the (dummy) handle's stream count, 0
        assert lib.aw_spatializer_set_gain(h, 1, one, n, 0.0) == AW_ERR_INVALID_ARGUMENT, n
    for bad in (float("nan"), float("inf"), -float("inf")):
        g = (ctypes.c_float * 1)(bad)
        assert lib.aw_spatializer_set_gain(h, 1, g, 1, 0.0) == AW_ERR_INVALID_ARGUMENT, bad
    for c in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert lib.aw_spatializer_set_gain(h, 2, None, 0, c) == AW_ERR_INVALID_ARGUMENT, c
    assert bytes(dummy) == bytes(4096)
    assert lib.aw_spatializer_info(None, 19) == -1 and lib.aw_spatializer_info(None, 20) == -1


def test_python_wrapper_checks_before_the_library():
    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def f(*a):
                self.calls.append((name, a[1:]))
                return 0
            return f
    sp = object.__new__(aw.Spatializer)
    sp._lib, sp._h, sp.n_streams, sp.n_channels = Recorder(), None, 3, 2
    bad = [(("rms",), {}), ((3,), {}), (("fixed",), {}), (("fixed",), {"gains": [1.0, 2.0]}), (("fixed",), {"gains": [1.0, float("nan"), 1.0]}),
           (("fixed",), {"gains": [float("inf")]}), (("fixed",), {"gains": np.ones((3, 1))}), (("peak_ceiling",), {}),
           (("peak_ceiling",), {"ceiling": 0.0}), (("peak_ceiling",), {"ceiling": 1.5}), (("peak_ceiling",), {"ceiling": float("nan")}),
           (("peak_ceiling",), {"ceiling": -1.0})]
    for a, kw in bad:
        with pytest.raises(ValueError):
            sp.set_gain(*a, **kw)
    for first, n in ((-1, 1), (0, 4), (3, 1)):
        with pytest.raises(ValueError):
            sp.levels(first, n)
    assert sp._lib.calls == []
    sp.set_gain("none")
    sp.set_gain("peak_ceiling", ceiling=0.98)
    sp.set_gain("fixed", gains=0.5)
    sp.set_gain(1, gains=[0.5, 0.25, 1.0])
    sp.set_metering(True)
    sp.set_metering(False)
    sp.reset_levels()
    lv = sp.levels(1, 2)
    calls = sp._lib.calls
    assert [c[0] for c in calls] == ["aw_spatializer_set_gain"] * 4 + ["aw_spatializer_set_metering"] * 2 + ["aw_spatializer_reset_levels",
                                                                                                           "aw_spatializer_get_levels"]
    assert calls[0][1][0] == 0 and calls[0][1][2] == 0
    assert calls[1][1][0] == 2 and abs(calls[1][1][3].value - 0.98) < 1e-7
    assert calls[2][1][0] == 1 and calls[2][1][2] == 1 and calls[3][1][2] == 3
    assert calls[4][1] == (1,) and calls[5][1] == (0,) and calls[7][1][:2] == (1, 2)
    assert lv.dtype == aw.LEVELS_DTYPE and lv.shape == (2,)
    assert {"metering", "gain_mode"} <= set(sp.info())
