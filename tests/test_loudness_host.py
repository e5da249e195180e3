"""CPU-side checks of the per-stream integrated loudness (include/airwave_hip.h: aw_stream_loudness, aw_spatializer_set_loudness /
_get_loudness / _get_loudness_hops, aw_loudness_gain): the rules of airwave_amd/csrc/device/loudness.hpp, compiled by plain g++ into a
test-only library, against the numpy restatement of loudness_ref.py; the struct and the entry points of the C header against Python's;
and the argument checks, which run before any HIP call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import airwave_amd as aw
from airwave_amd import _capi
import loudness_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "airwave_amd", "csrc", "device")
HEADER = os.path.join(ROOT, "include", "airwave_hip.h")
AW_OK, AW_ERR_INVALID_ARGUMENT = 0, 1
NEW_ENTRIES = ("aw_spatializer_set_loudness", "aw_spatializer_get_loudness", "aw_spatializer_get_loudness_hops", "aw_loudness_gain")
FIELDS = ["integrated_lufs", "relative_threshold_lufs", "blocks", "blocks_above_absolute", "blocks_gated", "reserved", "frames",
          "frames_dropped", "nonfinite"]

SHIM = r"""
#include <cstddef>
#include "loudness.hpp"
#include "../../../include/airwave_hip.h"
extern "C" {
void coefficients(double fs, double *c) {
    double k[awlo::kFilters][5];
    awlo::k_weighting(fs, k);
    for (int f = 0; f < awlo::kFilters; ++f) for (int i = 0; i < 5; ++i) c[f * 5 + i] = k[f][i];
}
long long hop_frames(double fs) { return awlo::hop_frames(fs); }
void gate(const double *e, long long n_hops, long long hop, double *lufs, unsigned *counts) {
    const awlo::Gated g = awlo::gate(e, n_hops, hop);
    lufs[0] = g.integrated_lufs; lufs[1] = g.relative_threshold_lufs;
    counts[0] = g.blocks; counts[1] = g.blocks_above_absolute; counts[2] = g.blocks_gated;
}
void filter_input(const float *y, long n, double *v, unsigned *nonfinite) { for (long i = 0; i < n; ++i) v[i] = awlo::filter_input(y[i], *nonfinite); }
int gain_to_target(double lufs, double target, float *g) { return awlo::gain_to_target(lufs, target, g) ? 1 : 0; }
void layout(long *o) {
    o[0] = sizeof(aw_stream_loudness); o[1] = offsetof(aw_stream_loudness, integrated_lufs); o[2] = offsetof(aw_stream_loudness, relative_threshold_lufs);
    o[3] = offsetof(aw_stream_loudness, blocks); o[4] = offsetof(aw_stream_loudness, blocks_above_absolute); o[5] = offsetof(aw_stream_loudness, blocks_gated);
    o[6] = offsetof(aw_stream_loudness, reserved); o[7] = offsetof(aw_stream_loudness, frames); o[8] = offsetof(aw_stream_loudness, frames_dropped);
    o[9] = offsetof(aw_stream_loudness, nonfinite);
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("loudness_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libloudness_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + DEVICE, str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.coefficients.argtypes = [ctypes.c_double, ctypes.c_void_p]
    lib.hop_frames.argtypes = [ctypes.c_double]
    lib.hop_frames.restype = ctypes.c_longlong
    lib.gate.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    lib.filter_input.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    lib.gain_to_target.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    lib.layout.argtypes = [ctypes.c_void_p]
    return lib


def shim_coefficients(lib, fs):
    c = np.zeros((2, 5))
    lib.coefficients(float(fs), c.ctypes.data)
    return c


def test_coefficients_at_48k_are_the_bs1770_table(shim):
    c = shim_coefficients(shim, 48000.0)
    got = np.column_stack([c[:, :3], np.ones(2), c[:, 3:]])          # b0 b1 b2 a0 a1 a2: the twelve table values
    err = np.max(np.abs(got - ref.BS1770_TABLE))
    print(f"largest difference from the BS.1770-4 table: {err:.2e}")
    assert got.shape == (2, 6) and err <= 1e-13


@pytest.mark.parametrize("fs", [44100.0, 96000.0, 48000.0, 32000.0, 192000.0])
def test_coefficients_at_other_rates_match_the_formulas(shim, fs):
    want = ref.k_coefficients(fs)[:, [0, 1, 2, 4, 5]]
    assert np.max(np.abs(shim_coefficients(shim, fs) - want)) <= 1e-13


def test_hop_is_a_tenth_of_a_rate_that_has_one(shim):
    for fs, hop in ((48000.0, 4800), (44100.0, 4410), (96000.0, 9600), (22050.0, 2205), (10.0, 1), (11025.0, 0), (44100.5, 0), (0.0, 0), (-48000.0, 0),
                    (float("nan"), 0), (float("inf"), 0), (48005.0, 0)):
        assert shim.hop_frames(fs) == hop, fs


def shim_gate(lib, e, hop):
    e = np.ascontiguousarray(e, np.float64)
    lufs, counts = np.zeros(2), np.zeros(3, np.uint32)
    lib.gate(e.ctypes.data, e.size, hop, lufs.ctypes.data, counts.ctypes.data)
    return lufs, counts.tolist()


def test_gating_matches_numpy(shim):
    rng = np.random.default_rng(5)
    hop = 4800
    full = 4.0 * hop * 10 ** ((-23.0 + 0.691) / 10)                  # four hops' energy of a -23 LUFS block, per hop: / 4
    cases = [np.zeros(0), np.ones(1), np.ones(3) * full, np.zeros(12),                              # fewer than 4 hops; silence
             np.full(40, 1e-9 * full),                                                             # every block below the absolute gate
             np.full(4, full / 4), np.full(50, full / 4)]
    for _ in range(40):                                                                             # loud and quiet stretches, random lengths
        parts = [np.full(rng.integers(1, 30), full / 4 * 10 ** (rng.uniform(-8, 1))) * rng.uniform(0.5, 2.0, 1) for _ in range(rng.integers(1, 8))]
        cases.append(np.concatenate(parts) * rng.uniform(0.9, 1.1, sum(p.size for p in parts)))
    cases.append(np.concatenate([np.full(30, full / 4), np.full(30, full / 4 * 1e-3), np.zeros(20)]))      # relative gate only, then digital silence
    seen = {"none": 0, "relative": 0, "short": 0}
    for e in cases:
        want = ref.gate(e, hop)
        lufs, counts = shim_gate(shim, e, hop)
        assert counts == [want["blocks"], want["above_absolute"], want["gated"]], e
        for got, w in zip(lufs, (want["integrated"], want["relative_threshold"])):
            assert (got == w == -np.inf) if np.isinf(w) else abs(got - w) <= 1e-12, (got, w)
        seen["none"] += want["gated"] == 0 and e.size >= 4
        seen["relative"] += 0 < want["gated"] < want["above_absolute"]
        seen["short"] += e.size < 4 and counts == [0, 0, 0]
    assert seen["none"] >= 2 and seen["relative"] >= 5 and seen["short"] == 3
    lufs, counts = shim_gate(shim, np.full(50, full / 4), hop)
    assert abs(lufs[0] + 23.0) < 1e-12 and abs(lufs[1] + 33.0) < 1e-12 and counts == [47, 47, 47]


def test_the_fast_reference_is_the_recurrence(shim):
    """loudness_ref.k_weight (scipy's lfilter, used where a GPU test measures minutes of signal to +-0.1 LU) is the frame-by-frame loop
    up to its own rounding: two Float64 evaluations of the 38 Hz section, whose double pole sits next to z = 1, drift apart by some
    1e-13 of the peak.  The tests that hold hop energies to the reassociation bound use the loop itself."""
    rng = np.random.default_rng(6)
    for fs in (44100, 48000, 96000):
        y = rng.uniform(-1, 1, (2, 6000))
        slow, _ = ref.k_weight_loop(y, fs)
        assert np.max(np.abs(ref.k_weight(y, fs) - slow)) <= 1e-11 * np.max(np.abs(slow))


def test_a_nonfinite_sample_enters_as_zero(shim):
    y = np.array([0.5, np.nan, -np.inf, np.inf, -0.0, 1e-45, -3.4e38], np.float32)
    v, nf = np.zeros(y.size), ctypes.c_uint(0)
    shim.filter_input(y.ctypes.data, y.size, v.ctypes.data, ctypes.addressof(nf))
    want, bad = ref.sanitize(y)
    assert np.array_equal(v, want) and nf.value == bad == 3


def test_struct_layout_matches_python(shim):
    o = (ctypes.c_long * 10)()
    shim.layout(ctypes.addressof(o))
    assert o[0] == 56 == ctypes.sizeof(_capi.StreamLoudness) == aw.LOUDNESS_DTYPE.itemsize
    assert list(o[1:10]) == [getattr(_capi.StreamLoudness, f).offset for f in FIELDS] == [aw.LOUDNESS_DTYPE.fields[f][1] for f in FIELDS]
    assert list(aw.LOUDNESS_DTYPE.names) == FIELDS == [f for f, _ in _capi.StreamLoudness._fields_]
    text = open(HEADER).read()
    body = re.search(r"typedef struct aw_stream_loudness \{(.*?)\} aw_stream_loudness;", text, re.S).group(1)
    assert re.findall(r"\b(?:double|uint32_t|uint64_t)\s+(\w+);", body) == FIELDS
    assert "are not provided" in text and "Integrated loudness in LUFS" in text


def test_new_entries_are_declared_exported_and_typed():
    text = open(HEADER).read()
    declared = set(re.findall(r"AW_API\s+[\w\s\*]+?\b(aw_\w+)\s*\(", text))
    lib = _capi.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert declared == set(_capi.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(NEW_ENTRIES) <= exported


def test_argument_checks_come_before_any_hip_call():
    lib = _capi.load()
    dummy = (ctypes.c_ubyte * 8192)()                              # a non-NULL handle of zero streams and rate 0 that the failing checks never write
    h = ctypes.addressof(dummy)
    rec = (ctypes.c_ubyte * 112)()
    buf = (ctypes.c_double * 4)()
    assert lib.aw_spatializer_set_loudness(None, 1, 10.0) == AW_ERR_INVALID_ARGUMENT
    assert b"NULL" in lib.aw_last_error_message()
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert lib.aw_spatializer_set_loudness(h, 1, bad) == AW_ERR_INVALID_ARGUMENT, bad
        assert b"max_seconds" in lib.aw_last_error_message()
    assert lib.aw_spatializer_set_loudness(h, 1, 10.0) == AW_ERR_INVALID_ARGUMENT       # the dummy's rate, 0, is no multiple of 10 Hz
    assert b"10 Hz" in lib.aw_last_error_message()
    assert lib.aw_spatializer_set_loudness(h, 0, float("nan")) == AW_OK                   # off: max_seconds is not looked at, nothing to allocate
    assert lib.aw_spatializer_get_loudness(None, 0, 1, ctypes.addressof(rec)) == AW_ERR_INVALID_ARGUMENT
    for first, n in ((-1, 1), (0, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.aw_spatializer_get_loudness(h, first, n, ctypes.addressof(rec)) == AW_ERR_INVALID_ARGUMENT, (first, n)
    assert lib.aw_spatializer_get_loudness_hops(None, 0, 0, 1, ctypes.addressof(buf)) == AW_ERR_INVALID_ARGUMENT
    for stream, first, n in ((0, 0, 1), (-1, 0, 1), (1, 0, 0)):
        assert lib.aw_spatializer_get_loudness_hops(h, stream, first, n, ctypes.addressof(buf)) == AW_ERR_INVALID_ARGUMENT, (stream, first, n)
    assert bytes(dummy) == bytes(8192)
    assert lib.aw_spatializer_info(None, 21) == -1
    g = ctypes.c_float(7.0)
    assert lib.aw_loudness_gain(-23.0, -16.0, None) == AW_ERR_INVALID_ARGUMENT
    for lufs, target in ((-float("inf"), -16.0), (float("nan"), -16.0), (float("inf"), -16.0), (-23.0, float("nan")), (-23.0, float("inf")),
                         (-1000.0, 0.0)):
        assert lib.aw_loudness_gain(lufs, target, ctypes.byref(g)) == AW_ERR_INVALID_ARGUMENT and g.value == 7.0, (lufs, target)
    assert lib.aw_loudness_gain(-23.0, -16.0, ctypes.byref(g)) == AW_OK
    assert g.value == float(np.float32(10.0 ** (7.0 / 20.0)))
    assert lib.aw_loudness_gain(-16.0, -23.0, ctypes.byref(g)) == AW_OK and g.value == float(np.float32(10.0 ** (-7.0 / 20.0)))


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
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sp.set_loudness(True, bad)
    for first, n in ((-1, 1), (0, 4), (3, 1)):
        with pytest.raises(ValueError):
            sp.loudness(first, n)
    for a in ((-1, 0, 1), (3, 0, 1), (0, -1, 1), (0, 0, -1)):
        with pytest.raises(ValueError):
            sp.loudness_hops(*a)
    for a in ((-np.inf, -16.0), (np.nan, -16.0), (-23.0, np.inf)):
        with pytest.raises(ValueError):
            aw.loudness_gain(*a)
    assert sp._lib.calls == []
    sp.set_loudness(True, 12.5)
    sp.set_loudness(False)
    ld = sp.loudness(1, 2)
    hops = sp.loudness_hops(2, 5, 7)
    calls = sp._lib.calls
    assert [c[0] for c in calls] == ["aw_spatializer_set_loudness"] * 2 + ["aw_spatializer_get_loudness", "aw_spatializer_get_loudness_hops"]
    assert calls[0][1] == (1, 12.5) and calls[1][1][0] == 0 and calls[2][1][:2] == (1, 2) and calls[3][1][:3] == (2, 5, 7)
    assert ld.dtype == aw.LOUDNESS_DTYPE and ld.shape == (2,) and hops.dtype == np.float64 and hops.shape == (7,)
    assert "loudness" in sp.info()
    assert abs(aw.loudness_gain(-23.0, -16.0) - 10 ** 0.35) < 1e-6
