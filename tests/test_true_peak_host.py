"""CPU-side checks of the per-stream true peak (include/airwave_hip.h: aw_stream_true_peak, aw_spatializer_set_true_peak /
_get_true_peak, aw_true_peak_filter): the rules of airwave_amd/csrc/device/truepeak.hpp, compiled by plain g++ into a test-only library,
against the numpy restatement of true_peak_ref.py; the struct of the C header against Python's; and the argument checks, which run
before any HIP call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import airwave_amd as aw
from airwave_amd import _capi
import true_peak_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "airwave_amd", "csrc", "device")
AW_OK, AW_ERR_INVALID_ARGUMENT = 0, 1
FIELDS = ["true_peak", "call_true_peak", "reserved", "frames", "nonfinite"]

SHIM = r"""
#include <cstddef>
#include "truepeak.hpp"
#include "../../../include/airwave_hip.h"
extern "C" {
void filter(float *c) { float f[awtp::kCoefficients]; awtp::filter(f); for (int i = 0; i < awtp::kCoefficients; ++i) c[i] = f[i]; }
// y [frames][2], hist [11][2] carried, rec: tp_bits[2], call_tp_bits, nonfinite (as 4 x uint64) carried
void sequential(const float *y, long long frames, float *hist, unsigned long long *rec) {
    float c[awtp::kCoefficients];
    awtp::filter(c);
    awtp::Record r{{(uint32_t)rec[0], (uint32_t)rec[1]}, (uint32_t)rec[2], rec[3]};
    awtp::sequential(c, y, frames, hist, r);
    rec[0] = r.tp_bits[0]; rec[1] = r.tp_bits[1]; rec[2] = r.call_tp_bits; rec[3] = r.nonfinite;
}
void layout(long *o) {
    o[0] = sizeof(aw_stream_true_peak); o[1] = offsetof(aw_stream_true_peak, true_peak); o[2] = offsetof(aw_stream_true_peak, call_true_peak);
    o[3] = offsetof(aw_stream_true_peak, reserved); o[4] = offsetof(aw_stream_true_peak, frames); o[5] = offsetof(aw_stream_true_peak, nonfinite);
    o[6] = AW_GAIN_TRUE_PEAK_CEILING;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("true_peak_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libtrue_peak_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + DEVICE, str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.filter.argtypes = [ctypes.c_void_p]
    lib.sequential.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    lib.layout.argtypes = [ctypes.c_void_p]
    return lib


class Stream:
    """One stream's carried state under the header's sequential rule."""

    def __init__(self, lib):
        self.lib, self.hist, self.rec = lib, np.zeros((11, 2), np.float32), np.zeros(4, np.uint64)

    def process(self, y):
        y = np.ascontiguousarray(y, np.float32)
        self.rec[2] = 0
        self.lib.sequential(y.ctypes.data, y.shape[0], self.hist.ctypes.data, self.rec.ctypes.data)

    def peaks(self):
        return self.rec[:2].astype(np.uint32).view(np.float32).astype(np.float64)

    def call_peak(self):
        return float(self.rec[2:3].astype(np.uint32).view(np.float32)[0])


def shim_filter(lib):
    c = np.zeros(36, np.float32)
    lib.filter(c.ctypes.data)
    return c.reshape(3, 12)


def test_coefficients_are_the_formula_rounded_once(shim):
    c, want = shim_filter(shim), ref.coefficients()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(c.astype(np.float64) - want.astype(np.float32).astype(np.float64))
    print(f"coefficients: largest difference from the rounded formula {float(np.max(err / ulp)):.1f} ulp")
    assert np.all(err <= ulp)                                          # 1 float32 ulp for libm
    assert np.array_equal(c, aw.true_peak_filter())
    h = ref.prototype()
    assert np.max(np.abs(h[0::4] - (np.arange(13) == 6))) <= 1e-15     # phase 0 is the identity: never computed
    assert np.allclose(c.sum(axis=1), 1.0, atol=2e-3)                  # every phase passes DC


@pytest.mark.parametrize("frames", [1, 11, 12, 13, 4097])
def test_sequential_rule_matches_numpy_within_the_bound(shim, frames):
    y = np.random.default_rng(frames).uniform(-1.0, 1.0, (frames, 2)).astype(np.float32)
    s = Stream(shim)
    s.process(y)
    want = ref.measure(y, shim_filter(shim))
    err = np.abs(s.peaks() - want["peak"])
    print(f"{frames} frames: true peak {s.peaks()} reference {want['peak']} difference {err} bound {want['bound']}")
    assert np.all(err <= want["bound"]) and s.rec[3] == 0
    assert s.call_peak() == s.peaks().max()
    assert np.all(s.peaks() >= np.abs(y).max(axis=0))
    assert np.array_equal(s.hist.astype(np.float64), want["hist"])


def test_splitting_calls_in_time_changes_no_bit(shim):
    y = np.random.default_rng(7).uniform(-1.0, 1.0, (4097, 2)).astype(np.float32)
    one, split = Stream(shim), Stream(shim)
    one.process(y)
    at = 0
    for n in (1, 10, 1, 4085):
        split.process(y[at:at + n])
        at += n
    assert at == 4097
    assert np.array_equal(one.rec[:2], split.rec[:2]) and np.array_equal(one.hist, split.hist)
    # the last call's own peak is that of its frames behind their true predecessors
    want = ref.measure(y[12:], shim_filter(shim), hist=y[1:12])
    assert abs(split.call_peak() - want["peak"].max()) <= want["bound"].max()


def test_nonfinite_samples_enter_as_zero_and_are_counted(shim):
    y = np.random.default_rng(8).uniform(-1.0, 1.0, (64, 2)).astype(np.float32)
    bad = y.copy()
    bad[5, 0], bad[20, 1], bad[63, 0] = np.nan, np.inf, -np.inf
    clean = np.where(np.isfinite(bad), bad, np.float32(0))
    a, b = Stream(shim), Stream(shim)
    a.process(bad)
    b.process(clean)
    assert a.rec[3] == 3 and b.rec[3] == 0
    assert np.array_equal(a.rec[:3], b.rec[:3]) and np.array_equal(a.hist, b.hist) and np.isfinite(a.peaks()).all()


def test_known_sines_read_their_amplitude(shim):
    """The reference alone, and the sequential rule: EBU Tech 3341's +0.2 / -0.4 dB around the amplitude of a sinusoid."""
    c = shim_filter(shim)
    for rate in (44100, 48000, 96000):
        for div, phase, amp in ((4, 0.0, 0.5), (4, 45.0, 0.5), (6, 60.0, 0.5), (8, 67.5, 0.5), (4, 45.0, 1.41)):
            y = ref.faded_sine(rate, rate / div, phase, amp)
            want = ref.measure(y, c)
            s = Stream(shim)
            s.process(y)
            d = ref.db(want["peak"][0]) - ref.db(amp)
            print(f"{rate} Hz fs/{div} at {phase} deg, amplitude {amp}: {ref.db(want['peak'][0]):.3f} dBTP ({d:+.3f}), sample peak {ref.db(np.abs(y).max()):.3f}")
            assert -0.4 <= d <= 0.2
            assert np.all(np.abs(s.peaks() - want["peak"]) <= want["bound"])


def test_struct_layout_matches_python(shim):
    o = (ctypes.c_long * 7)()
    shim.layout(ctypes.addressof(o))
    assert o[0] == 32 == ctypes.sizeof(_capi.StreamTruePeak) == aw.TRUE_PEAK_DTYPE.itemsize
    assert list(o[1:6]) == [getattr(_capi.StreamTruePeak, f).offset for f in FIELDS] == [aw.TRUE_PEAK_DTYPE.fields[f][1] for f in FIELDS]
    assert list(aw.TRUE_PEAK_DTYPE.names) == FIELDS == [f for f, _ in _capi.StreamTruePeak._fields_]
    assert o[6] == 3 == aw.GAIN_MODES["true_peak_ceiling"]


def test_argument_errors_come_before_any_hip_call():
    lib = _capi.load()
    out = np.zeros(1, aw.TRUE_PEAK_DTYPE)
    assert lib.aw_spatializer_set_true_peak(None, 1) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_get_true_peak(None, 0, 1, ctypes.c_void_p(out.ctypes.data)) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_true_peak_filter(None) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_set_gain(None, 3, None, 0, ctypes.c_float(0.5)) == AW_ERR_INVALID_ARGUMENT
    dummy = (ctypes.c_ubyte * 4096)()                              # a non-NULL handle of zero streams: nothing to measure or gain
    h = ctypes.addressof(dummy)
    assert lib.aw_spatializer_set_gain(h, 3, None, 0, ctypes.c_float(0.5)) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_set_true_peak(h, 1) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_spatializer_get_true_peak(h, 0, 1, ctypes.c_void_p(out.ctypes.data)) == AW_ERR_INVALID_ARGUMENT
    assert bytes(dummy) == bytes(4096)
