"""TEST-ONLY: ctypes access to the thread-emulated loudness kernels (tests/emu/emu_loudness.cpp)."""
import ctypes
import os

import numpy as np

import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB = os.path.join(_HERE, "libemu_loudness.so")
_UNITS = [(os.path.join(_HERE, "emu_loudness.cpp"), []), (os.path.join(_ROOT, "airwave_amd/csrc/host/eq.cpp"), [])]
_lib = None
dp = ctypes.POINTER(ctypes.c_double)


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, _UNITS, link_flags=["-pthread"])
        _lib.emu_loudness.restype = ctypes.c_longlong
        _lib.emu_loudness.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_longlong, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
        _lib.emu_loudness_tables.argtypes = [ctypes.c_double, dp, dp, dp]
    return _lib


class Meter:
    """The carried state of n_streams streams: filter state, hop energies, non-finite counts, frames so far."""

    def __init__(self, n_streams, rate, cap_hops):
        self.rate, self.n = float(rate), int(n_streams)
        self.z = np.zeros((self.n, 2, 4), np.float64)
        self.hops = np.zeros((self.n, int(cap_hops)), np.float64)
        self.nonfinite = np.zeros(self.n, np.uint64)
        self.frames = 0
        self.hop = 0

    def process(self, y):
        """y: [streams][frames][2] float32, the next frames of every stream."""
        y = np.ascontiguousarray(y, np.float32)
        assert y.shape[0] == self.n and y.shape[2] == 2
        self.hop = lib().emu_loudness(y.ctypes.data, self.n, y.shape[1], self.rate, self.frames, self.z.ctypes.data, self.hops.ctypes.data,
                                      self.hops.shape[1], self.nonfinite.ctypes.data)
        assert self.hop > 0
        self.frames += y.shape[1]


def tables(rate):
    """(coef [2][5], tab [2][tab_doubles], plane [2][64][4]) of the two K-weighting sections at a rate."""
    coef, tab, plane = np.zeros((2, 5)), np.zeros((2, 512)), np.zeros((2, 64, 4))
    td = lib().emu_loudness_tables(float(rate), coef.ctypes.data_as(dp), tab.ctypes.data_as(dp), plane.ctypes.data_as(dp))
    return coef, tab.reshape(-1)[: 2 * td].reshape(2, td), plane
