"""TEST-ONLY: ctypes access to the thread-emulated equalizer stage (tests/emu/emu_eq_stage.cpp)."""
import ctypes
import os

import numpy as np

import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB = os.path.join(_HERE, "libemu_eq_stage.so")
_UNITS = [(os.path.join(_HERE, "emu_eq_stage.cpp"), []), (os.path.join(_ROOT, "airwave_amd/csrc/host/eq.cpp"), [])]
_lib = None
dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int32)


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, _UNITS, link_flags=["-pthread"])
        _lib.emu_eq_stage.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ip, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, dp, ip, dp,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_int]
        _lib.emu_eq_plain.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_double, dp,
                                      ctypes.c_int, ctypes.c_int]
    return _lib


def _filters(filters):
    return np.ascontiguousarray(np.asarray(filters, dtype=np.float64).reshape(-1, 4))


class Stage:
    """n_streams streams, each through the preset its map entry names (-1: none).  presets: [(preamp_db, [(type, fc, gain_db, q)])]."""

    def __init__(self, presets, stream_map, sample_rate, ear_split=False):
        self.rate, self.ear_split = float(sample_rate), bool(ear_split)
        self.map = np.ascontiguousarray(stream_map, dtype=np.int32)
        self.preamps = np.ascontiguousarray([p for p, _ in presets], dtype=np.float64)
        self.counts = np.ascontiguousarray([len(f) for _, f in presets], dtype=np.int32)
        self.filters = _filters([f for _, fl in presets for f in fl])
        self.kmax = int(self.counts.max())
        self.z = np.zeros((self.map.size, self.kmax, 4), np.float64)

    def process(self, x):
        """x: [streams][frames][2] float32, the next frames of every stream -> the same shape."""
        y = np.array(x, dtype=np.float32, order="C")
        assert y.shape[0] == self.map.size and y.shape[2] == 2
        rc = lib().emu_eq_stage(y.ctypes.data, self.z.ctypes.data, self.map.ctypes.data_as(ip), y.shape[0], y.shape[1], self.rate,
                                self.preamps.ctypes.data_as(dp), self.counts.ctypes.data_as(ip), self.filters.ctypes.data_as(dp), self.counts.size,
                                self.kmax, int(self.ear_split))
        assert rc == 0, rc
        return y


class Plain:
    """One preset over every stream: the emulated eq_cascade_stream + eq_sequential on the dense state."""

    def __init__(self, preamp_db, filters, n_streams, sample_rate, ear_split=False):
        self.rate, self.ear_split, self.preamp = float(sample_rate), bool(ear_split), float(preamp_db)
        self.filters = _filters(filters)
        self.z = np.zeros((n_streams, max(len(self.filters), 1), 4), np.float64)

    def process(self, x):
        y = np.array(x, dtype=np.float32, order="C")
        rc = lib().emu_eq_plain(y.ctypes.data, self.z.ctypes.data, y.shape[0], y.shape[1], self.rate, self.preamp, self.filters.ctypes.data_as(dp),
                                len(self.filters), int(self.ear_split))
        assert rc == len(self.filters), rc
        return y
