"""TEST-ONLY: ctypes access to the thread-emulated true-peak kernel (tests/emu/emu_true_peak.cpp)."""
import ctypes
import os

import numpy as np

import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_true_peak.so")
_lib = None
V = ctypes.c_void_p


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, [(os.path.join(_HERE, "emu_true_peak.cpp"), [])], link_flags=["-pthread"])
        _lib.emu_true_peak.argtypes = [V, ctypes.c_int, ctypes.c_longlong, V, V, V, V, V]
        _lib.emu_true_peak_sequential.argtypes = [V, ctypes.c_int, ctypes.c_longlong, V, V, V, V]
        _lib.emu_true_peak_filter.argtypes = [V]
    return _lib


def tile():
    return lib().emu_true_peak_tile()


class Meter:
    """The carried state of n_streams streams: peaks, counts, the two history slots.  kernel: the emulated kernel, else the header's
    sequential rule."""

    def __init__(self, n_streams, kernel, records=True):
        self.n, self.kernel, self.records = int(n_streams), kernel, records
        self.tp = np.zeros((self.n, 2), np.uint32)
        self.nonfinite = np.zeros(self.n, np.uint64)
        self.call = np.zeros(self.n, np.uint32)
        self.hist = [np.zeros((self.n, 11, 2), np.float32), np.full((self.n, 11, 2), np.nan, np.float32)]
        self.cur = 0

    def process(self, y, shift=0):
        """y: [streams][frames][2] float32, the next frames of every stream; shift: floats past a 16-byte boundary the buffer starts at."""
        y = np.asarray(y, np.float32)
        assert y.shape[0] == self.n and y.shape[2] == 2
        raw = np.zeros(y.size * 4 + 64, np.uint8)
        off = (-raw.ctypes.data) % 16 + 4 * shift
        buf = raw[off:off + y.size * 4].view(np.float32)
        buf[:] = y.reshape(-1)
        self.call[:] = 0
        if self.kernel:
            lib().emu_true_peak(buf.ctypes.data, self.n, y.shape[1], self.hist[self.cur].ctypes.data, self.hist[self.cur ^ 1].ctypes.data,
                                self.tp.ctypes.data if self.records else None, self.nonfinite.ctypes.data, self.call.ctypes.data)
            self.cur ^= 1
        else:
            lib().emu_true_peak_sequential(buf.ctypes.data, self.n, y.shape[1], self.hist[self.cur].ctypes.data, self.tp.ctypes.data,
                                           self.nonfinite.ctypes.data, self.call.ctypes.data)

    def history(self):
        return self.hist[self.cur]
