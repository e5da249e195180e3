"""TEST-ONLY: ctypes access to the thread-emulated limiter kernel and the sequential rule (tests/emu/emu_limiter.cpp)."""
import ctypes
import os

import numpy as np

import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_limiter.so")
_lib = None
V = ctypes.c_void_p
ONE_BITS = 0x3F800000


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, [(os.path.join(_HERE, "emu_limiter.cpp"), [])], link_flags=["-pthread"])
        i, ll, f = ctypes.c_int, ctypes.c_longlong, ctypes.c_float
        _lib.emu_limiter.argtypes = [V, V, i, ll, V, i, i, f, V, V, V, V, V]
        _lib.emu_limiter_sequential.argtypes = [V, V, i, ll, V, i, i, f, V, V, V, V, V, V]
        _lib.emu_limiter_true_peak.argtypes = [V, ll]
        _lib.emu_limiter_true_peak.restype = ctypes.c_uint32
        _lib.emu_limiter_halo.argtypes = [i, i]
        _lib.emu_limiter_delay.argtypes = [i]
        _lib.emu_limiter_filter.argtypes = [V]
    return _lib


def tile():
    return lib().emu_limiter_tile()


def halo(L, H):
    return lib().emu_limiter_halo(L, H)


def delay(L):
    return lib().emu_limiter_delay(L)


def true_peak(y):
    """awtp::sequential over one stream [frames][2] from silence: the larger ear's true peak as float32."""
    y = np.ascontiguousarray(y, np.float32)
    return np.array([lib().emu_limiter_true_peak(y.ctypes.data, y.shape[0])], np.uint32).view(np.float32)[0]


def _shifted(n_floats, shift):
    raw = np.zeros(n_floats * 4 + 64, np.uint8)
    off = (-raw.ctypes.data) % 16 + 4 * shift
    return raw[off:off + n_floats * 4].view(np.float32)


class Limiter:
    """The carried state of n_streams streams: records and the two history slots.  kernel: the emulated kernel, else the header's
    sequential rule (which also keeps the last call's gains g [streams][frames] and detector bits p)."""

    def __init__(self, n_streams, L, H, ceiling, gains=None, kernel=False):
        self.n, self.L, self.H, self.c, self.kernel = int(n_streams), int(L), int(H), float(ceiling), kernel
        self.gains = None if gains is None else np.ascontiguousarray(gains, np.float32)
        hl = halo(L, H)
        self.min_gain = np.full(self.n, ONE_BITS, np.uint32)
        self.limited = np.zeros(self.n, np.uint64)
        self.nonfinite = np.zeros(self.n, np.uint64)
        self.hist = [np.zeros((self.n, hl, 2), np.float32), np.full((self.n, hl, 2), np.nan, np.float32)]
        self.cur = 0
        self.g = self.p = None

    def process(self, y, shift=0):
        """y: [streams][frames][2] float32, the next frames of every stream; shift: floats past a 16-byte boundary both buffers start
        at.  Returns z of the same shape."""
        y = np.asarray(y, np.float32)
        assert y.shape[0] == self.n and y.shape[2] == 2
        frames = y.shape[1]
        buf, out = _shifted(y.size, shift), _shifted(y.size, shift)
        buf[:] = y.reshape(-1)
        out[:] = np.nan
        gp = None if self.gains is None else self.gains.ctypes.data
        if self.kernel:
            lib().emu_limiter(buf.ctypes.data, out.ctypes.data, self.n, frames, gp, self.L, self.H, self.c, self.hist[self.cur].ctypes.data,
                              self.hist[self.cur ^ 1].ctypes.data, self.min_gain.ctypes.data, self.limited.ctypes.data, self.nonfinite.ctypes.data)
            self.cur ^= 1
        else:
            self.g = np.zeros((self.n, frames), np.float32)
            self.p = np.zeros((self.n, frames), np.uint32)
            lib().emu_limiter_sequential(buf.ctypes.data, out.ctypes.data, self.n, frames, gp, self.L, self.H, self.c,
                                         self.hist[self.cur].ctypes.data, self.min_gain.ctypes.data, self.limited.ctypes.data,
                                         self.nonfinite.ctypes.data, self.g.ctypes.data, self.p.ctypes.data)
        return out.reshape(y.shape).copy()

    def history(self):
        return self.hist[self.cur]

    def records(self):
        return self.min_gain.copy(), self.limited.copy(), self.nonfinite.copy()
