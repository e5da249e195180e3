"""TEST-ONLY: ctypes access to the thread-emulated sample-rate converter kernel and the header's sequential rule
(tests/emu/emu_rateconv.cpp)."""
import ctypes
import os

import numpy as np

import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_rateconv.so")
_lib = None
V = ctypes.c_void_p
_D, _I, _LL = ctypes.c_double, ctypes.c_int, ctypes.c_longlong


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, [(os.path.join(_HERE, "emu_rateconv.cpp"), [])], link_flags=["-pthread"])
        _lib.emu_rateconv_plan.argtypes = [_D, _D, V]
        _lib.emu_rateconv_filter.argtypes = [_D, _D, V]
        _lib.emu_rateconv_tile.argtypes = [_D, _D, _I]
        _lib.emu_rateconv.argtypes = [_D, _D, _I, V, _I, _LL, V, V, V, V, V]
        _lib.emu_rateconv.restype = _LL
        _lib.emu_rateconv_sequential.argtypes = [_D, _D, _I, V, _I, _LL, V, V, V]
        _lib.emu_rateconv_sequential.restype = _LL
    return _lib


def plan(in_rate, out_rate):
    """(L, M, taps, latency) of the header's plan, or None where it refuses."""
    o = np.zeros(4, np.int32)
    return None if lib().emu_rateconv_plan(in_rate, out_rate, o.ctypes.data) else tuple(int(v) for v in o)


def filter_table(in_rate, out_rate):
    L, _, T, _ = plan(in_rate, out_rate)
    c = np.zeros((L, T), np.float32)
    assert lib().emu_rateconv_filter(in_rate, out_rate, c.ctypes.data) == 0
    return c


def tile(in_rate, out_rate, channels):
    return lib().emu_rateconv_tile(in_rate, out_rate, channels)


def lds_floats():
    return lib().emu_rateconv_lds_floats()


def input_frames_for(n_out, L, M, D):
    """The fewest input frames after which n_out outputs exist: floor((n_out - 1) M / L) + D + 1."""
    return (n_out - 1) * M // L + D + 1 if n_out > 0 else 0


def shifted(a, shift):
    """A copy of the float32 array `a`, flat, that starts `shift` floats past a 16-byte boundary, behind and in front of NaNs."""
    raw = np.full(a.size + 16, np.nan, np.float32)
    off = ((-raw.ctypes.data) % 16) // 4 + shift
    buf = raw[off:off + a.size]
    buf[:] = np.asarray(a, np.float32).reshape(-1)
    return buf


class Converter:
    """The carried state of n_streams streams: the two history slots and the counts.  kernel: the emulated kernel, else the header's
    sequential rule."""

    def __init__(self, in_rate, out_rate, n_streams, channels, kernel):
        self.rates, self.n, self.C, self.kernel = (float(in_rate), float(out_rate)), int(n_streams), int(channels), kernel
        self.L, self.M, self.T, self.D = plan(in_rate, out_rate)
        self.hist = [np.zeros((self.n, self.T - 1, self.C), np.float32), np.full((self.n, self.T - 1, self.C), np.nan, np.float32)]
        self.cur = 0
        self.counts = np.zeros(2, np.int64)
        self.dev_counts = np.zeros((self.n, 2), np.int64)

    def output_frames(self, in_frames):
        N = int(self.counts[0]) + in_frames
        return max(0, -((N - self.D) * self.L // -self.M)) - int(self.counts[1])

    def process(self, x, shift=0, out_shift=0):
        """x: [streams][frames][channels] float32, the next frames of every stream; shift, out_shift: floats past a 16-byte boundary the
        input and the output start at.  Returns [streams][produced][channels]."""
        x = np.asarray(x, np.float32)
        assert x.shape[0] == self.n and x.shape[2] == self.C and x.shape[1] > 0
        buf = shifted(x, shift)
        return self._run(buf.ctypes.data, x.shape[1], out_shift, keep=buf)

    def _run(self, in_ptr, frames, out_shift=0, keep=None):
        n_out = self.output_frames(frames)
        out = shifted(np.full((self.n, max(n_out, 0), self.C), np.nan, np.float32), out_shift)
        if self.kernel:
            made = lib().emu_rateconv(*self.rates, self.C, in_ptr, self.n, frames, self.hist[self.cur].ctypes.data,
                                      self.hist[self.cur ^ 1].ctypes.data, self.counts.ctypes.data, self.dev_counts.ctypes.data, out.ctypes.data)
            self.cur ^= 1
        else:
            made = lib().emu_rateconv_sequential(*self.rates, self.C, in_ptr, self.n, frames, self.hist[self.cur].ctypes.data,
                                                 self.counts.ctypes.data, out.ctypes.data)
            self.dev_counts[:] = self.counts
        assert made == n_out, (made, n_out)
        del keep
        base = out.base                                # (out is a view into a larger NaN buffer: anything written beside it shows there)
        lo = (out.ctypes.data - base.ctypes.data) // 4
        assert np.isnan(base[:lo]).all() and np.isnan(base[lo + out.size:]).all(), "wrote outside the output"
        return out.reshape(self.n, n_out, self.C).copy()

    def flush(self):
        """process of D zero frames, then reset."""
        y = self._run(None, self.D)
        self.reset()
        return y

    def reset(self):
        self.hist[self.cur][:] = 0
        self.counts[:] = 0
        self.dev_counts[:] = 0

    def history(self):
        return self.hist[self.cur]
