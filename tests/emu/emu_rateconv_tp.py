"""TEST-ONLY: ctypes access to the measuring forms of the sample-rate converter's kernel on emulated workgroups and to the true-peak rule
alone (tests/emu/emu_rateconv_tp.cpp).  The reference is the COMPOSITION: emu_rateconv_pcm's composition (awp::decode_at, awrc::sequential,
gain, encode) for the bytes, the levels and the float32 outputs y, then awrc::true_peak_sequential over y, element by element."""
import ctypes
import os

import numpy as np

import _build
import emu_rateconv as emu
import emu_rateconv_pcm as pcm
from emu_rateconv_pcm import BYTES, F32, NONE, SENTINEL, Settings, shifted_bytes

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_rateconv_tp.so")
_lib = None
V = ctypes.c_void_p
_D, _I, _LL = ctypes.c_double, ctypes.c_int, ctypes.c_longlong

HISTORY = 11
TRUE_PEAK = np.dtype([("true_peak", np.float32), ("sample_peak", np.float32), ("frames", np.uint64)])
assert TRUE_PEAK.itemsize == 16


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, [(os.path.join(_HERE, "emu_rateconv_tp.cpp"), [])], link_flags=["-pthread"])
        _lib.emu_rateconv_tp_tiles.argtypes = [_I, _I, _I, _I, V, V]
        _lib.emu_rateconv_tp_filter.argtypes = [V]
        _lib.emu_rateconv_tp_ceiling_gain.argtypes = [ctypes.c_float, ctypes.c_float]
        _lib.emu_rateconv_tp_ceiling_gain.restype = ctypes.c_float
        _lib.emu_rateconv_tp.argtypes = [_D, _D, _I, V, _I, _LL, V, V, V, V, V, V, V, V, V, _I]
        _lib.emu_rateconv_tp.restype = _LL
        _lib.emu_rateconv_tp_rule.argtypes = [V, _I, _LL, _I, V, V]
        _lib.emu_rateconv_tp_rule.restype = None
    return _lib


def tiles(L, M, T, channels):
    """(rc_tile, rc_tp_tile) of (L, M, T, channels)."""
    a, b = ctypes.c_int(), ctypes.c_int()
    lib().emu_rateconv_tp_tiles(L, M, T, channels, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def tp_tile(in_rate, out_rate, channels):
    L, M, T, _ = emu.plan(in_rate, out_rate)
    return tiles(L, M, T, channels)[1]


def filter36():
    c = np.zeros(36, np.float32)
    lib().emu_rateconv_tp_filter(c.ctypes.data)
    return c


def ceiling_gain(tp, c):
    return np.float32(lib().emu_rateconv_tp_ceiling_gain(float(tp), float(c)))


def rule(y, hist, records):
    """awrc::true_peak_sequential over y [streams][frames][channels]; hist [streams][11][channels] and records are updated in place."""
    y = np.ascontiguousarray(y, np.float32)
    assert hist.dtype == np.float32 and hist.shape == (y.shape[0], HISTORY, y.shape[2]) and records.dtype == TRUE_PEAK
    if y.shape[1]:
        lib().emu_rateconv_tp_rule(y.ctypes.data, y.shape[0], y.shape[1], y.shape[2], hist.ctypes.data, records.ctypes.data)


class Kernel(pcm.Converter):
    """pcm.Converter over the measuring forms of the emulated kernel: process and flush also measure; measure and measure_flush only do."""

    def __init__(self, in_rate, out_rate, n_streams, channels, dither=NONE, seed=0, first_stream=0, gains=None, metering=True):
        super().__init__(in_rate, out_rate, n_streams, channels, True, dither, seed, first_stream, gains, metering)
        self.tp_hist = [np.zeros((self.n, HISTORY, self.C), np.float32), np.full((self.n, HISTORY, self.C), np.nan, np.float32)]
        self.tp_cur = 0
        self.records = np.zeros(self.n, TRUE_PEAK)

    def _run(self, in_ptr, frames, fi, fo, out_shift=0, keep=None, measure_only=False):
        n_out = self.output_frames(frames)
        out = shifted_bytes(np.full(self.n * max(n_out, 0) * self.C * BYTES[fo], SENTINEL ^ 0xFF, np.uint8), out_shift)
        st = Settings(fi, fo, self.dither, 0, self.seed, self.first_stream, self.gains.ctypes.data if self.gains is not None else None,
                      self.levels.ctypes.data if self.levels is not None else None, self.clipped.ctypes.data)
        made = lib().emu_rateconv_tp(*self.rates, self.C, in_ptr, self.n, frames, self.hist[self.cur].ctypes.data, self.hist[self.cur ^ 1].ctypes.data,
                                     self.counts.ctypes.data, self.dev_counts.ctypes.data, out.ctypes.data, ctypes.byref(st),
                                     self.tp_hist[self.tp_cur].ctypes.data, self.tp_hist[self.tp_cur ^ 1].ctypes.data, self.records.ctypes.data,
                                     int(measure_only))
        self.cur ^= 1
        if n_out > 0:
            self.tp_cur ^= 1
        assert made == n_out, (made, n_out)
        del keep
        base = out.base
        lo = out.ctypes.data - base.ctypes.data
        assert np.all(base[:lo] == SENTINEL) and np.all(base[lo + out.size:] == SENTINEL), "wrote outside the output"
        if measure_only:
            assert np.all(out == SENTINEL ^ 0xFF), "measure wrote output"
            return n_out
        return out.reshape(self.n, n_out, self.C, BYTES[fo]).copy()

    def measure(self, x, fi, shift=0):
        x = np.asarray(x, np.uint8)
        buf = shifted_bytes(x, shift)
        return self._run(buf.ctypes.data, x.shape[1], fi, F32, keep=buf, measure_only=True)

    def measure_flush(self):
        n = self._run(None, self.D, F32, F32, measure_only=True)
        self.reset()
        return n

    def reset(self):
        super().reset()
        self.tp_hist[self.tp_cur][:] = 0

    def tp_history(self):
        return self.tp_hist[self.tp_cur]


class Composition:
    """The reference: pcm's composition for bytes, levels and counts, a second one (float32 out, no gain, no dither) for y, then the rule."""

    def __init__(self, in_rate, out_rate, n_streams, channels, dither=NONE, seed=0, first_stream=0, gains=None, metering=True):
        self.q = pcm.Converter(in_rate, out_rate, n_streams, channels, False, dither, seed, first_stream, gains, metering)
        self.qy = pcm.Converter(in_rate, out_rate, n_streams, channels, False, NONE, 0, 0, None, False)
        self.n, self.C, self.D = self.q.n, self.q.C, self.q.D
        self.tp_hist = np.zeros((self.n, HISTORY, self.C), np.float32)
        self.records = np.zeros(self.n, TRUE_PEAK)

    levels = property(lambda self: self.q.levels)
    clipped = property(lambda self: self.q.clipped)
    counts = property(lambda self: self.q.counts)

    def history(self):
        return self.q.history()

    def tp_history(self):
        return self.tp_hist

    def output_frames(self, n):
        return self.q.output_frames(n)

    def process(self, x, fi, fo):
        rule(pcm.from_bytes(self.qy.process(x, fi, F32), F32), self.tp_hist, self.records)
        return self.q.process(x, fi, fo)

    def flush(self, fo):
        rule(pcm.from_bytes(self.qy.flush(F32), F32), self.tp_hist, self.records)
        self.tp_hist[:] = 0
        return self.q.flush(fo)

    def _unrecorded(self, run):
        keep = (None if self.q.levels is None else self.q.levels.copy()), self.q.clipped.copy()
        y = run()
        if keep[0] is not None:
            self.q.levels[:] = keep[0]
        self.q.clipped[:] = keep[1]
        return y.shape[1]

    def measure(self, x, fi):
        rule(pcm.from_bytes(self.qy.process(x, fi, F32), F32), self.tp_hist, self.records)
        return self._unrecorded(lambda: self.q.process(x, fi, F32))

    def measure_flush(self):
        rule(pcm.from_bytes(self.qy.flush(F32), F32), self.tp_hist, self.records)
        self.tp_hist[:] = 0
        return self._unrecorded(lambda: self.q.flush(F32))
