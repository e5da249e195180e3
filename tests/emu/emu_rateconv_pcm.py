"""TEST-ONLY: ctypes access to the PCM form of the sample-rate converter's kernel on emulated workgroups and to the composition of the
separately tested rules that is its reference (tests/emu/emu_rateconv_pcm.cpp).  Samples travel as uint8 arrays [streams][frames][channels]
[bytes of the format], little-endian, so that s24 needs no special case."""
import ctypes
import os

import numpy as np

import _build
import emu_rateconv as emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_rateconv_pcm.so")
_lib = None
V = ctypes.c_void_p
_D, _I, _LL, _U64 = ctypes.c_double, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong

F32, S16, S24, S32 = 0, 1, 2, 3
FORMATS = (F32, S16, S24, S32)
NAMES = {F32: "f32", S16: "s16", S24: "s24", S32: "s32"}
BYTES = {F32: 4, S16: 2, S24: 3, S32: 4}
NONE, TPDF, TPDF_HP = 0, 1, 2
SENTINEL = 0xA5
PAIR_KEY = 0xA0761D6478BD642F
LEVELS = np.dtype([("peak", np.float32), ("reserved", np.uint32), ("frames", np.uint64), ("clipped", np.uint64), ("nonfinite", np.uint64)])
assert LEVELS.itemsize == 32


class Settings(ctypes.Structure):
    _fields_ = [("in_format", _I), ("out_format", _I), ("dither", _I), ("reserved", _I), ("seed", _U64), ("first_stream", _U64),
                ("gains", V), ("levels", V), ("clipped", V)]


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, [(os.path.join(_HERE, "emu_rateconv_pcm.cpp"), [])], link_flags=["-pthread"])
        _lib.emu_rateconv_pcm.argtypes = [_D, _D, _I, V, _I, _LL, V, V, V, V, V, V]
        _lib.emu_rateconv_pcm.restype = _LL
        _lib.emu_rateconv_pcm_composition.argtypes = [_D, _D, _I, V, _I, _LL, V, V, V, V]
        _lib.emu_rateconv_pcm_composition.restype = _LL
        _lib.emu_rateconv_pcm_key.argtypes = [_U64, _U64, _I]
        _lib.emu_rateconv_pcm_key.restype = _U64
        _lib.emu_rateconv_pcm_dither.argtypes = [_I, _U64, _U64, _I]
        _lib.emu_rateconv_pcm_dither.restype = ctypes.c_float
    return _lib


def key(seed, global_stream, channel):
    return int(lib().emu_rateconv_pcm_key(seed, global_stream, channel))


def dither(mode, k, n, e):
    return float(lib().emu_rateconv_pcm_dither(mode, k, n, e))


def to_bytes(a, fmt):
    """An int16 / int32 / float32 array, or 24-bit integers held in int32, as [...][bytes] uint8."""
    if fmt == S24:
        v = np.asarray(a, np.int32)
        return np.stack([(v >> (8 * i)) & 0xFF for i in range(3)], axis=-1).astype(np.uint8)
    dt = {F32: np.float32, S16: np.int16, S32: np.int32}[fmt]
    v = np.ascontiguousarray(a, dt)
    return v.view(np.uint8).reshape(*v.shape, BYTES[fmt]).copy()


def from_bytes(b, fmt):
    """[...][bytes] uint8 -> int16 / int32 / float32 values (s24: sign-extended in int32)."""
    b = np.ascontiguousarray(b, np.uint8)
    if fmt == S24:
        u = b[..., 0].astype(np.int32) | (b[..., 1].astype(np.int32) << 8) | (b[..., 2].astype(np.int32) << 16)
        return (u << 8) >> 8
    dt = {F32: np.float32, S16: np.int16, S32: np.int32}[fmt]
    return b.view(dt).reshape(b.shape[:-1])


def random_input(rng, shape, fmt, scale=0.25):
    """Normal samples of standard deviation `scale` of full scale in format fmt, as bytes [*shape][bytes]."""
    x = scale * rng.standard_normal(shape)
    if fmt == F32:
        return to_bytes(x.astype(np.float32), F32)
    bits = {S16: 15, S24: 23, S32: 31}[fmt]
    return to_bytes(np.clip(np.rint(x * 2.0 ** bits), -2.0 ** bits, 2.0 ** bits - 1).astype(np.int64).astype(np.int32), fmt)


def shifted_bytes(b, shift):
    """A flat copy of the uint8 array b that starts `shift` bytes past a 16-byte boundary, between sentinel bytes."""
    raw = np.full(b.size + 64, SENTINEL, np.uint8)
    off = (-raw.ctypes.data) % 16 + 16 + shift
    buf = raw[off:off + b.size]
    buf[:] = np.asarray(b, np.uint8).reshape(-1)
    return buf


class Converter:
    """The carried state of n_streams streams and the settings of the PCM entries.  kernel: the emulated kernel, else the composition."""

    def __init__(self, in_rate, out_rate, n_streams, channels, kernel, dither=NONE, seed=0, first_stream=0, gains=None, metering=True):
        self.rates, self.n, self.C, self.kernel = (float(in_rate), float(out_rate)), int(n_streams), int(channels), kernel
        self.L, self.M, self.T, self.D = emu.plan(in_rate, out_rate)
        self.hist = [np.zeros((self.n, self.T - 1, self.C), np.float32), np.full((self.n, self.T - 1, self.C), np.nan, np.float32)]
        self.cur = 0
        self.counts = np.zeros(2, np.int64)
        self.dev_counts = np.zeros((self.n, 2), np.int64)
        self.dither, self.seed, self.first_stream = dither, seed, first_stream
        self.gains = None if gains is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gains, np.float32), (self.n,)))
        self.levels = np.zeros(self.n, LEVELS) if metering else None
        self.clipped = np.zeros(1, np.uint64)

    def output_frames(self, in_frames):
        N = int(self.counts[0]) + in_frames
        return max(0, -((N - self.D) * self.L // -self.M)) - int(self.counts[1])

    def process(self, x, fi, fo, shift=0, out_shift=0):
        """x: [streams][frames][channels][bytes of fi] uint8; shift, out_shift: bytes past a 16-byte boundary the buffers start at.
        Returns [streams][produced][channels][bytes of fo] uint8."""
        x = np.asarray(x, np.uint8)
        assert x.shape[0] == self.n and x.shape[2] == self.C and x.shape[1] > 0 and x.shape[3] == BYTES[fi]
        buf = shifted_bytes(x, shift)
        return self._run(buf.ctypes.data, x.shape[1], fi, fo, out_shift, keep=buf)

    def _run(self, in_ptr, frames, fi, fo, out_shift=0, keep=None):
        n_out = self.output_frames(frames)
        out = shifted_bytes(np.full(self.n * max(n_out, 0) * self.C * BYTES[fo], SENTINEL ^ 0xFF, np.uint8), out_shift)
        st = Settings(fi, fo, self.dither, 0, self.seed, self.first_stream, self.gains.ctypes.data if self.gains is not None else None,
                      self.levels.ctypes.data if self.levels is not None else None, self.clipped.ctypes.data)
        if self.kernel:
            made = lib().emu_rateconv_pcm(*self.rates, self.C, in_ptr, self.n, frames, self.hist[self.cur].ctypes.data,
                                          self.hist[self.cur ^ 1].ctypes.data, self.counts.ctypes.data, self.dev_counts.ctypes.data, out.ctypes.data,
                                          ctypes.byref(st))
            self.cur ^= 1
        else:
            made = lib().emu_rateconv_pcm_composition(*self.rates, self.C, in_ptr, self.n, frames, self.hist[self.cur].ctypes.data,
                                                      self.counts.ctypes.data, out.ctypes.data, ctypes.byref(st))
            self.dev_counts[:] = self.counts
        assert made == n_out, (made, n_out)
        del keep
        base = out.base                                # (out is a view into a larger sentinel buffer: anything written beside it shows there)
        lo = out.ctypes.data - base.ctypes.data
        assert np.all(base[:lo] == SENTINEL) and np.all(base[lo + out.size:] == SENTINEL), "wrote outside the output"
        return out.reshape(self.n, n_out, self.C, BYTES[fo]).copy()

    def flush(self, fo):
        """process of D zero frames, then reset; the records stay."""
        y = self._run(None, self.D, F32, fo)
        self.reset()
        return y

    def reset(self):
        self.hist[self.cur][:] = 0
        self.counts[:] = 0
        self.dev_counts[:] = 0

    def history(self):
        return self.hist[self.cur]
