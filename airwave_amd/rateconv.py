"""Batch sample-rate converter over the C ABI (aw_rateconv_*, include/airwave_hip.h): a polyphase Kaiser-windowed sinc on the device, any
channel count 1..16, one handle for n_streams streams of one pair of rates.  Audio-rate conversion has no counterpart in the reference:
its Resampler (Resampler.swift:31-68) interpolates an HRIR linearly at activation, which images and aliases at about -30 dB on audio.
Nothing here computes audio."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np

from . import _capi
from .api import Context, _check, _f32, _finalizing, _fp, default_context

_INFO = ("L", "M", "taps", "latency", "tile", "frames_consumed", "frames_produced")


def rateconv_plan(in_rate: float, out_rate: float) -> Dict[str, int]:
    """aw_rateconv_plan: what a pair of rates means — L = out / g, M = in / g, taps per phase and the latency D in input frames.
    AirwaveError (INVALID_ARGUMENT) for equal, non-integral or non-positive rates and for a reduced term above 640."""
    v = [ctypes.c_int32() for _ in range(4)]
    _check(_capi.load().aw_rateconv_plan(float(in_rate), float(out_rate), *[ctypes.byref(x) for x in v]))
    return dict(zip(("L", "M", "taps", "latency"), (int(x.value) for x in v)))


def rateconv_filter(in_rate: float, out_rate: float) -> np.ndarray:
    """aw_rateconv_filter: the float32 table c[p][k] as an [L][taps] array."""
    p = rateconv_plan(in_rate, out_rate)
    c = np.zeros((p["L"], p["taps"]), np.float32)
    _check(_capi.load().aw_rateconv_filter(float(in_rate), float(out_rate), _fp(c), c.size))
    return c


class RateConverter:
    """aw_rateconv: n_streams streams of n_channels channels from in_rate to out_rate.  Output n of a stream sits at input time n M / L
    and is written once input frame floor(n M / L) + latency has arrived; flush() delivers the rest."""

    def __init__(self, in_rate: float, out_rate: float, n_streams: int, n_channels: int, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self._lib = _capi.load()
        h = ctypes.c_void_p()
        _check(self._lib.aw_rateconv_create(self.ctx._h, float(in_rate), float(out_rate), int(n_streams), int(n_channels), ctypes.byref(h)))
        self._h = h
        self.in_rate, self.out_rate, self.n_streams, self.n_channels = float(in_rate), float(out_rate), int(n_streams), int(n_channels)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.aw_rateconv_destroy(self._h)
            self._h = None

    def __del__(self):
        if not _finalizing():
            self.close()

    def info(self) -> Dict[str, int]:
        return {name: int(self._lib.aw_rateconv_info(self._h, i)) for i, name in enumerate(_INFO)}

    def output_frames(self, in_frames: int) -> int:
        """What the next process call of in_frames frames writes."""
        n = int(self._lib.aw_rateconv_output_frames(self._h, int(in_frames)))
        if n < 0:
            raise ValueError(f"in_frames must be >= 0, got {in_frames}")
        return n

    def flush_frames(self) -> int:
        """What flush() writes now."""
        return self.output_frames(self.info()["latency"])

    def process_device(self, in_ptr: int, in_frames: int, out_ptr: int, capacity: int) -> int:
        """[streams][in_frames][channels] -> [streams][n][channels] float32 device buffers, n returned; asynchronous on the context's stream."""
        n = ctypes.c_int64()
        _check(self._lib.aw_rateconv_process(self._h, ctypes.c_void_p(in_ptr), int(in_frames), ctypes.c_void_p(out_ptr), int(capacity), ctypes.byref(n)))
        return int(n.value)

    def flush_device(self, out_ptr: int, capacity: int) -> int:
        n = ctypes.c_int64()
        _check(self._lib.aw_rateconv_flush(self._h, ctypes.c_void_p(out_ptr), int(capacity), ctypes.byref(n)))
        return int(n.value)

    def _to_host(self, run, n_out: int) -> np.ndarray:
        out = np.full((self.n_streams, n_out, self.n_channels), np.nan, np.float32)
        d = self.ctx.alloc(max(out.nbytes, 4))
        try:
            made = run(d, n_out)
            assert made == n_out
            if out.size:
                self.ctx.d2h(out, d)
            else:
                self.ctx.synchronize()
        finally:
            self.ctx.free(d)
        return out

    def process(self, x) -> np.ndarray:
        """Host arrays: x [streams][frames][channels] -> [streams][output_frames(frames)][channels]."""
        x = _f32(x)
        if x.ndim != 3 or x.shape[0] != self.n_streams or x.shape[2] != self.n_channels:
            raise ValueError(f"expected [{self.n_streams}][frames][{self.n_channels}], got {x.shape}")
        frames = x.shape[1]
        if frames == 0:
            return np.zeros((self.n_streams, 0, self.n_channels), np.float32)
        d_in = self.ctx.alloc(x.nbytes)
        try:
            self.ctx.h2d(d_in, x)
            return self._to_host(lambda d, cap: self.process_device(d_in, frames, d, cap), self.output_frames(frames))
        finally:
            self.ctx.free(d_in)

    def flush(self) -> np.ndarray:
        """The outputs still owed for the input so far (`latency` zero frames pushed behind it), then reset()."""
        return self._to_host(self.flush_device, self.flush_frames())

    def reset(self) -> None:
        _check(self._lib.aw_rateconv_reset(self._h))


def convert(x, in_rate: float, out_rate: float, ctx: Optional[Context] = None) -> np.ndarray:
    """One shot: x [streams][N][channels] (or [N][channels]) -> [..][ceil(N L / M)][channels]: process + flush, concatenated."""
    a = _f32(x)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"expected [streams][frames][channels] or [frames][channels], got {a.shape}")
    rc = RateConverter(in_rate, out_rate, a.shape[0], a.shape[2], ctx=ctx)
    try:
        y = np.concatenate([rc.process(a), rc.flush()], axis=1)
    finally:
        rc.close()
    return y[0] if squeeze else y
