"""Batch sample-rate converter over the C ABI (aw_rateconv_*, include/airwave_hip.h): a polyphase Kaiser-windowed sinc on the device, any
channel count 1..16, one handle for n_streams streams of one pair of rates.  Audio-rate conversion has no counterpart in the reference:
its Resampler (Resampler.swift:31-68) interpolates an HRIR linearly at activation, which images and aliases at about -30 dB on audio.
Nothing here computes audio."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np

from . import _capi
from .api import (DITHER_MODES, GAIN_MODES, SAMPLE_FORMATS, _FORMAT_DTYPE, Context, _check, _f32, _finalizing, _fp, _pcm_array,
                  default_context)

_INFO = ("L", "M", "taps", "latency", "tile", "frames_consumed", "frames_produced", "dither", "gain_mode", "metering", "true_peak", "true_peak_tile")
# aw_rateconv_levels, byte for byte (RateConverter.levels)
RATECONV_LEVELS_DTYPE = np.dtype([("peak", np.float32), ("reserved", np.uint32), ("frames", np.uint64), ("clipped", np.uint64),
                                  ("nonfinite", np.uint64)], align=False)
# aw_rateconv_true_peak, byte for byte (RateConverter.true_peak)
RATECONV_TRUE_PEAK_DTYPE = np.dtype([("true_peak", np.float32), ("sample_peak", np.float32), ("frames", np.uint64)], align=False)


def _format_code(fmt) -> int:
    code = SAMPLE_FORMATS.get(fmt, -1) if isinstance(fmt, str) else int(fmt)
    if code not in _FORMAT_DTYPE:
        raise ValueError(f"unknown sample format {fmt!r}")
    return code


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
            # a reference cycle is finalised in no particular order: where the context went first, its stream is gone, and
            # aw_rateconv_destroy, which waits for that stream, must not run (what the handle owns on the device then stays
            # allocated until the process ends)
            if getattr(self.ctx, "_h", None):
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

    # ---- integer PCM in and out, with dither, gain and levels (aw_pcm_rateconv_*) ----

    def process_pcm_device(self, in_ptr: int, in_format, in_frames: int, out_ptr: int, out_format, capacity: int, clipped_ptr: int = 0) -> int:
        """aw_pcm_rateconv_process on device buffers of any byte alignment; formats by name ('f32', 's16', 's24', 's32') or code.
        clipped_ptr: 0, or a device uint64 the call adds its clipped-sample count to.  Returns the frames written."""
        n = ctypes.c_int64()
        _check(self._lib.aw_pcm_rateconv_process(self._h, ctypes.c_void_p(in_ptr), _format_code(in_format), int(in_frames), ctypes.c_void_p(out_ptr),
                                                 _format_code(out_format), int(capacity), ctypes.byref(n), ctypes.c_void_p(clipped_ptr or None)))
        return int(n.value)

    def flush_pcm_device(self, out_ptr: int, out_format, capacity: int, clipped_ptr: int = 0) -> int:
        n = ctypes.c_int64()
        _check(self._lib.aw_pcm_rateconv_flush(self._h, ctypes.c_void_p(out_ptr), _format_code(out_format), int(capacity), ctypes.byref(n),
                                               ctypes.c_void_p(clipped_ptr or None)))
        return int(n.value)

    def set_dither(self, mode, seed: int = 0, first_stream: int = 0) -> None:
        """aw_pcm_rateconv_set_dither: dither of every later s16 / s24 encode of the PCM entries ('none', 'tpdf', 'tpdf_hp', or the
        aw_dither code).  first_stream: the global index of this handle's stream 0."""
        if isinstance(mode, str):
            if mode not in DITHER_MODES:
                raise ValueError(f"unknown dither mode {mode!r} (one of {', '.join(DITHER_MODES)})")
            mode = DITHER_MODES[mode]
        _check(self._lib.aw_pcm_rateconv_set_dither(self._h, int(mode), int(seed), int(first_stream)))

    def set_gain(self, mode, gains=None) -> None:
        """aw_pcm_rateconv_set_gain: 'none', or 'fixed' with one gain (every stream) or one per stream.  The ceiling modes are refused by
        the library: they are per-call functions of a peak, which the one-pass converter does not have."""
        if isinstance(mode, str):
            if mode not in GAIN_MODES:
                raise ValueError(f"unknown gain mode {mode!r} (one of {', '.join(GAIN_MODES)})")
            mode = GAIN_MODES[mode]
        g = None
        if gains is not None:
            g = np.ascontiguousarray(np.atleast_1d(np.asarray(gains, np.float32)))
            if g.ndim != 1:
                raise ValueError(f"gains must be 1 or {self.n_streams} values, got shape {g.shape}")
        _check(self._lib.aw_pcm_rateconv_set_gain(self._h, int(mode), None if g is None else _fp(g), 0 if g is None else int(g.size)))

    def set_metering(self, on: bool = True) -> None:
        """aw_pcm_rateconv_set_metering: per-stream records of every later PCM call; switching it on allocates them here."""
        _check(self._lib.aw_pcm_rateconv_set_metering(self._h, int(bool(on))))

    def levels(self, first_stream: int = 0, n: Optional[int] = None) -> np.ndarray:
        """aw_pcm_rateconv_get_levels: the records of n streams from first_stream on (default: all) as a structured array of
        RATECONV_LEVELS_DTYPE (peak, frames, clipped, nonfinite).  Synchronises the context's stream."""
        first_stream = int(first_stream)
        n = self.n_streams - first_stream if n is None else int(n)
        out = np.zeros(max(n, 0), RATECONV_LEVELS_DTYPE)
        _check(self._lib.aw_pcm_rateconv_get_levels(self._h, first_stream, n, ctypes.c_void_p(out.ctypes.data)))
        return out

    def reset_levels(self) -> None:
        _check(self._lib.aw_pcm_rateconv_reset_levels(self._h))

    def _pcm_to_host(self, run, n_out: int, fo: int):
        """-> (array in the conventions of Spatializer's PCM methods, clipped count of the call)."""
        shape = (self.n_streams, n_out, self.n_channels) + ((3,) if fo == 2 else ())
        out = np.zeros(shape, _FORMAT_DTYPE[fo])
        d = self.ctx.alloc(max(out.nbytes, 4) + 8)       # the clipped count leads, the samples follow it
        d_clip = d
        try:
            zero = np.zeros(1, np.uint64)
            self.ctx.h2d(d_clip, zero)
            made = run(d + 8, n_out, d_clip)
            assert made == n_out
            if out.size:
                self.ctx.d2h(out, d + 8)
            self.ctx.d2h(zero, d_clip)
        finally:
            self.ctx.free(d)
        return out, int(zero[0])

    def process_pcm(self, x, out_format, in_format=None):
        """Host arrays: x [streams][frames][channels] of int16, int32, float32 or packed s24 (uint8 [..., 3], in_format='s24') ->
        (y, clipped): y [streams][output_frames(frames)][channels] in out_format (packed s24: uint8 [..., 3]) and the call's clipped count."""
        if not isinstance(x, np.ndarray) or x.ndim < 3:
            raise ValueError("x: [streams][frames][channels] array required")
        frames = x.shape[1]
        x, fi = _pcm_array(x, in_format, (self.n_streams, frames, self.n_channels), "x")
        fo = _format_code(out_format)
        if frames == 0:
            return np.zeros((self.n_streams, 0, self.n_channels) + ((3,) if fo == 2 else ()), _FORMAT_DTYPE[fo]), 0
        d_in = self.ctx.alloc(x.nbytes)
        try:
            self.ctx.h2d(d_in, x)
            return self._pcm_to_host(lambda d, cap, clip: self.process_pcm_device(d_in, fi, frames, d, fo, cap, clip), self.output_frames(frames), fo)
        finally:
            self.ctx.free(d_in)

    def flush_pcm(self, out_format):
        """(the outputs still owed in out_format, their clipped count), then reset(); the records stay."""
        fo = _format_code(out_format)
        return self._pcm_to_host(lambda d, cap, clip: self.flush_pcm_device(d, fo, cap, clip), self.flush_frames(), fo)

    # ---- true peak of the converted output and the ceiling pass (aw_tp_rateconv_*) ----

    def set_true_peak(self, on: bool = True) -> None:
        """aw_tp_rateconv_set: measure the true peak of every later PCM call's own output (before gain, dither and encode); switching it
        on makes the feature's one device allocation here.  The float32 family (process / flush) is not measured.  AirwaveError
        (INVALID_ARGUMENT) for the few handles whose tile leaves no room for the measuring form (info()['true_peak_tile'] == 0)."""
        _check(self._lib.aw_tp_rateconv_set(self._h, int(bool(on))))

    def true_peak(self, first_stream: int = 0, n: Optional[int] = None) -> np.ndarray:
        """aw_tp_rateconv_get: the records of n streams from first_stream on (default: all) as a structured array of
        RATECONV_TRUE_PEAK_DTYPE (true_peak, sample_peak, frames).  Synchronises the context's stream."""
        first_stream = int(first_stream)
        n = self.n_streams - first_stream if n is None else int(n)
        out = np.zeros(max(n, 0), RATECONV_TRUE_PEAK_DTYPE)
        _check(self._lib.aw_tp_rateconv_get(self._h, first_stream, n, ctypes.c_void_p(out.ctypes.data)))
        return out

    def reset_true_peak(self) -> None:
        _check(self._lib.aw_tp_rateconv_reset_records(self._h))

    def measure_device(self, in_ptr: int, in_format, in_frames: int) -> int:
        """aw_tp_rateconv_measure: process_pcm_device without an output — the counts and the history move, only the true-peak records
        change.  Returns the frames the call would have written."""
        n = ctypes.c_int64()
        _check(self._lib.aw_tp_rateconv_measure(self._h, ctypes.c_void_p(in_ptr), _format_code(in_format), int(in_frames), ctypes.byref(n)))
        return int(n.value)

    def measure_flush_device(self) -> int:
        """aw_tp_rateconv_measure_flush: flush_pcm_device without an output; ends with the reset, so a second pass starts clean."""
        n = ctypes.c_int64()
        _check(self._lib.aw_tp_rateconv_measure_flush(self._h, ctypes.byref(n)))
        return int(n.value)

    def measure(self, x, in_format=None) -> int:
        """Host arrays: measure_device over x [streams][frames][channels] (the conventions of process_pcm).  Returns the frames measured."""
        if not isinstance(x, np.ndarray) or x.ndim < 3:
            raise ValueError("x: [streams][frames][channels] array required")
        frames = x.shape[1]
        x, fi = _pcm_array(x, in_format, (self.n_streams, frames, self.n_channels), "x")
        if frames == 0:
            return 0
        d_in = self.ctx.alloc(x.nbytes)
        try:
            self.ctx.h2d(d_in, x)
            n = self.measure_device(d_in, fi, frames)
            self.ctx.synchronize()
        finally:
            self.ctx.free(d_in)
        return n

    def ceiling_gains(self, ceiling: float) -> np.ndarray:
        """The per-stream gains that hold `ceiling` (linear full scale) over what the records have measured: g = tp > c ? c / tp : 1 in
        float32, for set_gain('fixed', g) before a second pass over the same input."""
        c = np.float32(ceiling)
        if not np.isfinite(c) or c <= 0:
            raise ValueError(f"ceiling must be positive and finite, got {ceiling!r}")
        t = self.true_peak()["true_peak"]
        return np.where(t > c, c / np.maximum(t, np.float32(1e-38)), np.float32(1.0)).astype(np.float32)


def convert(x, in_rate: float, out_rate: float, ctx: Optional[Context] = None, out_format=None, dither="none", seed: int = 0,
            in_format=None, true_peak_ceiling: Optional[float] = None, gains=None) -> np.ndarray:
    """One shot: x [streams][N][channels] (or [N][channels]) -> [..][ceil(N L / M)][channels]: process + flush, concatenated.  With
    out_format ('f32', 's16', 's24', 's32') x may be int16, int32, float32 or packed s24 (uint8 [..., 3], in_format='s24') and the result
    is in out_format, s16 / s24 dithered by `dither` ('none', 'tpdf', 'tpdf_hp') with `seed`.  `gains`: a fixed gain, one or one per
    stream.  true_peak_ceiling (linear full scale; needs an out_format): a measuring pass (measure + measure_flush) first, then the
    converting pass under the smaller of the ceiling's gain and the caller's, per stream."""
    if out_format is None:
        if dither not in ("none", 0) or in_format is not None or true_peak_ceiling is not None or gains is not None:
            raise ValueError("dither, in_format, gains and true_peak_ceiling need an out_format")
        a = _f32(x)
        packed = 0
    else:
        a = np.ascontiguousarray(x)
        packed = 1 if (in_format in ("s24", 2)) else 0
    squeeze = a.ndim - packed == 2
    if squeeze:
        a = a[None]
    if a.ndim - packed != 3:
        raise ValueError(f"expected [streams][frames][channels] or [frames][channels], got {a.shape}")
    rc = RateConverter(in_rate, out_rate, a.shape[0], a.shape[2], ctx=ctx)
    try:
        if out_format is None:
            y = np.concatenate([rc.process(a), rc.flush()], axis=1)
        else:
            rc.set_dither(dither, seed)
            g = None if gains is None else np.broadcast_to(np.atleast_1d(np.asarray(gains, np.float32)), (rc.n_streams,))
            if true_peak_ceiling is not None:
                rc.set_true_peak(True)
                rc.measure(a, in_format)
                rc.measure_flush_device()
                held = rc.ceiling_gains(true_peak_ceiling)
                g = held if g is None else np.minimum(g, held)
                rc.set_true_peak(False)
            if g is not None:
                rc.set_gain("fixed", g)
            y = np.concatenate([rc.process_pcm(a, out_format, in_format)[0], rc.flush_pcm(out_format)[0]], axis=1)
    finally:
        rc.close()
    return y[0] if squeeze else y
