"""Host-side mirror of the reference's operator surface for the HRIR convolution path, over the C ABI.

Same names, argument meaning and error behaviour as the Swift types (cited per class), so parity
tests read like the reference's XCTests.  All arithmetic happens in libairwave_hip.so on the GPU;
nothing here computes audio.
"""
from __future__ import annotations

import ctypes
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from ._capi import c_float_p, c_int32_p

AW_OK = 0
EQ_KEEP = -2          # AW_EQ_KEEP: a stream that is not part of a target change (Spatializer.set_equalizer_target)
STATUS_NAMES = {
    1: "INVALID_ARGUMENT", 2: "OUT_OF_MEMORY", 3: "HIP", 4: "NO_DEVICE", 5: "INVALID_CHANNEL_MAPPING",
    6: "CONVOLUTION_SETUP_FAILED", 7: "INVALID_CHANNEL_COUNT", 8: "WAV_FILE_READ", 9: "WAV_EMPTY_FILE",
    10: "WAV_UNSUPPORTED_FORMAT", 11: "BLOCK_SIZE_MISMATCH", 12: "EQ_PARSE", 13: "EQ_INVALID_SAMPLE_RATE",
    14: "EQ_NON_FINITE_PREAMP", 15: "EQ_TOO_MANY_FILTERS", 16: "EQ_INVALID_FILTER",
}


class AirwaveError(RuntimeError):
    """Any non-zero aw_status.  `.status` is the code, `.name` its symbolic name."""

    def __init__(self, status: int, message: str):
        self.status = status
        self.name = STATUS_NAMES.get(status, str(status))
        super().__init__(f"AW_ERR_{self.name}: {message}")


class HRIRError(AirwaveError):          # HRIRManager.swift:737-759
    pass


class WAVError(AirwaveError):           # WAVLoader.swift:127-147
    pass


def _finalizing() -> bool:
    """True while the interpreter shuts down.  Handles that own device memory are not destroyed then: module globals and reference
    cycles are collected in no particular order (a context can go before the objects created on it), and the HIP runtime's own exit
    handlers may already have run — the process is about to return everything to the driver anyway.  (Found by tools/fuzz_eq.py, whose
    last processor died at exit: std::bad_variant_access out of the HIP runtime, exit code 134 after a clean run.)"""
    return sys.is_finalizing()


def _check(status: int) -> None:
    if status == AW_OK:
        return
    msg = (_capi.load().aw_last_error_message() or b"").decode("utf-8", "replace")
    if status in (5, 6, 7):
        raise HRIRError(status, msg)
    if status in (8, 9, 10):
        raise WAVError(status, msg)
    raise AirwaveError(status, msg)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _fp(a: np.ndarray):
    return a.ctypes.data_as(c_float_p)


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(c_int32_p)


# aw_sample_format (include/airwave_hip.h): sample formats of the PCM entries
SAMPLE_FORMATS = {"f32": 0, "s16": 1, "s24": 2, "s32": 3}
_FORMAT_DTYPE = {0: np.dtype(np.float32), 1: np.dtype(np.int16), 2: np.dtype(np.uint8), 3: np.dtype(np.int32)}
# aw_dither (include/airwave_hip.h): dither of the s16 / s24 encode (Spatializer.set_dither)
DITHER_MODES = {"none": 0, "tpdf": 1, "tpdf_hp": 2}
# aw_gain_mode: output gain of the batch entries (Spatializer.set_gain)
GAIN_MODES = {"none": 0, "fixed": 1, "peak_ceiling": 2, "true_peak_ceiling": 3}
# aw_stream_levels, byte for byte (Spatializer.levels)
LEVELS_DTYPE = np.dtype([("peak", np.float32, (2,)), ("gain", np.float32), ("reserved", np.uint32), ("energy", np.float64, (2,)),
                         ("frames", np.uint64), ("clipped", np.uint64), ("nonfinite", np.uint64)], align=False)

# aw_stream_loudness, byte for byte (Spatializer.loudness)
LOUDNESS_DTYPE = np.dtype([("integrated_lufs", np.float64), ("relative_threshold_lufs", np.float64), ("blocks", np.uint32),
                           ("blocks_above_absolute", np.uint32), ("blocks_gated", np.uint32), ("reserved", np.uint32),
                           ("frames", np.uint64), ("frames_dropped", np.uint64), ("nonfinite", np.uint64)], align=False)

# aw_stream_true_peak, byte for byte (Spatializer.true_peak)
TRUE_PEAK_DTYPE = np.dtype([("true_peak", np.float32, (2,)), ("call_true_peak", np.float32), ("reserved", np.uint32), ("frames", np.uint64),
                            ("nonfinite", np.uint64)], align=False)

# aw_stream_limiter, byte for byte (Spatializer.limiter)
LIMITER_DTYPE = np.dtype([("min_gain", np.float32), ("reserved", np.uint32), ("frames", np.uint64), ("limited_frames", np.uint64),
                          ("nonfinite", np.uint64)], align=False)


def true_peak_filter() -> np.ndarray:
    """aw_true_peak_filter: the interpolator's float32 coefficients c[p][k], p = 1 .. 3, as a [3][12] array."""
    c = np.zeros(36, np.float32)
    _check(_capi.load().aw_true_peak_filter(_fp(c)))
    return c.reshape(3, 12)


def loudness_gain(lufs: float, target_lufs: float) -> float:
    """aw_loudness_gain: 10^((target - lufs) / 20) as float32.  ValueError for a non-finite loudness (a silent stream) or target."""
    lufs, target_lufs = float(lufs), float(target_lufs)
    if not (np.isfinite(lufs) and np.isfinite(target_lufs)):
        raise ValueError(f"loudness and target must be finite, got {lufs!r} and {target_lufs!r}")
    g = ctypes.c_float(0.0)
    _check(_capi.load().aw_loudness_gain(lufs, target_lufs, ctypes.byref(g)))
    return float(g.value)


def sample_format_bytes(fmt) -> int:
    """aw_sample_format_bytes: 4, 2, 3, 4 for f32, s16, s24, s32; 0 for an unknown format."""
    code = SAMPLE_FORMATS.get(fmt, -1) if isinstance(fmt, str) else int(fmt)
    return int(_capi.load().aw_sample_format_bytes(code))


def _pcm_array(a, fmt, shape3, what: str) -> Tuple[np.ndarray, int]:
    """Checks one PCM buffer against its format and the [S, F, C] shape it must have (s24: packed bytes, uint8 [S, F, C, 3]) and
    returns (array, aw_sample_format).  fmt None: from the dtype (float32, int16, int32; packed s24 must be named).  Raises before
    the library is called."""
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{what}: a numpy array is required")
    if fmt is None:
        code = {np.dtype(np.float32): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 3}.get(a.dtype)
        if code is None:
            raise TypeError(f"{what}: dtype {a.dtype} has no implied sample format (float32, int16, int32; packed s24: fmt='s24', uint8 [..., 3])")
    else:
        code = SAMPLE_FORMATS.get(fmt) if isinstance(fmt, str) else (int(fmt) if int(fmt) in _FORMAT_DTYPE else None)
        if code is None:
            raise ValueError(f"{what}: unknown sample format {fmt!r}")
        if a.dtype != _FORMAT_DTYPE[code]:
            raise TypeError(f"{what}: format {fmt!r} needs dtype {_FORMAT_DTYPE[code]}, got {a.dtype}")
    want = tuple(shape3) + ((3,) if code == 2 else ())
    if a.shape != want:
        raise ValueError(f"{what}: shape {a.shape}, expected {want}")
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{what}: must be C-contiguous")
    return a, code


class Context:
    """Device + stream + shared twiddle tables (FFTSetupManager analogue, FFTSetupManager.swift:41-60)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._lib = _capi.load()
        h = ctypes.c_void_p()
        if stream is None:
            _check(self._lib.aw_context_create(device, ctypes.byref(h)))
        else:
            _check(self._lib.aw_context_create_on_stream(device, ctypes.c_void_p(stream), ctypes.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.aw_context_destroy(self._h)
            self._h = None

    def __del__(self):
        if not _finalizing():
            self.close()

    def set_resampler(self, literal_vgenp: bool = False) -> None:
        """Which resampler activatePreset uses for this context: the intended interpolation (default) or the literal
        vDSP_vgenp call of the shipped reference."""
        _check(self._lib.aw_context_set_resampler(self._h, int(literal_vgenp)))

    def synchronize(self):
        _check(self._lib.aw_context_synchronize(self._h))

    @property
    def stream(self) -> int:
        return self._lib.aw_context_stream(self._h) or 0

    def timer_start(self):
        _check(self._lib.aw_context_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = ctypes.c_float()
        _check(self._lib.aw_context_timer_stop(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def reserve_scratch(self, nbytes: int) -> None:
        """Size the context's scratch pool (shared by its spatializers) ahead of time: the one large hipMalloc at start-up."""
        _check(self._lib.aw_context_reserve_scratch(self._h, int(nbytes)))

    @property
    def scratch_bytes(self) -> int:
        return int(self._lib.aw_context_scratch_bytes(self._h))

    def bandwidth_probe(self, nbytes: int = 4 << 30, repetitions: int = 3) -> Dict[str, float]:
        """Measured read-only / write-only / copy rates of this device in GB/s (copy = bytes read + bytes written per second):
        the ceiling SURVEY.md 8d asks to quote next to the vendor peak."""
        r, w, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _check(self._lib.aw_context_bandwidth_probe(self._h, nbytes, repetitions, ctypes.byref(r), ctypes.byref(w), ctypes.byref(c)))
        return {"read": r.value, "write": w.value, "copy": c.value}

    def pcie_probe(self, nbytes: int = 1 << 30, repetitions: int = 2) -> Dict[str, float]:
        """Page-locked hipMemcpyAsync rates in GB/s: host to device, device to host, and both at once (bytes both ways per second)."""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _check(self._lib.aw_context_pcie_probe(self._h, nbytes, repetitions, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"h2d": a.value, "d2h": b.value, "duplex": c.value}

    def pinned_empty(self, shape, dtype=np.float32) -> np.ndarray:
        """A numpy array over page-locked host memory (aw_host_alloc_pinned); freed when the array's base object dies."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        _check(self._lib.aw_host_alloc_pinned(self._h, n, ctypes.byref(p)))
        owner = _PinnedOwner(self, p.value, max(n, 1))
        return np.asarray(owner)[:n].view(dtype).reshape(shape)

    # raw device memory for hosts without torch
    def alloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        _check(self._lib.aw_device_alloc(self._h, nbytes, ctypes.byref(p)))
        return p.value

    def free(self, dptr: int):
        _check(self._lib.aw_device_free(self._h, ctypes.c_void_p(dptr)))

    def h2d(self, dptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        _check(self._lib.aw_memcpy_h2d(self._h, ctypes.c_void_p(dptr), arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes))

    def d2h(self, arr: np.ndarray, dptr: int):
        assert arr.flags["C_CONTIGUOUS"]
        _check(self._lib.aw_memcpy_d2h(self._h, arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dptr), arr.nbytes))

    def synth_fill(self, dptr: int, n_streams: int, frames: int, n_channels: int, seed: int = 0xA17AE, first_stream: int = 0):
        _check(self._lib.aw_synth_fill(self._h, ctypes.c_void_p(dptr), n_streams, frames, n_channels, seed, first_stream))


class _PinnedOwner:
    """Base object of the numpy views over one page-locked allocation (array interface): alive as long as any view is, then frees it."""

    def __init__(self, ctx: "Context", ptr: int, nbytes: int):
        self._ctx, self._ptr = ctx, ptr
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    def __del__(self):
        try:
            if self._ptr and getattr(self._ctx, "_h", None) and not _finalizing():
                self._ctx._lib.aw_host_free_pinned(self._ctx._h, ctypes.c_void_p(self._ptr))
        finally:
            self._ptr = 0


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ---- WAVLoader -------------------------------------------------------------------------------------
class WAVData:
    """WAVData (WAVLoader.swift:12-17): sampleRate, channelCount, frameCount, audioData [[Float]]."""

    def __init__(self, sample_rate: float, channel_count: int, frame_count: int, audio_data: np.ndarray):
        self.sample_rate = sample_rate
        self.channel_count = channel_count
        self.frame_count = frame_count
        self.audio_data = audio_data


class WAVLoader:
    @staticmethod
    def load(path: str) -> WAVData:
        """WAVLoader.load(from:)  WAVLoader.swift:26-99"""
        lib = _capi.load()
        h = ctypes.c_void_p()
        _check(lib.aw_wav_load(path.encode(), ctypes.byref(h)))
        try:
            ch, fr = lib.aw_wav_channel_count(h), lib.aw_wav_frame_count(h)
            data = np.ctypeslib.as_array(lib.aw_wav_planar(h), shape=(ch, fr)).copy()
            return WAVData(lib.aw_wav_sample_rate(h), ch, fr, data)
        finally:
            lib.aw_wav_destroy(h)


# ---- InputLayout / HRIRChannelMap --------------------------------------------------------------------
class InputLayout:
    """InputLayout (VirtualSpeaker.swift:59-100)."""

    def __init__(self, channels: Sequence[str], name: str = ""):
        lib = _capi.load()
        arr = (ctypes.c_char_p * max(len(channels), 1))(*[c.encode() for c in channels])
        h = ctypes.c_void_p()
        _check(lib.aw_layout_create(arr, len(channels), name.encode(), ctypes.byref(h)))
        self._h, self._lib = h, lib

    @classmethod
    def _wrap(cls, h):
        obj = cls.__new__(cls)
        obj._h, obj._lib = h, _capi.load()
        return obj

    @classmethod
    def detect(cls, channel_count: int) -> "InputLayout":
        h = ctypes.c_void_p()
        _check(_capi.load().aw_layout_detect(channel_count, ctypes.byref(h)))
        return cls._wrap(h)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.aw_layout_destroy(self._h)
            self._h = None

    @property
    def channels(self) -> List[str]:
        return [self._lib.aw_layout_speaker(self._h, i).decode() for i in range(self._lib.aw_layout_count(self._h))]

    @property
    def name(self) -> str:
        return self._lib.aw_layout_name(self._h).decode()


InputLayout.stereo = staticmethod(lambda: InputLayout.detect(2))          # type: ignore[attr-defined]
InputLayout.surround51 = staticmethod(lambda: InputLayout.detect(6))      # type: ignore[attr-defined]
InputLayout.surround71 = staticmethod(lambda: InputLayout.detect(8))      # type: ignore[attr-defined]
InputLayout.atmos714 = staticmethod(lambda: InputLayout.detect(12))       # type: ignore[attr-defined]


class HRIRChannelMap:
    """HRIRChannelMap (VirtualSpeaker.swift:103-347)."""

    def __init__(self, h):
        self._h, self._lib = h, _capi.load()

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.aw_map_destroy(self._h)
            self._h = None

    @classmethod
    def _make(cls, fn_name: str, arg) -> "HRIRChannelMap":
        h = ctypes.c_void_p()
        _check(getattr(_capi.load(), fn_name)(arg, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def hesuvi14Channel(cls, speakers: InputLayout):
        return cls._make("aw_map_hesuvi14", speakers._h)

    @classmethod
    def hesuvi7Channel(cls, speakers: InputLayout):
        return cls._make("aw_map_hesuvi7", speakers._h)

    @classmethod
    def interleavedPairs(cls, speakers: InputLayout):
        return cls._make("aw_map_interleaved_pairs", speakers._h)

    @classmethod
    def splitBlocks(cls, speakers: InputLayout):
        return cls._make("aw_map_split_blocks", speakers._h)

    @classmethod
    def parseHeSuViFormat(cls, text: str):
        return cls._make("aw_map_parse_text", text.encode())

    def getIndices(self, speaker: str) -> Optional[Tuple[int, int]]:
        l, r = ctypes.c_int32(), ctypes.c_int32()
        if self._lib.aw_map_get(self._h, speaker.encode(), ctypes.byref(l), ctypes.byref(r)):
            return (l.value, r.value)
        return None

    def hasMappingFor(self, speaker: str) -> bool:
        return self.getIndices(speaker) is not None

    def __len__(self):
        return self._lib.aw_map_count(self._h)

    def resolve(self, layout: InputLayout, n_tracks: int) -> Tuple[np.ndarray, np.ndarray]:
        n = len(layout.channels)
        lt = np.zeros(max(n, 1), dtype=np.int32)
        rt = np.zeros(max(n, 1), dtype=np.int32)
        _check(self._lib.aw_map_resolve(self._h, layout._h, n_tracks, _i32p(lt), _i32p(rt)))
        return lt[:n], rt[:n]


class Resampler:
    """Resampler (Resampler.swift:12-69)."""

    @staticmethod
    def resampleHighQuality(input, fromRate: float, toRate: float, literal_vgenp: bool = False) -> np.ndarray:
        """The intended interpolation out[i] = lerp(input, i * fromRate / toRate) by default; literal_vgenp=True is the
        call the reference actually makes (vDSP_vramp + vDSP_vgenp, Resampler.swift:56-65) as Apple documents vgenp."""
        lib = _capi.load()
        x = _f32(input)
        n = max(lib.aw_resample_output_count(x.size, fromRate, toRate), 0)
        out = np.zeros(max(n, 1), dtype=np.float32)
        cnt = ctypes.c_int32()
        fn = lib.aw_resample_vgenp if literal_vgenp else lib.aw_resample
        _check(fn(_fp(x), x.size, fromRate, toRate, _fp(out), out.size, ctypes.byref(cnt)))
        return out[: cnt.value]

    resample = resampleHighQuality


# ---- device objects -----------------------------------------------------------------------------------
class HRIR:
    def __init__(self, tracks, sample_rate: float = 48000.0, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        t = _f32(tracks)
        if t.ndim == 1:
            t = t[None]
        self._lib = _capi.load()
        h = ctypes.c_void_p()
        _check(self._lib.aw_hrir_create(self.ctx._h, _fp(t), t.shape[0], t.shape[1], sample_rate, ctypes.byref(h)))
        self._h = h
        self.n_tracks, self.taps = t.shape

    def __del__(self):
        if getattr(self, "_h", None) and not _finalizing():
            self._lib.aw_hrir_destroy(self._h)
            self._h = None


class Spatializer:
    """Batch engine network: S streams x (one convolution per (input channel, ear)) + stereo downmix."""

    def __init__(self, hrir: HRIR, left_track, right_track, n_streams: int = 1, ctx: Optional[Context] = None, _h=None):
        self._lib = _capi.load()
        self.ctx = ctx or (hrir.ctx if hrir is not None else default_context())
        if _h is not None:
            self._h = _h
        else:
            lt = np.ascontiguousarray(left_track, dtype=np.int32)
            rt = np.ascontiguousarray(right_track, dtype=np.int32)
            assert lt.size == rt.size
            h = ctypes.c_void_p()
            _check(self._lib.aw_spatializer_create(self.ctx._h, hrir._h, lt.size, _i32p(lt), _i32p(rt), n_streams, 0,
                                                   ctypes.byref(h)))
            self._h = h
        self.n_streams = self._lib.aw_spatializer_stream_count(self._h)
        self.n_channels = self._lib.aw_spatializer_channel_count(self._h)

    def __del__(self):
        if getattr(self, "_h", None) and not _finalizing():
            self._lib.aw_spatializer_destroy(self._h)
            self._h = None

    _ENTRY_PREFIX = "aw_spatializer_"

    def _entry(self, name: str):
        """The C entry behind a setting or a record getter: MultiSpatializer has the same ones under its own prefix."""
        return getattr(self._lib, self._ENTRY_PREFIX + name)

    def info(self) -> Dict[str, int]:
        g = lambda i: int(self._lib.aw_spatializer_info(self._h, i))
        return {"fft": g(0), "hop": g(1), "partitions": g(2), "path": g(3), "history": g(4), "dominant_frames": g(5), "scratch_bytes": g(6),
                "long_window_rows": g(7),       # long-window kernels ran in the last call on windows of rows x 4096 frames (0: they did not)
                "long_window_rows_rest": g(8),  # ... and a last, shorter window of this many rows for the remainder (0: one window length)
                "long_window_table_sets": g(9), # table sets built so far (one per window length)
                # the last reserve(): float64 table build on host threads / table upload / scratch pool growth, milliseconds
                "reserve_tables_ms": g(10) / 1e3, "reserve_upload_ms": g(11) / 1e3, "reserve_scratch_ms": g(12) / 1e3,
                "device_allocs": g(13),         # device / page-locked allocations made so far on behalf of the context's handles
                "sync_copies": g(14),           # blocking table uploads likewise
                "host_chunk_streams": g(15),    # streams per staged chunk of the last host-entry call (0: one piece)
                "overlap_add_rows": g(16),      # the last call ran the overlap-add tile on blocks of 512 x this many frames (0: it did not)
                "overlap_add_rows_policy": g(17),   # ... which this spatializer's calls do when they have enough blocks (0: never)
                "position_frames": g(18),       # frames processed since creation / the last reset (the dither's frame position)
                "metering": g(19),              # the level meter is on (set_metering)
                "gain_mode": g(20),             # aw_gain_mode of the batch entries (set_gain)
                "loudness": g(21),              # the loudness measurement is on (set_loudness)
                "true_peak": g(22),             # the true-peak measurement is on (set_true_peak)
                "limiter": g(23),               # the limiter is on (set_limiter)
                "limiter_latency": g(24),       # its latency in frames (0 while it is off)
                "equalizer": g(25),             # presets the equalizer stage holds (set_equalizer, set_equalizer_target; 0 and no fade: the stage is off)
                "equalizer_filters": g(26),     # the largest enabled-filter count among them
                "equalizer_fade": g(27),        # frames left of the running fade to a new target (set_equalizer_target); 0: none
                "equalizer_pending": g(28)}     # 1: a target is published and has not begun

    def process_device(self, in_ptr: int, out_ptr: int, frames: int) -> None:
        _check(self._lib.aw_spatializer_process(self._h, ctypes.c_void_p(in_ptr), ctypes.c_void_p(out_ptr), frames))

    def process(self, x) -> np.ndarray:
        """x: [streams][frames][channels] (or [frames][channels] for one stream) host array."""
        a = _f32(x)
        squeeze = a.ndim == 2
        if squeeze:
            a = a[None]
        S, F, C = a.shape
        assert S == self.n_streams and C == self.n_channels
        out = np.full((S, F, 2), np.nan, dtype=np.float32)
        _check(self._lib.aw_spatializer_process_host(self._h, _fp(a), _fp(out), F))
        return out[0] if squeeze else out

    def process_planar(self, input_left, input_right=None) -> Tuple[np.ndarray, np.ndarray]:
        l = _f32(input_left)
        r = None if input_right is None else _f32(input_right)
        ol = np.full(l.size, np.nan, dtype=np.float32)
        orr = np.full(l.size, np.nan, dtype=np.float32)
        _check(self._lib.aw_spatializer_process_planar(self._h, _fp(l), None if r is None else _fp(r), _fp(ol), _fp(orr), l.size))
        return ol, orr

    def reserve(self, max_frames: int) -> None:
        """Size every internal device buffer for calls of up to max_frames frames: process never allocates afterwards."""
        _check(self._lib.aw_spatializer_reserve(self._h, int(max_frames)))

    def reserve_host(self, max_frames: int) -> None:
        """reserve() plus the device-side staging of the host entry (process / process_host_into)."""
        _check(self._lib.aw_spatializer_reserve_host(self._h, int(max_frames)))

    def process_host_into(self, x: np.ndarray, out: np.ndarray, in_format=None, out_format=None) -> int:
        """Host entry on caller-owned arrays (e.g. Context.pinned_empty): x [streams][frames][channels], out [streams][frames][2].
        float32 arrays take aw_spatializer_process_host; int16 / int32 arrays (or packed s24: uint8 [..., 3] with the format named,
        in_format / out_format 's24') take aw_spatializer_process_host_pcm.  Returns the clipped-sample count (0 for float32 output)."""
        if x.dtype == np.float32 and out.dtype == np.float32 and in_format in (None, "f32", 0) and out_format in (None, "f32", 0):
            assert x.flags["C_CONTIGUOUS"] and out.flags["C_CONTIGUOUS"]
            S, F, C = x.shape
            assert S == self.n_streams and C == self.n_channels and out.shape == (S, F, 2)
            _check(self._lib.aw_spatializer_process_host(self._h, _fp(x), _fp(out), F))
            return 0
        if not isinstance(x, np.ndarray) or x.ndim < 3:
            raise ValueError("x: [streams][frames][channels] array required")
        F = x.shape[1]
        x, fi = _pcm_array(x, in_format, (self.n_streams, F, self.n_channels), "x")
        out, fo = _pcm_array(out, out_format, (self.n_streams, F, 2), "out")
        clipped = ctypes.c_uint64(0)
        _check(self._lib.aw_spatializer_process_host_pcm(self._h, ctypes.c_void_p(x.ctypes.data), fi, ctypes.c_void_p(out.ctypes.data), fo, F,
                                                         ctypes.byref(clipped)))
        return int(clipped.value)

    def process_pcm_device(self, in_ptr: int, in_format, out_ptr: int, out_format, frames: int, clipped_ptr: int = 0) -> None:
        """aw_spatializer_process_pcm on device buffers (asynchronous on the context's stream); formats by name ('f32', 's16', 's24',
        's32') or code.  clipped_ptr: 0, or a device uint64 the call adds its clipped-sample count to."""
        codes = []
        for fmt in (in_format, out_format):
            code = SAMPLE_FORMATS.get(fmt, -1) if isinstance(fmt, str) else int(fmt)
            if code not in _FORMAT_DTYPE:
                raise ValueError(f"unknown sample format {fmt!r}")
            codes.append(code)
        _check(self._lib.aw_spatializer_process_pcm(self._h, ctypes.c_void_p(in_ptr), codes[0], ctypes.c_void_p(out_ptr), codes[1], int(frames),
                                                    ctypes.c_void_p(clipped_ptr or None)))

    def reserve_pcm(self, max_frames: int, in_format, out_format) -> None:
        """reserve_host() for these sample formats: neither PCM entry allocates afterwards for calls of up to max_frames frames."""
        fi = SAMPLE_FORMATS.get(in_format, -1) if isinstance(in_format, str) else int(in_format)
        fo = SAMPLE_FORMATS.get(out_format, -1) if isinstance(out_format, str) else int(out_format)
        _check(self._lib.aw_spatializer_reserve_pcm(self._h, int(max_frames), fi, fo))

    def set_dither(self, mode, seed: int = 0, first_stream: int = 0) -> None:
        """aw_spatializer_set_dither: dither of every later s16 / s24 encode ('none', 'tpdf', 'tpdf_hp', or the aw_dither code).
        first_stream: the global index of this handle's stream 0, so that a batch sharded over handles gets one handle's noise."""
        if isinstance(mode, str):
            if mode not in DITHER_MODES:
                raise ValueError(f"unknown dither mode {mode!r} (one of {', '.join(DITHER_MODES)})")
            mode = DITHER_MODES[mode]
        _check(self._entry("set_dither")(self._h, int(mode), int(seed), int(first_stream)))

    def set_metering(self, on: bool = True) -> None:
        """aw_spatializer_set_metering: per-stream levels of every later batch call (process, process_host_into, the PCM entries).
        Switching it on allocates the records here, not on the process path."""
        _check(self._entry("set_metering")(self._h, int(bool(on))))

    def levels(self, first_stream: int = 0, n: Optional[int] = None) -> np.ndarray:
        """aw_spatializer_get_levels: the records of n streams from first_stream on (default: all) as a structured array of
        LEVELS_DTYPE (peak[2], gain, energy[2], frames, clipped, nonfinite).  Synchronises the context's stream."""
        first_stream = int(first_stream)
        n = self.n_streams - first_stream if n is None else int(n)
        if first_stream < 0 or n < 0 or first_stream + n > self.n_streams:
            raise ValueError(f"streams [{first_stream}, {first_stream + n}) outside [0, {self.n_streams})")
        out = np.zeros(n, LEVELS_DTYPE)
        _check(self._entry("get_levels")(self._h, first_stream, n, ctypes.c_void_p(out.ctypes.data)))
        return out

    def reset_levels(self) -> None:
        _check(self._entry("reset_levels")(self._h))

    def set_gain(self, mode, gains=None, ceiling: Optional[float] = None) -> None:
        """aw_spatializer_set_gain: 'none'; 'fixed' with one gain (every stream) or one per stream; 'peak_ceiling' with 0 < ceiling <= 1,
        which scales every stream of every call down to the ceiling where that call's peak exceeds it; 'true_peak_ceiling' likewise over
        the call's true peak (or the aw_gain_mode code)."""
        if isinstance(mode, str):
            if mode not in GAIN_MODES:
                raise ValueError(f"unknown gain mode {mode!r} (one of {', '.join(GAIN_MODES)})")
            mode = GAIN_MODES[mode]
        mode = int(mode)
        if mode not in GAIN_MODES.values():
            raise ValueError(f"unknown gain mode {mode}")
        g, c = None, 0.0
        if mode == GAIN_MODES["fixed"]:
            if gains is None:
                raise ValueError("fixed gain needs gains")
            g = np.ascontiguousarray(np.atleast_1d(np.asarray(gains, np.float32)))
            if g.ndim != 1 or g.size not in (1, self.n_streams):
                raise ValueError(f"gains must be 1 or {self.n_streams} values, got shape {g.shape}")
            if not np.all(np.isfinite(g)):
                raise ValueError("gains must be finite")
        elif mode in (GAIN_MODES["peak_ceiling"], GAIN_MODES["true_peak_ceiling"]):
            if ceiling is None or not (0.0 < float(np.float32(ceiling)) <= 1.0):
                raise ValueError(f"a ceiling gain needs 0 < ceiling <= 1, got {ceiling!r}")
            c = float(ceiling)
        _check(self._entry("set_gain")(self._h, mode, None if g is None else _fp(g), 0 if g is None else int(g.size), ctypes.c_float(c)))

    def set_loudness(self, on: bool = True, max_seconds: float = 0.0) -> None:
        """aw_spatializer_set_loudness: BS.1770 integrated loudness of every later batch call, per stream, measured before the gain.
        Switching it on allocates the hop energies of max_seconds per stream here, not on the process path."""
        if on and not (np.isfinite(max_seconds) and max_seconds > 0):
            raise ValueError(f"max_seconds must be finite and positive, got {max_seconds!r}")
        _check(self._entry("set_loudness")(self._h, int(bool(on)), float(max_seconds)))

    def loudness(self, first_stream: int = 0, n: Optional[int] = None) -> np.ndarray:
        """aw_spatializer_get_loudness: the gated loudness of n streams from first_stream on (default: all) as a structured array of
        LOUDNESS_DTYPE.  Synchronises the context's stream."""
        first_stream = int(first_stream)
        n = self.n_streams - first_stream if n is None else int(n)
        if first_stream < 0 or n < 0 or first_stream + n > self.n_streams:
            raise ValueError(f"streams [{first_stream}, {first_stream + n}) outside [0, {self.n_streams})")
        out = np.zeros(n, LOUDNESS_DTYPE)
        _check(self._entry("get_loudness")(self._h, first_stream, n, ctypes.c_void_p(out.ctypes.data)))
        return out

    def loudness_hops(self, stream: int, first_hop: int, n: int) -> np.ndarray:
        """aw_spatializer_get_loudness_hops: the raw 100 ms hop energies [first_hop, first_hop + n) of one stream (float64)."""
        stream, first_hop, n = int(stream), int(first_hop), int(n)
        if not 0 <= stream < self.n_streams or first_hop < 0 or n < 0:
            raise ValueError(f"stream {stream}, hops [{first_hop}, {first_hop + n}) out of range")
        out = np.zeros(n, np.float64)
        _check(self._entry("get_loudness_hops")(self._h, stream, first_hop, n, ctypes.c_void_p(out.ctypes.data)))
        return out

    def set_true_peak(self, on: bool = True) -> None:
        """aw_spatializer_set_true_peak: the true peak (4x oversampled) of every later batch call, per stream, measured before the gain.
        Switching it on allocates the records here, not on the process path."""
        _check(self._entry("set_true_peak")(self._h, int(bool(on))))

    def true_peak(self, first_stream: int = 0, n: Optional[int] = None) -> np.ndarray:
        """aw_spatializer_get_true_peak: the records of n streams from first_stream on (default: all) as a structured array of
        TRUE_PEAK_DTYPE.  Synchronises the context's stream."""
        first_stream = int(first_stream)
        n = self.n_streams - first_stream if n is None else int(n)
        if first_stream < 0 or n < 0 or first_stream + n > self.n_streams:
            raise ValueError(f"streams [{first_stream}, {first_stream + n}) outside [0, {self.n_streams})")
        out = np.zeros(n, TRUE_PEAK_DTYPE)
        _check(self._entry("get_true_peak")(self._h, first_stream, n, ctypes.c_void_p(out.ctypes.data)))
        return out

    def set_limiter(self, on: bool = True, ceiling: float = 1.0, attack_frames: int = 64, hold_frames: int = 128) -> None:
        """aw_spatializer_set_limiter: a look-ahead true-peak limiter on the output of every later batch call, behind the fixed gain;
        0 < ceiling <= 1, 16 <= attack_frames <= 512, 0 <= hold_frames <= 1024.  The output is attack_frames + 11 frames late
        (info()['limiter_latency']).  Switching it on allocates here, not on the process path."""
        _check(self._entry("set_limiter")(self._h, int(bool(on)), ctypes.c_float(ceiling), int(attack_frames), int(hold_frames)))

    def limiter(self, first_stream: int = 0, n: Optional[int] = None) -> np.ndarray:
        """aw_spatializer_get_limiter: the records of n streams from first_stream on (default: all) as a structured array of
        LIMITER_DTYPE.  Synchronises the context's stream."""
        first_stream = int(first_stream)
        n = self.n_streams - first_stream if n is None else int(n)
        if first_stream < 0 or n < 0 or first_stream + n > self.n_streams:
            raise ValueError(f"streams [{first_stream}, {first_stream + n}) outside [0, {self.n_streams})")
        out = np.zeros(n, LIMITER_DTYPE)
        _check(self._entry("get_limiter")(self._h, first_stream, n, ctypes.c_void_p(out.ctypes.data)))
        return out

    def set_equalizer(self, definitions, stream_definition=None) -> None:
        """aw_spatializer_set_equalizer: the equalizer stage of every later batch call, between the convolution and the first meter.
        definitions: the presets (EqualizerDefinition; one alone is taken as a list of one; none or an empty list: the stage is off);
        stream_definition: per stream the index of its preset, -1 = not equalized (None: every stream takes preset 0).  Allocates and
        uploads here, not on the process path, and starts the filter state from zero.  A preset that cannot be prepared raises
        ParametricEqualizerPreparationError, as ParametricEqualizerState does; the previous stage then stays."""
        self._set_equalizer(self._entry("set_equalizer"), definitions, stream_definition)

    def set_equalizer_target(self, definitions, stream_definition=None) -> None:
        """aw_spatializer_set_equalizer_target: publishes a target that the equalizer stage fades to over max(1, round(0.020 * rate))
        frames, from the first frame of the next batch call on (or from where a running fade ends).  definitions as set_equalizer's;
        stream_definition: per stream the index of its target, -1 = fade to unity, EQ_KEEP = the stream is not part of the change (None:
        every stream takes definition 0).  A stage that is off counts as every stream at -1.  Allocates, uploads and synchronises here,
        not on the process path; info()['equalizer_fade'] / ['equalizer_pending'] follow the fade.  A failing call changes nothing."""
        self._set_equalizer(self._entry("set_equalizer_target"), definitions, stream_definition)

    def _set_equalizer(self, entry, definitions, stream_definition) -> None:
        from .eq import _DefHandle, _check_eq            # (eq.py imports this module)
        if definitions is None:
            definitions = []
        elif not isinstance(definitions, (list, tuple)):
            definitions = [definitions]
        sd = None
        if stream_definition is not None:
            sd = np.ascontiguousarray(stream_definition, dtype=np.int32)
            if sd.shape != (self.n_streams,):
                raise ValueError(f"stream_definition needs one entry per stream ({self.n_streams}), got shape {sd.shape}")
        handles = []
        try:
            for d in definitions:
                handles.append(_DefHandle(d))
            if any(h.h is None for h in handles):
                raise ValueError("a definition is None (map the stream to -1 instead)")
            arr = (ctypes.c_void_p * max(len(handles), 1))(*[h.h for h in handles])
            _check_eq(entry(self._h, ctypes.cast(arr, _capi.c_void_pp) if handles else None, len(handles), None if sd is None else _i32p(sd)))
        finally:
            for h in handles:
                h.__exit__()

    def reset(self) -> None:
        _check(self._lib.aw_spatializer_reset(self._h))

    def set_profiling(self, on: bool) -> None:
        _check(self._lib.aw_spatializer_set_profiling(self._h, int(on)))

    def kernel_time(self) -> Tuple[int, float, str]:
        ms = ctypes.c_double()
        name = ctypes.c_char_p()
        n = self._lib.aw_spatializer_kernel_time(self._h, ctypes.byref(ms), ctypes.byref(name))
        return n, float(ms.value), (name.value or b"").decode()

    def stage_times(self) -> List[Tuple[str, float, int]]:
        """(kernel name, total ms, launches) of every separately timed launch since profiling was switched on."""
        out = []
        i = 0
        while True:
            name, ms, n = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int32()
            if not self._lib.aw_spatializer_stage_time(self._h, i, ctypes.byref(name), ctypes.byref(ms), ctypes.byref(n)):
                return out
            out.append(((name.value or b"").decode(), float(ms.value), int(n.value)))
            i += 1


def device_count() -> int:
    """aw_device_count: visible HIP devices; 0 when there is none or no driver."""
    return int(_capi.load().aw_device_count())


def device_info(ordinal: int) -> Dict[str, object]:
    """aw_device_info: name, arch, compute_units, total_bytes and free_bytes of one device (AW_ERR_NO_DEVICE for an ordinal out of range)."""
    d = _capi.DeviceInfo()
    _check(_capi.load().aw_device_info(int(ordinal), ctypes.byref(d)))
    return {"name": d.name.decode("utf-8", "replace"), "arch": d.arch.decode("utf-8", "replace"), "compute_units": int(d.compute_units),
            "total_bytes": int(d.total_bytes), "free_bytes": int(d.free_bytes)}


class _MultiPinnedOwner:
    """_PinnedOwner for aw_multi_alloc_pinned: page-locked memory every device of the handle can DMA."""

    def __init__(self, multi: "MultiSpatializer", ptr: int, nbytes: int):
        self._multi, self._ptr = multi, ptr
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    def __del__(self):
        try:
            if self._ptr and getattr(self._multi, "_h", None) and not _finalizing():
                self._multi._lib.aw_multi_free_pinned(self._multi._h, ctypes.c_void_p(self._ptr))
        finally:
            self._ptr = 0


class MultiSpatializer(Spatializer):
    """aw_multi: the batch spatializer over several devices behind one handle.  devices: one ordinal per shard (an ordinal may repeat:
    several contexts on one device); shard i owns sharding.shard_streams(n_streams, len(devices), i).  The Spatializer methods of the same
    name, over host arrays laid out as one handle of n_streams streams takes them; per-stream settings and records are sliced and
    gathered across the shards.  Bit-exact against separately driven handles of the shards' stream counts, not against one big handle."""

    _ENTRY_PREFIX = "aw_multi_"          # set_dither .. set_equalizer_target, levels .. limiter: Spatializer's methods over the multi entries

    def __init__(self, devices: Sequence[int], hrir_tracks, sample_rate: float, left_track, right_track, n_streams: int):
        self._lib = _capi.load()
        dev = np.ascontiguousarray(devices, dtype=np.int32).reshape(-1)
        t = _f32(hrir_tracks)
        if t.ndim == 1:
            t = t[None]
        lt = np.ascontiguousarray(left_track, dtype=np.int32)
        rt = np.ascontiguousarray(right_track, dtype=np.int32)
        assert lt.size == rt.size
        h = ctypes.c_void_p()
        _check(self._lib.aw_multi_create(_i32p(dev) if dev.size else None, int(dev.size), _fp(t), t.shape[0], t.shape[1], float(sample_rate), int(lt.size),
                                         _i32p(lt), _i32p(rt), int(n_streams), 0, ctypes.byref(h)))
        self._h = h
        self.ctx = None
        self.devices = [int(d) for d in dev]
        self.n_streams = int(self._lib.aw_multi_stream_count(self._h))
        self.n_channels = int(self._lib.aw_multi_channel_count(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and not _finalizing():
            self._lib.aw_multi_destroy(self._h)
            self._h = None

    def shards(self) -> List[Dict[str, int]]:
        """One entry per device of the list: ordinal, first_stream, count (0: an empty shard, which owns nothing)."""
        out = []
        for i in range(self._lib.aw_multi_shard_count(self._h)):
            o, f, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
            _check(self._lib.aw_multi_shard(self._h, i, ctypes.byref(o), ctypes.byref(f), ctypes.byref(c)))
            out.append({"ordinal": int(o.value), "first_stream": int(f.value), "count": int(c.value)})
        return out

    def shard_info(self, shard: int) -> Optional[Dict[str, int]]:
        """Spatializer.info() of one shard through its borrowed handle; None for an empty shard."""
        h = self._lib.aw_multi_spatializer(self._h, int(shard))
        if not h:
            return None
        view = Spatializer.__new__(Spatializer)
        view._lib, view._h = self._lib, ctypes.c_void_p(h)
        try:
            return view.info()
        finally:
            view._h = None          # borrowed: never destroyed from here

    def info(self) -> Dict[str, int]:
        raise NotImplementedError("a MultiSpatializer has one info() per shard: shard_info(i)")

    def pinned_empty(self, shape, dtype=np.float32) -> np.ndarray:
        """A numpy array over page-locked host memory that every device of the handle can DMA (aw_multi_alloc_pinned)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        _check(self._lib.aw_multi_alloc_pinned(self._h, n, ctypes.byref(p)))
        owner = _MultiPinnedOwner(self, p.value, max(n, 1))
        return np.asarray(owner)[:n].view(dtype).reshape(shape)

    def process(self, x) -> np.ndarray:
        """x: [streams][frames][channels] float32 host array; returns [streams][frames][2]."""
        a = _f32(x)
        S, F, C = a.shape
        assert S == self.n_streams and C == self.n_channels
        out = np.full((S, F, 2), np.nan, dtype=np.float32)
        self.process_host_into(a, out)
        return out

    def process_host_into(self, x: np.ndarray, out: np.ndarray, in_format=None, out_format=None) -> int:
        """aw_multi_process_host_pcm on caller-owned arrays (e.g. pinned_empty), formats as Spatializer.process_host_into; returns the
        clipped-sample count summed over the shards."""
        if not isinstance(x, np.ndarray) or x.ndim < 3:
            raise ValueError("x: [streams][frames][channels] array required")
        F = x.shape[1]
        x, fi = _pcm_array(x, in_format, (self.n_streams, F, self.n_channels), "x")
        out, fo = _pcm_array(out, out_format, (self.n_streams, F, 2), "out")
        clipped = ctypes.c_uint64(0)
        _check(self._lib.aw_multi_process_host_pcm(self._h, ctypes.c_void_p(x.ctypes.data), fi, ctypes.c_void_p(out.ctypes.data), fo, F, ctypes.byref(clipped)))
        return int(clipped.value)

    def reserve_pcm(self, max_frames: int, in_format="f32", out_format="f32") -> None:
        fi = SAMPLE_FORMATS.get(in_format, -1) if isinstance(in_format, str) else int(in_format)
        fo = SAMPLE_FORMATS.get(out_format, -1) if isinstance(out_format, str) else int(out_format)
        _check(self._lib.aw_multi_reserve_pcm(self._h, int(max_frames), fi, fo))

    def reset(self) -> None:
        _check(self._lib.aw_multi_reset(self._h))

    # the entries of one handle that the multi handle does not have
    def _not_here(self, *a, **k):
        raise NotImplementedError("not an entry of the multi-device handle (host buffers only)")

    process_device = process_planar = process_pcm_device = reserve = reserve_host = set_profiling = kernel_time = stage_times = _not_here


class ConvolutionEngine:
    """ConvolutionEngine (ConvolutionEngine.swift:14-408) on the GPU."""

    def __init__(self, hrirSamples, blockSize: int = 512, ctx: Optional[Context] = None):
        self._lib = _capi.load()
        self.ctx = ctx or default_context()
        h = _f32(hrirSamples)
        e = ctypes.c_void_p()
        _check(self._lib.aw_engine_create(self.ctx._h, _fp(h), h.size, blockSize, ctypes.byref(e)))
        self._h = e
        self.blockSize = blockSize

    def __del__(self):
        if getattr(self, "_h", None) and not _finalizing():
            self._lib.aw_engine_destroy(self._h)
            self._h = None

    def process(self, input, frameCount: Optional[int] = None) -> Optional[np.ndarray]:
        """process(input:output:frameCount:) — returns None (output untouched) when count != blockSize,
        like the Swift wrapper's silent return (ConvolutionEngine.swift:370-373)."""
        x = _f32(input)
        count = self.blockSize if frameCount is None else frameCount
        out = np.zeros(self.blockSize, dtype=np.float32)
        st = self._lib.aw_engine_process_n(self._h, _fp(x), _fp(out), count)
        if st == 11:
            return None
        _check(st)
        return out

    def processAndAccumulate(self, input, outputAccumulator: np.ndarray) -> None:
        x = _f32(input)
        assert outputAccumulator.dtype == np.float32 and outputAccumulator.size == self.blockSize
        _check(self._lib.aw_engine_process_accumulate(self._h, _fp(x), _fp(outputAccumulator)))

    def reset(self) -> None:
        _check(self._lib.aw_engine_reset(self._h))


class RealtimeAudioProcessor:
    """RealtimeAudioProcessor (RealtimeAudioProcessor.swift:11-191).  renderers: [(leftTrack, rightTrack)]
    index pairs into `hrir` (the VirtualSpeakerRenderer's two engines)."""

    def __init__(self, hrir: HRIR, renderers: Sequence[Tuple[int, int]], blockSize: int = 512,
                 maxFramesPerCallback: int = 4096):
        self._lib = _capi.load()
        self.ctx = hrir.ctx
        lt = np.ascontiguousarray([r[0] for r in renderers] or [0], dtype=np.int32)
        rt = np.ascontiguousarray([r[1] for r in renderers] or [0], dtype=np.int32)
        h = ctypes.c_void_p()
        _check(self._lib.aw_realtime_create(self.ctx._h, hrir._h, len(renderers), _i32p(lt), _i32p(rt), blockSize,
                                            maxFramesPerCallback, ctypes.byref(h)))
        self._h = h
        self.blockSize, self.maxFramesPerCallback = blockSize, maxFramesPerCallback

    def __del__(self):
        if getattr(self, "_h", None) and not _finalizing():
            self._lib.aw_realtime_destroy(self._h)
            self._h = None

    def process(self, inputLeft, inputRight=None, outputLeft: Optional[np.ndarray] = None,
                outputRight: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        l = _f32(inputLeft)
        r = None if inputRight is None else _f32(inputRight)
        n = l.size
        ol = outputLeft if outputLeft is not None else np.full(n, np.nan, dtype=np.float32)
        orr = outputRight if outputRight is not None else np.full(n, np.nan, dtype=np.float32)
        _check(self._lib.aw_realtime_process(self._h, _fp(l), None if r is None else _fp(r), _fp(ol), _fp(orr), n))
        return ol, orr

    def reset(self) -> None:
        _check(self._lib.aw_realtime_reset(self._h))

    def info(self) -> Dict[str, int]:
        """What the processor holds (all of it allocated in __init__, like RealtimeAudioProcessor.init, :30-62)."""
        g = lambda i: int(self._lib.aw_realtime_info(self._h, i))
        return {"host_bytes": g(0), "device_bytes": g(1), "device_allocs": g(2)}


class HRIRManager:
    """The activation + processing part of HRIRManager (HRIRManager.swift:316-449, 531-568):
    activatePreset builds the renderer network; process is the StereoAudioProcessing entry
    (AudioPipeline.swift:3-28) with passthrough when no preset is active."""

    def __init__(self, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self._lib = _capi.load()
        self.spatializer: Optional[Spatializer] = None
        self.errorMessage: Optional[str] = None

    @property
    def isReady(self) -> bool:                                   # AudioSpatialEffect.isReady
        return self.spatializer is not None

    isConvolutionActive = isReady

    def activatePreset(self, fileURL: str, targetSampleRate: float, inputLayout: InputLayout,
                       hrirMap: Optional[HRIRChannelMap] = None, n_streams: int = 1) -> Spatializer:
        sp = ctypes.c_void_p()
        st = self._lib.aw_preset_activate(self.ctx._h, fileURL.encode(), targetSampleRate, inputLayout._h,
                                          hrirMap._h if hrirMap is not None else None, n_streams, ctypes.byref(sp), None)
        if st != AW_OK:
            msg = (self._lib.aw_last_error_message() or b"").decode()
            self.errorMessage = "Failed to activate preset: " + msg       # HRIRManager.swift:441
            _check(st)
        self.errorMessage = None
        self.spatializer = Spatializer(None, None, None, ctx=self.ctx, _h=sp)
        return self.spatializer

    def deactivatePreset(self) -> None:
        self.spatializer = None

    def process(self, inputLeft, inputRight=None) -> Tuple[np.ndarray, np.ndarray]:
        if self.spatializer is None:                               # passthrough, HRIRManager.swift:550-559
            l = _f32(inputLeft)
            return l.copy(), (l.copy() if inputRight is None else _f32(inputRight).copy())
        return self.spatializer.process_planar(inputLeft, inputRight)

    def resetConvolutionState(self) -> None:
        if self.spatializer is not None:
            self.spatializer.reset()
