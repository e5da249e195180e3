"""Mixed-rate batches (BASELINE cfg 5): streams are bucketed by sample rate and every
bucket gets its own renderer network built exactly as HRIRManager.activatePreset builds one for an output
device of that rate — the HRIR (not the audio) is resampled to the stream rate with Resampler
(HRIRManager.swift:389-403, Resampler.swift:31-68) — so one preset serves 44.1/48/96 kHz streams side by
side.  Host-side orchestration over the kernels of the convolution path; nothing here touches samples."""
from __future__ import annotations

import sys
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from .api import Context, HRIR, HRIRChannelMap, InputLayout, Resampler, Spatializer, default_context


@dataclass
class RateBucket:
    sample_rate: float
    stream_ids: List[int]            # positions in the caller's stream list, in order
    hrir_taps: int                   # taps of the tracks the spatializer convolves with (HRIR resampled to the rate, equalizer folded in if it was)
    spatializer: Spatializer
    equalizer: Optional[object] = None      # ParametricEqualizerState that runs AFTER the spatializer (None: no equalizer, folded into the HRIR, or the spatializer's own stage)
    eq_response_taps: int = 0        # equalizer folded into the HRIR: samples of its impulse response that were kept (0: not folded)
    eq_tail_bound: float = 0.0       # ... and the bound on what the cut can change, relative to the spatializer output's peak
    converter: Optional[object] = None      # RateConverter (two channels) behind the spatializer and its trailing equalizer: the bucket leaves at output_rate
    stage: int = 0                   # device staging of the bucket's stereo output at its own rate, in front of the converter (grow-only)
    stage_bytes: int = 0


# An equalizer is folded into the HRIR (fold=None, the default) when that is the cheaper form: the folded HRIR is longer by the
# equalizer's response (thousands of taps for a low shelf at 100 Hz), which only lengthens the window overlap of the long-window kernels
# (cfg 4: 8640 -> 22 464 taps, +7 % of three memory-bound launches, against a Float64 cascade pass of 40 % of the step) but would push a
# short HRIR off the on-chip tile.  So: fold when the HRIR alone is already beyond the fused tiles, or when the folded one still fits them.
FUSED_TILE_TAPS = 5121


def _fold_pays(hrir_taps: int, folded_taps: int) -> bool:
    return hrir_taps > FUSED_TILE_TAPS or folded_taps <= FUSED_TILE_TAPS


def bucket_by_rate(stream_rates: Sequence[float]) -> Dict[float, List[int]]:
    """Stable bucketing: rates in first-appearance order, stream ids ascending inside a bucket."""
    buckets: Dict[float, List[int]] = {}
    for i, r in enumerate(stream_rates):
        buckets.setdefault(float(r), []).append(i)
    return buckets


def resample_tracks(tracks: np.ndarray, from_rate: float, to_rate: float, literal_vgenp: bool = False) -> np.ndarray:
    """Every HRIR track through Resampler.resampleHighQuality (identity when the rates agree, :33-35)."""
    if from_rate == to_rate:
        return np.ascontiguousarray(tracks, dtype=np.float32)
    return np.stack([Resampler.resampleHighQuality(t, from_rate, to_rate, literal_vgenp=literal_vgenp) for t in tracks])


class MixedRateBatch:
    """One preset, streams at several sample rates: `buckets[rate].spatializer` convolves that rate's streams."""

    def __init__(self, tracks, hrir_rate: float, layout: InputLayout, stream_rates: Sequence[float],
                 hrirMap: Optional[HRIRChannelMap] = None, ctx: Optional[Context] = None, literal_vgenp: bool = False,
                 equalizer=None, fold_equalizer: Optional[bool] = None, eq_tail_tolerance: float = 1e-7, eq_max_taps: int = 65536,
                 stream_equalizers=None, output_rate: Optional[float] = None, output_true_peak_ceiling: Optional[float] = None):
        """equalizer: an EqualizerDefinition applied after the spatializer, as AudioEffectGraph orders the two effects
        (AudioEffectGraph.swift:195-211).  fold_equalizer: True = folded into the HRIR (aw_eq_fold_hrir; raises EqualizerNotFoldable
        if its response is too long), False = the cascade kernel after the spatializer, None = whichever is cheaper (see _fold_pays),
        the cascade if it cannot be folded.
        stream_equalizers: instead of `equalizer`, one EqualizerDefinition or None per stream, in the caller's order (one headphone
        preset per output device, DeviceProfileManager): every bucket's spatializer runs them as its equalizer stage
        (Spatializer.set_equalizer), the bucket's distinct definitions being the presets.  Never folded: the HRIR is shared.
        output_rate: every stream leaves at this rate: a bucket at another rate gets a two-channel RateConverter (aw_rateconv, a
        Kaiser-windowed sinc on the audio — not the HRIR's linear interpolation) behind its spatializer and its trailing equalizer.  None:
        every stream leaves at the rate it came in with.
        output_true_peak_ceiling (linear full scale; needs output_rate): process() holds the true peak of every CONVERTED stream, measured
        behind the converter, at or below it — a measuring pass over the bucket's device staging (RateConverter.measure_device), the
        per-stream gains min(1, ceiling / true peak), then the converting pass.  Buckets already at output_rate have no converter and are
        left as they are (a ceiling on them is the spatializer's own: Spatializer.set_gain('true_peak_ceiling')).  process_device is
        untouched."""
        from .rateconv import RateConverter
        from .eq import EqualizerNotFoldable, ParametricEqualizerState, fold_equalizer as fold
        if equalizer is not None and stream_equalizers is not None:
            raise ValueError("equalizer= and stream_equalizers= are mutually exclusive")
        if stream_equalizers is not None and len(stream_equalizers) != len(stream_rates):
            raise ValueError(f"stream_equalizers needs one entry per stream ({len(stream_rates)}), got {len(stream_equalizers)}")
        self.ctx = ctx or default_context()
        self.output_rate = None if output_rate is None else float(output_rate)
        if output_true_peak_ceiling is not None and (self.output_rate is None or not (float(output_true_peak_ceiling) > 0.0)):
            raise ValueError("output_true_peak_ceiling needs an output_rate and must be positive")
        self.output_true_peak_ceiling = None if output_true_peak_ceiling is None else float(output_true_peak_ceiling)
        tracks = np.ascontiguousarray(tracks, dtype=np.float32)
        # the reference's chooser: 7-track files take the 7-channel map, everything else the 14-channel one
        # (HRIRManager.swift:355-360; aw_preset_activate does the same) — an 8..13-track HRIR then fails the bounds check
        cmap = hrirMap or (HRIRChannelMap.hesuvi7Channel(layout) if tracks.shape[0] == 7 else HRIRChannelMap.hesuvi14Channel(layout))
        lt, rt = cmap.resolve(layout, tracks.shape[0])
        self.left_track, self.right_track = lt, rt
        self.buckets: Dict[float, RateBucket] = {}
        for rate, ids in bucket_by_rate(stream_rates).items():
            tr = resample_tracks(tracks, hrir_rate, rate, literal_vgenp=literal_vgenp)     # literal_vgenp: what the shipped reference computes
            eq_state, folded = None, None
            if equalizer is not None and fold_equalizer is not False:
                try:
                    f = fold(tr, equalizer, rate, tailTolerance=eq_tail_tolerance, maxTaps=eq_max_taps)
                    if fold_equalizer or _fold_pays(int(tr.shape[1]), int(f.tracks.shape[1])):
                        folded, tr = f, f.tracks
                except EqualizerNotFoldable:
                    if fold_equalizer:
                        raise
            if equalizer is not None and folded is None:
                eq_state = ParametricEqualizerState(equalizer, float(rate), n_streams=len(ids), ctx=self.ctx)
            sp = Spatializer(HRIR(tr, rate, ctx=self.ctx), lt, rt, n_streams=len(ids), ctx=self.ctx)
            if stream_equalizers is not None:
                presets, which = [], []
                for i in ids:
                    d = stream_equalizers[i]
                    if d is not None and d not in presets:
                        presets.append(d)
                    which.append(-1 if d is None else presets.index(d))
                sp.set_equalizer(presets, which if presets else None)
            conv = None
            if self.output_rate is not None and rate != self.output_rate:
                conv = RateConverter(rate, self.output_rate, len(ids), 2, ctx=self.ctx)
            self.buckets[rate] = RateBucket(rate, ids, int(tr.shape[1]), sp, eq_state, folded.responseTaps if folded else 0, folded.tailBound if folded else 0.0,
                                            conv)

    KEEP = "keep"          # retarget_equalizers: the stream is not part of the change

    def retarget_equalizers(self, stream_equalizers) -> None:
        """A target change of the buckets' equalizer stages (Spatializer.set_equalizer_target): one EqualizerDefinition (fade to it), None
        (fade to unity) or MixedRateBatch.KEEP per stream, in the caller's order.  Every bucket fades over 20 ms at its own rate, from its
        next call on; a bucket whose streams all keep is left alone, and a bucket without a stage starts at unity.  Not for a batch made
        with equalizer=: its equalizer is folded or trails the spatializer as one state."""
        if len(stream_equalizers) != sum(len(b.stream_ids) for b in self.buckets.values()):
            raise ValueError("retarget_equalizers needs one entry per stream")
        if any(b.equalizer is not None or b.eq_response_taps for b in self.buckets.values()):
            raise ValueError("this batch was made with equalizer=: its equalizer cannot be retargeted per stream")
        from .api import EQ_KEEP
        for b in self.buckets.values():
            presets, which = [], []
            for i in b.stream_ids:
                d = stream_equalizers[i]
                if isinstance(d, str) and d == self.KEEP:
                    which.append(EQ_KEEP)
                    continue
                if d is not None and d not in presets:
                    presets.append(d)
                which.append(-1 if d is None else presets.index(d))
            if any(w != EQ_KEEP for w in which):
                b.spatializer.set_equalizer_target(presets, which)

    def __del__(self):
        if sys.is_finalizing() or not getattr(getattr(self, "ctx", None), "_h", None):
            return
        for b in getattr(self, "buckets", {}).values():
            if b.stage:
                self.ctx.synchronize()
                self.ctx.free(b.stage)
                b.stage, b.stage_bytes = 0, 0

    def reserve_output_staging(self, frames: Dict[float, int]) -> None:
        """output_rate: sizes the staging in front of every converter for calls of up to frames[rate] frames, so that process_device
        allocates nothing afterwards."""
        for rate, b in self.buckets.items():
            need = len(b.stream_ids) * int(frames.get(rate, 0)) * 2 * 4
            if b.converter is not None and need > b.stage_bytes:
                if b.stage:
                    self.ctx.synchronize()
                    self.ctx.free(b.stage)
                b.stage, b.stage_bytes = self.ctx.alloc(need), need

    def process_device(self, in_ptrs: Dict[float, int], out_ptrs: Dict[float, int], frames: Dict[float, int],
                       out_capacities: Optional[Dict[float, int]] = None) -> Optional[Dict[float, int]]:
        """Per-rate device buffers ([bucket streams][frames][C] -> [..][frames][2]); all launches are queued on
        the context stream, buckets back to back.
        output_rate: a converted bucket writes [bucket streams][n][2] at output_rate, dense in the n frames this call produced (what
        converter.output_frames(frames) said; the rest follows with later calls or flush_device), and needs out_capacities[rate] >= n;
        the other buckets write `frames` frames as before.  Returns the counts per rate (None without output_rate)."""
        if self.output_rate is not None:
            self.reserve_output_staging(frames)
        counts: Dict[float, int] = {}
        for rate, b in self.buckets.items():
            y = b.stage if b.converter is not None else out_ptrs[rate]
            b.spatializer.process_device(in_ptrs[rate], y, frames[rate])
            if b.equalizer is not None:
                b.equalizer.process_device(y, y, frames[rate])      # in place, same stream
            counts[rate] = frames[rate]
            if b.converter is not None:
                counts[rate] = b.converter.process_device(y, frames[rate], out_ptrs[rate], (out_capacities or {}).get(rate, 0))
        return counts if self.output_rate is not None else None

    def flush_device(self, out_ptrs: Dict[float, int], out_capacities: Dict[float, int]) -> Dict[float, int]:
        """output_rate: the frames every converter still owes for its input so far, [bucket streams][n][2] per converted rate; the
        converters start over.  Returns the counts per converted rate."""
        return {rate: b.converter.flush_device(out_ptrs[rate], out_capacities[rate]) for rate, b in self.buckets.items() if b.converter is not None}

    def process(self, streams: Sequence[np.ndarray], stream_rates: Sequence[float]) -> List[np.ndarray]:
        """Host convenience for tests: streams[i] is [frames_i][C] at stream_rates[i]; streams of one bucket must
        have equal length.  Returns the stereo outputs in the caller's order — with output_rate, every stream at that rate and
        flushed: ceil(frames_i L / M) frames for a stream of a converted bucket."""
        out: List[Optional[np.ndarray]] = [None] * len(streams)
        for rate, b in self.buckets.items():
            x = np.stack([np.asarray(streams[i], dtype=np.float32) for i in b.stream_ids])
            y = b.spatializer.process(x)
            if b.equalizer is not None:
                y = b.equalizer.process_batch(y)
            if b.converter is not None and self.output_true_peak_ceiling is not None and y.shape[1] > 0:
                y = self._convert_under_ceiling(rate, b, np.ascontiguousarray(y, dtype=np.float32))
            elif b.converter is not None:
                y = np.concatenate([b.converter.process(y), b.converter.flush()], axis=1)
            for k, i in enumerate(b.stream_ids):
                out[i] = y[k]
        return out  # type: ignore[return-value]

    def _convert_under_ceiling(self, rate: float, b: RateBucket, y: np.ndarray) -> np.ndarray:
        """process(): y [bucket streams][frames][2] through the bucket's converter in two passes from the device staging — measure and
        measure_flush, the ceiling's gains, then process and flush to float32."""
        c, frames = b.converter, y.shape[1]
        self.reserve_output_staging({rate: frames})
        self.ctx.h2d(b.stage, y)
        c.reset_true_peak()
        c.set_true_peak(True)
        try:
            c.measure_device(b.stage, "f32", frames)
            c.measure_flush_device()
            c.set_gain("fixed", c.ceiling_gains(self.output_true_peak_ceiling))
            c.set_true_peak(False)
            head = c._pcm_to_host(lambda d, cap, clip: c.process_pcm_device(b.stage, "f32", frames, d, "f32", cap, clip), c.output_frames(frames), 0)[0]
            return np.concatenate([head, c.flush_pcm("f32")[0]], axis=1)
        finally:
            c.set_true_peak(False)
            c.set_gain("none")

    def reset(self) -> None:
        for b in self.buckets.values():
            b.spatializer.reset()
            if b.equalizer is not None:
                b.equalizer.reset()
            if b.converter is not None:
                b.converter.reset()
