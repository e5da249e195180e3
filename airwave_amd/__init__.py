"""airwave_amd — MI355X-native batch HRIR spatializer (drop-in for Airwave's ConvolutionEngine path).

The product is libairwave_hip.so (hand-written HIP for gfx950 behind the C ABI of
include/airwave_hip.h).  This package is the Python host mirror of the reference's Swift operator
surface over that ABI.  Importing it loads the library; a missing build is an ImportError
(there is no CPU fallback).
"""
from . import _capi

_capi.load()

from .api import (  # noqa: E402
    AirwaveError, Context, ConvolutionEngine, DITHER_MODES, GAIN_MODES, HRIR, HRIRChannelMap, HRIRError, HRIRManager, InputLayout, LEVELS_DTYPE,
    LOUDNESS_DTYPE, loudness_gain, TRUE_PEAK_DTYPE, true_peak_filter, LIMITER_DTYPE,
    RealtimeAudioProcessor, Resampler, SAMPLE_FORMATS, Spatializer, EQ_KEEP, WAVData, WAVError, WAVLoader, default_context, sample_format_bytes,
    MultiSpatializer, device_count, device_info,
)

from .rateconv import RateConverter, convert, rateconv_filter, rateconv_plan  # noqa: E402
from .batching import MixedRateBatch, RateBucket, bucket_by_rate, resample_tracks  # noqa: E402
from .graph import AudioEffectGraph, AudioEffectPreparationResult, AudioEffectWarning  # noqa: E402
from .eq import (  # noqa: E402
    BiquadCoefficientBuilder, BiquadCoefficientError, EqualizerAPOParser, EqualizerAudioEffectError, EqualizerDefinition,
    EqualizerFilter, EqualizerParseError, EqualizerRuntimeEffect, ParametricEqualizerPreparationError,
    ParametricEqualizerProcessor, ParametricEqualizerState, EqualizerNotFoldable, FoldedHRIR, fold_equalizer,
)

__all__ = [
    "AudioEffectGraph", "AudioEffectPreparationResult", "AudioEffectWarning",
    "MixedRateBatch", "RateBucket", "bucket_by_rate", "resample_tracks",
    "RateConverter", "convert", "rateconv_filter", "rateconv_plan",
    "BiquadCoefficientBuilder", "BiquadCoefficientError", "EqualizerAPOParser", "EqualizerAudioEffectError",
    "EqualizerDefinition", "EqualizerFilter", "EqualizerParseError", "EqualizerRuntimeEffect",
    "ParametricEqualizerPreparationError", "ParametricEqualizerProcessor", "ParametricEqualizerState", "EqualizerNotFoldable", "FoldedHRIR", "fold_equalizer",
    "AirwaveError", "Context", "ConvolutionEngine", "HRIR", "HRIRChannelMap", "HRIRError", "HRIRManager",
    "InputLayout", "RealtimeAudioProcessor", "Resampler", "Spatializer", "WAVData", "WAVError", "WAVLoader",
    "default_context", "SAMPLE_FORMATS", "sample_format_bytes", "DITHER_MODES", "GAIN_MODES", "LEVELS_DTYPE",
    "LOUDNESS_DTYPE", "loudness_gain", "TRUE_PEAK_DTYPE", "true_peak_filter", "LIMITER_DTYPE", "EQ_KEEP",
    "MultiSpatializer", "device_count", "device_info",
]
