"""ctypes binding of include/airwave_hip.h — the same symbols a Swift module map would import.

Fails loudly when the shared library is missing: there is no Python/CPU fallback path.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AIRWAVE_HIP_LIBRARY") or os.path.join(HERE, "libairwave_hip.so")

c_float_p = ctypes.POINTER(ctypes.c_float)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)

# every symbol include/airwave_hip.h declares: (restype, argtypes)
_V, _I32, _I64, _U64, _D, _SZ, _S = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double, ctypes.c_size_t, ctypes.c_char_p
SIGNATURES = {
    "aw_status_string": (_S, [_I32]),
    "aw_last_error_message": (_S, []),
    "aw_last_eq_filter_error": (_I32, [c_int32_p, c_int32_p, c_int32_p]),
    "aw_version": (_S, []),
    "aw_context_create": (_I32, [_I32, c_void_pp]),
    "aw_context_create_on_stream": (_I32, [_I32, _V, c_void_pp]),
    "aw_context_destroy": (None, [_V]),
    "aw_context_synchronize": (_I32, [_V]),
    "aw_context_stream": (_V, [_V]),
    "aw_context_timer_start": (_I32, [_V]),
    "aw_context_timer_stop": (_I32, [_V, c_float_p]),
    "aw_context_reserve_scratch": (_I32, [_V, _SZ]),
    "aw_context_scratch_bytes": (_SZ, [_V]),
    "aw_context_bandwidth_probe": (_I32, [_V, _SZ, _I32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "aw_context_pcie_probe": (_I32, [_V, _SZ, _I32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "aw_host_alloc_pinned": (_I32, [_V, _SZ, c_void_pp]),
    "aw_host_free_pinned": (_I32, [_V, _V]),
    "aw_device_alloc": (_I32, [_V, _SZ, c_void_pp]),
    "aw_device_free": (_I32, [_V, _V]),
    "aw_memcpy_h2d": (_I32, [_V, _V, _V, _SZ]),
    "aw_memcpy_d2h": (_I32, [_V, _V, _V, _SZ]),
    "aw_hrir_create": (_I32, [_V, c_float_p, _I32, _I32, _D, c_void_pp]),
    "aw_hrir_destroy": (None, [_V]),
    "aw_hrir_track_count": (_I32, [_V]),
    "aw_hrir_taps": (_I32, [_V]),
    "aw_hrir_sample_rate": (_D, [_V]),
    "aw_spatializer_create": (_I32, [_V, _V, _I32, c_int32_p, c_int32_p, _I32, _I32, c_void_pp]),
    "aw_spatializer_destroy": (None, [_V]),
    "aw_spatializer_process": (_I32, [_V, _V, _V, _I64]),
    "aw_spatializer_process_host": (_I32, [_V, c_float_p, c_float_p, _I64]),
    "aw_spatializer_process_planar": (_I32, [_V, c_float_p, c_float_p, c_float_p, c_float_p, _I32]),
    "aw_spatializer_reserve": (_I32, [_V, _I64]),
    "aw_spatializer_reserve_host": (_I32, [_V, _I64]),
    "aw_sample_format_bytes": (_I32, [_I32]),
    "aw_spatializer_process_pcm": (_I32, [_V, _V, _I32, _V, _I32, _I64, _V]),
    "aw_spatializer_process_host_pcm": (_I32, [_V, _V, _I32, _V, _I32, _I64, ctypes.POINTER(ctypes.c_uint64)]),
    "aw_spatializer_reserve_pcm": (_I32, [_V, _I64, _I32, _I32]),
    "aw_spatializer_set_dither": (_I32, [_V, _I32, _U64, _U64]),
    "aw_spatializer_set_metering": (_I32, [_V, _I32]),
    "aw_spatializer_get_levels": (_I32, [_V, _I32, _I32, _V]),
    "aw_spatializer_reset_levels": (_I32, [_V]),
    "aw_spatializer_set_gain": (_I32, [_V, _I32, c_float_p, _I32, ctypes.c_float]),
    "aw_spatializer_set_loudness": (_I32, [_V, _I32, _D]),
    "aw_spatializer_get_loudness": (_I32, [_V, _I32, _I32, _V]),
    "aw_spatializer_get_loudness_hops": (_I32, [_V, _I32, _I64, _I64, _V]),
    "aw_loudness_gain": (_I32, [_D, _D, c_float_p]),
    "aw_spatializer_set_true_peak": (_I32, [_V, _I32]),
    "aw_spatializer_get_true_peak": (_I32, [_V, _I32, _I32, _V]),
    "aw_true_peak_filter": (_I32, [c_float_p]),
    "aw_spatializer_set_limiter": (_I32, [_V, _I32, ctypes.c_float, _I32, _I32]),
    "aw_spatializer_get_limiter": (_I32, [_V, _I32, _I32, _V]),
    "aw_spatializer_set_equalizer": (_I32, [_V, c_void_pp, _I32, c_int32_p]),
    "aw_spatializer_set_equalizer_target": (_I32, [_V, c_void_pp, _I32, c_int32_p]),
    "aw_spatializer_reset": (_I32, [_V]),
    "aw_spatializer_stream_count": (_I32, [_V]),
    "aw_spatializer_channel_count": (_I32, [_V]),
    "aw_spatializer_info": (_I64, [_V, _I32]),
    "aw_spatializer_set_profiling": (_I32, [_V, _I32]),
    "aw_spatializer_kernel_time": (_I32, [_V, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_char_p)]),
    "aw_spatializer_stage_time": (_I32, [_V, _I32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]),
    "aw_spatializer_debug_stamps": (_I32, [_V, ctypes.POINTER(ctypes.c_uint64), _I64, ctypes.POINTER(ctypes.c_int64)]),
    "aw_engine_create": (_I32, [_V, c_float_p, _I32, _I32, c_void_pp]),
    "aw_engine_destroy": (None, [_V]),
    "aw_engine_process": (_I32, [_V, c_float_p, c_float_p]),
    "aw_engine_process_n": (_I32, [_V, c_float_p, c_float_p, _I32]),
    "aw_engine_process_accumulate": (_I32, [_V, c_float_p, c_float_p]),
    "aw_engine_reset": (_I32, [_V]),
    "aw_engine_block_size": (_I32, [_V]),
    "aw_realtime_create": (_I32, [_V, _V, _I32, c_int32_p, c_int32_p, _I32, _I32, c_void_pp]),
    "aw_realtime_destroy": (None, [_V]),
    "aw_realtime_process": (_I32, [_V, c_float_p, c_float_p, c_float_p, c_float_p, _I32]),
    "aw_realtime_reset": (_I32, [_V]),
    "aw_realtime_info": (_I64, [_V, _I32]),
    "aw_wav_load": (_I32, [_S, c_void_pp]),
    "aw_wav_destroy": (None, [_V]),
    "aw_wav_sample_rate": (_D, [_V]),
    "aw_wav_channel_count": (_I32, [_V]),
    "aw_wav_frame_count": (_I32, [_V]),
    "aw_wav_channel": (c_float_p, [_V, _I32]),
    "aw_wav_planar": (c_float_p, [_V]),
    "aw_layout_detect": (_I32, [_I32, c_void_pp]),
    "aw_layout_create": (_I32, [ctypes.POINTER(ctypes.c_char_p), _I32, _S, c_void_pp]),
    "aw_layout_destroy": (None, [_V]),
    "aw_layout_count": (_I32, [_V]),
    "aw_layout_speaker": (_S, [_V, _I32]),
    "aw_layout_name": (_S, [_V]),
    "aw_map_hesuvi14": (_I32, [_V, c_void_pp]),
    "aw_map_hesuvi7": (_I32, [_V, c_void_pp]),
    "aw_map_interleaved_pairs": (_I32, [_V, c_void_pp]),
    "aw_map_split_blocks": (_I32, [_V, c_void_pp]),
    "aw_map_parse_text": (_I32, [_S, c_void_pp]),
    "aw_map_destroy": (None, [_V]),
    "aw_map_count": (_I32, [_V]),
    "aw_map_get": (_I32, [_V, _S, c_int32_p, c_int32_p]),
    "aw_map_resolve": (_I32, [_V, _V, _I32, c_int32_p, c_int32_p]),
    "aw_resample_output_count": (_I32, [_I32, _D, _D]),
    "aw_resample": (_I32, [c_float_p, _I32, _D, _D, c_float_p, _I32, c_int32_p]),
    "aw_resample_vgenp": (_I32, [c_float_p, _I32, _D, _D, c_float_p, _I32, c_int32_p]),
    "aw_context_set_resampler": (_I32, [_V, _I32]),
    "aw_preset_activate": (_I32, [_V, _S, _D, _V, _V, _I32, c_void_pp, c_void_pp]),
    "aw_synth_fill": (_I32, [_V, _V, _I32, _I64, _I32, _U64, _U64]),
    # parametric EQ row
    "aw_biquad_make": (_I32, [_I32, _D, _D, _D, _D, ctypes.POINTER(ctypes.c_double), c_int32_p]),
    "aw_eq_definition_create": (_I32, [_D, c_void_pp]),
    "aw_eq_definition_add_filter": (_I32, [_V, _I32, _I32, _D, _D, _D]),
    "aw_eq_definition_set_source": (_I32, [_V, _I32, _I32, _I64]),
    "aw_eq_definition_destroy": (None, [_V]),
    "aw_eq_definition_preamp_db": (_D, [_V]),
    "aw_eq_definition_filter_count": (_I32, [_V]),
    "aw_eq_definition_filter": (_I32, [_V, _I32, c_int32_p, ctypes.POINTER(ctypes.c_int64), c_int32_p, c_int32_p,
                                       ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "aw_eq_parse": (_I32, [_V, _SZ, c_void_pp, ctypes.c_char_p, _SZ]),
    "aw_eq_state_create": (_I32, [_V, _V, _D, _I32, c_void_pp]),
    "aw_eq_state_destroy": (None, [_V]),
    "aw_eq_state_reset": (_I32, [_V]),
    "aw_eq_state_process": (_I32, [_V, _V, _V, _I64]),
    "aw_eq_state_filter_count": (_I32, [_V]),
    "aw_eq_state_preamp_linear": (_D, [_V]),
    "aw_eq_fold_hrir": (_I32, [_V, _D, c_float_p, _I32, _I32, _D, _I32, c_float_p, c_int32_p, c_int32_p, ctypes.POINTER(ctypes.c_double)]),
    "aw_eq_create": (_I32, [_V, _D, _I32, _I32, c_void_pp]),
    "aw_eq_destroy": (None, [_V]),
    "aw_eq_set_target": (_I32, [_V, _V]),
    "aw_eq_reset": (_I32, [_V]),
    "aw_eq_drain_retired": (_I32, [_V]),
    "aw_eq_process": (_I32, [_V, _V, _V, _I64]),
    "aw_eq_process_planar": (_I32, [_V, c_float_p, c_float_p, c_float_p, c_float_p, _I32]),
    "aw_eq_debug_hold_publication_lock": (_I32, [_V, _I32]),
    "aw_eq_transition_length": (_I32, [_V]),
    "aw_eq_is_transitioning": (_I32, [_V]),
    "aw_rateconv_plan": (_I32, [_D, _D, c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    "aw_rateconv_filter": (_I32, [_D, _D, c_float_p, _I64]),
    "aw_rateconv_create": (_I32, [_V, _D, _D, _I32, _I32, c_void_pp]),
    "aw_rateconv_destroy": (None, [_V]),
    "aw_rateconv_info": (_I64, [_V, _I32]),
    "aw_rateconv_output_frames": (_I64, [_V, _I64]),
    "aw_rateconv_process": (_I32, [_V, _V, _I64, _V, _I64, ctypes.POINTER(ctypes.c_int64)]),
    "aw_rateconv_flush": (_I32, [_V, _V, _I64, ctypes.POINTER(ctypes.c_int64)]),
    "aw_rateconv_reset": (_I32, [_V]),
    "aw_pcm_rateconv_process": (_I32, [_V, _V, _I32, _I64, _V, _I32, _I64, ctypes.POINTER(ctypes.c_int64), _V]),
    "aw_pcm_rateconv_flush": (_I32, [_V, _V, _I32, _I64, ctypes.POINTER(ctypes.c_int64), _V]),
    "aw_pcm_rateconv_set_dither": (_I32, [_V, _I32, _U64, _U64]),
    "aw_pcm_rateconv_set_gain": (_I32, [_V, _I32, c_float_p, _I32]),
    "aw_pcm_rateconv_set_metering": (_I32, [_V, _I32]),
    "aw_pcm_rateconv_get_levels": (_I32, [_V, _I32, _I32, _V]),
    "aw_pcm_rateconv_reset_levels": (_I32, [_V]),
    "aw_tp_rateconv_set": (_I32, [_V, _I32]),
    "aw_tp_rateconv_get": (_I32, [_V, _I32, _I32, _V]),
    "aw_tp_rateconv_reset_records": (_I32, [_V]),
    "aw_tp_rateconv_measure": (_I32, [_V, _V, _I32, _I64, ctypes.POINTER(ctypes.c_int64)]),
    "aw_tp_rateconv_measure_flush": (_I32, [_V, ctypes.POINTER(ctypes.c_int64)]),
    # device enumeration and the multi-device batch spatializer
    "aw_device_count": (_I32, []),
    "aw_device_info": (_I32, [_I32, _V]),
    "aw_multi_create": (_I32, [c_int32_p, _I32, c_float_p, _I32, _I32, _D, _I32, c_int32_p, c_int32_p, _I32, _I32, c_void_pp]),
    "aw_multi_destroy": (None, [_V]),
    "aw_multi_shard_count": (_I32, [_V]),
    "aw_multi_stream_count": (_I32, [_V]),
    "aw_multi_channel_count": (_I32, [_V]),
    "aw_multi_shard": (_I32, [_V, _I32, c_int32_p, c_int32_p, c_int32_p]),
    "aw_multi_spatializer": (_V, [_V, _I32]),
    "aw_multi_context": (_V, [_V, _I32]),
    "aw_multi_reserve_pcm": (_I32, [_V, _I64, _I32, _I32]),
    "aw_multi_process_host_pcm": (_I32, [_V, _V, _I32, _V, _I32, _I64, ctypes.POINTER(ctypes.c_uint64)]),
    "aw_multi_reset": (_I32, [_V]),
    "aw_multi_alloc_pinned": (_I32, [_V, _SZ, c_void_pp]),
    "aw_multi_free_pinned": (_I32, [_V, _V]),
    "aw_multi_set_dither": (_I32, [_V, _I32, _U64, _U64]),
    "aw_multi_set_metering": (_I32, [_V, _I32]),
    "aw_multi_reset_levels": (_I32, [_V]),
    "aw_multi_set_gain": (_I32, [_V, _I32, c_float_p, _I32, ctypes.c_float]),
    "aw_multi_set_loudness": (_I32, [_V, _I32, _D]),
    "aw_multi_set_true_peak": (_I32, [_V, _I32]),
    "aw_multi_set_limiter": (_I32, [_V, _I32, ctypes.c_float, _I32, _I32]),
    "aw_multi_set_equalizer": (_I32, [_V, c_void_pp, _I32, c_int32_p]),
    "aw_multi_set_equalizer_target": (_I32, [_V, c_void_pp, _I32, c_int32_p]),
    "aw_multi_get_levels": (_I32, [_V, _I32, _I32, _V]),
    "aw_multi_get_loudness": (_I32, [_V, _I32, _I32, _V]),
    "aw_multi_get_loudness_hops": (_I32, [_V, _I32, _I64, _I64, _V]),
    "aw_multi_get_true_peak": (_I32, [_V, _I32, _I32, _V]),
    "aw_multi_get_limiter": (_I32, [_V, _I32, _I32, _V]),
}


class DeviceInfo(ctypes.Structure):
    """struct aw_device_info (344 bytes)."""
    _fields_ = [("name", ctypes.c_char * 256), ("arch", ctypes.c_char * 64), ("compute_units", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("total_bytes", ctypes.c_uint64), ("free_bytes", ctypes.c_uint64)]



class StreamLevels(ctypes.Structure):
    """aw_stream_levels (56 bytes)."""
    _fields_ = [("peak", ctypes.c_float * 2), ("gain", ctypes.c_float), ("reserved", ctypes.c_uint32), ("energy", ctypes.c_double * 2),
                ("frames", ctypes.c_uint64), ("clipped", ctypes.c_uint64), ("nonfinite", ctypes.c_uint64)]


class StreamLoudness(ctypes.Structure):
    """aw_stream_loudness (56 bytes)."""
    _fields_ = [("integrated_lufs", ctypes.c_double), ("relative_threshold_lufs", ctypes.c_double), ("blocks", ctypes.c_uint32),
                ("blocks_above_absolute", ctypes.c_uint32), ("blocks_gated", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("frames", ctypes.c_uint64), ("frames_dropped", ctypes.c_uint64), ("nonfinite", ctypes.c_uint64)]


class StreamTruePeak(ctypes.Structure):
    """aw_stream_true_peak (32 bytes)."""
    _fields_ = [("true_peak", ctypes.c_float * 2), ("call_true_peak", ctypes.c_float), ("reserved", ctypes.c_uint32),
                ("frames", ctypes.c_uint64), ("nonfinite", ctypes.c_uint64)]


class StreamLimiter(ctypes.Structure):
    """aw_stream_limiter (32 bytes)."""
    _fields_ = [("min_gain", ctypes.c_float), ("reserved", ctypes.c_uint32), ("frames", ctypes.c_uint64),
                ("limited_frames", ctypes.c_uint64), ("nonfinite", ctypes.c_uint64)]


_lib = None


def load() -> ctypes.CDLL:
    """dlopen libairwave_hip.so and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python airwave_amd/build.py` (hipcc, gfx950). "
            "airwave_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)        # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
