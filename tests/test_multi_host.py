"""CPU-side checks of the multi-device handle (aw_multi_*, aw_device_*, include/airwave_hip.h "multi-device batch spatializer"): the names
are declared, exported and typed; the header's earlier sections are untouched; multi_runtime.cpp keeps the library's exception barrier;
the C++ mirror compiles; argument errors are answered before any device call and name the argument; without a device the enumeration
says 0 and creation says AW_ERR_NO_DEVICE; the example is strict C99 and fails loudly without a device."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import airwave_amd as aw
from airwave_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "airwave_hip.h")
AW_ERR_INVALID_ARGUMENT, AW_ERR_NO_DEVICE = 1, 4
NAMES = ["aw_device_count", "aw_device_info", "aw_multi_create", "aw_multi_destroy", "aw_multi_shard_count", "aw_multi_stream_count", "aw_multi_channel_count",
         "aw_multi_shard", "aw_multi_spatializer", "aw_multi_context", "aw_multi_reserve_pcm", "aw_multi_process_host_pcm", "aw_multi_reset",
         "aw_multi_alloc_pinned", "aw_multi_free_pinned", "aw_multi_set_dither", "aw_multi_set_metering", "aw_multi_reset_levels", "aw_multi_set_gain",
         "aw_multi_set_loudness", "aw_multi_set_true_peak", "aw_multi_set_limiter", "aw_multi_set_equalizer", "aw_multi_set_equalizer_target",
         "aw_multi_get_levels", "aw_multi_get_loudness", "aw_multi_get_loudness_hops", "aw_multi_get_true_peak", "aw_multi_get_limiter"]
# the last declaration of the section in front of the new one (the rate converter's), and the digest of the header up to and including it
LAST_EARLIER_ENTRY = "AW_API aw_status aw_tp_rateconv_measure_flush(aw_rateconv *rc, int64_t *out_frames);\n"
EARLIER_SECTIONS_SHA256 = "225341b82968fdace521b2050317ee2a9a3902a0ac763b6c3f294ad8919d01ff"
SRC = os.path.join(ROOT, "examples", "offline_batch_multi.c")
EXE = os.path.join(ROOT, "examples", "offline_batch_multi")


def test_names_are_declared_exported_and_typed_and_the_earlier_header_is_untouched():
    text = open(HEADER).read()
    declared = set(re.findall(r"AW_API[^;]*?\b(aw_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for n in NAMES:
        assert n in declared and hasattr(lib, n) and n in _capi.SIGNATURES, n
    assert sorted(n for n in declared if n.startswith(("aw_multi_", "aw_device_count", "aw_device_info"))) == sorted(NAMES)
    # the new section sits between the rate converter's last entry and aw_version
    at = [text.index(LAST_EARLIER_ENTRY)] + [text.index("AW_API " + d) for d in ("int32_t aw_device_count(void);", "aw_status aw_multi_get_limiter(")] + [text.index("AW_API const char *aw_version(void);")]
    assert at == sorted(at)
    assert ctypes.sizeof(_capi.DeviceInfo) == 344 and "/* 344 bytes */" in text
    for n in ("MultiSpatializer", "device_count", "device_info"):
        assert n in aw.__all__ and hasattr(aw, n), n
    for method in ("process", "process_host_into", "reserve_pcm", "set_dither", "set_metering", "levels", "reset_levels", "set_gain", "set_loudness", "loudness",
                   "loudness_hops", "set_true_peak", "true_peak", "set_limiter", "limiter", "set_equalizer", "set_equalizer_target", "reset", "shards", "pinned_empty"):
        assert callable(getattr(aw.MultiSpatializer, method)), method
    # ... and everything in front of the new section is byte for byte what it was: the digest of the header up to the rate converter's last
    # entry, and, where the tree is a checkout, the committed header's text up to that entry
    earlier = text[:text.index(LAST_EARLIER_ENTRY) + len(LAST_EARLIER_ENTRY)]
    assert text.count(LAST_EARLIER_ENTRY) == 1 and hashlib.sha256(earlier.encode()).hexdigest() == EARLIER_SECTIONS_SHA256
    r = subprocess.run(["git", "-C", ROOT, "show", "HEAD:include/airwave_hip.h"], capture_output=True, text=True)
    if r.returncode == 0 and LAST_EARLIER_ENTRY in r.stdout:
        assert r.stdout[:r.stdout.index(LAST_EARLIER_ENTRY) + len(LAST_EARLIER_ENTRY)] == earlier


def test_multi_runtime_keeps_the_exception_barrier():
    """tests/test_process_path_contract.py's rule and regular expressions, for the new unit."""
    src = open(os.path.join(ROOT, "airwave_amd", "csrc", "multi_runtime.cpp")).read()
    n = 0
    for m in re.finditer(r"^aw_status (aw_\w+)\(", src, re.M):
        head = src[m.start():src.index("{", m.end())]
        assert head.rstrip().endswith("try"), m.group(1)
        n += 1
    assert src.count("AW_NOEXCEPT_TAIL") == len(re.findall(r"^aw_status aw_\w+\(", src, re.M)) == n
    assert n == 22          # every name of NAMES that returns a status
    assert "getenv" not in src
    assert "multi_runtime.cpp" in open(os.path.join(ROOT, "airwave_amd", "build.py")).read()


def test_cpp_mirror_compiles(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", os.path.join(ROOT, "tests", "harness", "multi_mirror_check.cpp"),
                    "-o", str(tmp_path / "multi_mirror_check.o")], check=True)


def _create(lib, devices, n_devices, n_streams, out=True, tracks=True):
    h = ctypes.c_void_p()
    t = np.ones((2, 8), np.float32)
    lt, rt = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    dev = None if devices is None else np.ascontiguousarray(devices, np.int32)
    st = lib.aw_multi_create(None if dev is None else dev.ctypes.data_as(_capi.c_int32_p), n_devices, t.ctypes.data_as(_capi.c_float_p) if tracks else None, 2, 8,
                             48000.0, 2, lt.ctypes.data_as(_capi.c_int32_p), rt.ctypes.data_as(_capi.c_int32_p), n_streams, 0, ctypes.byref(h) if out else None)
    return st, h, (lib.aw_last_error_message() or b"").decode()


def test_argument_errors_come_before_any_device_call_and_name_the_argument():
    lib = _capi.load()
    for devices, n_devices, n_streams, out, word in (([0], 0, 5, True, "n_devices"), ([0] * 65, 65, 5, True, "n_devices"), (None, 2, 5, True, "device_ordinals"),
                                                     ([0, 0], 2, 0, True, "n_streams"), ([0, 0], 2, -3, True, "n_streams"), ([0, 0], 2, 5, False, "out")):
        st, h, msg = _create(lib, devices, n_devices, n_streams, out)
        assert st == AW_ERR_INVALID_ARGUMENT and not h.value and word in msg, (devices, n_devices, n_streams, out, st, msg)
    st, h, msg = _create(lib, [0], 1, 5, tracks=False)
    assert st == AW_ERR_INVALID_ARGUMENT and "tracks" in msg
    # the entries on a NULL handle
    assert lib.aw_multi_shard_count(None) == 0 and lib.aw_multi_spatializer(None, 0) is None and lib.aw_multi_context(None, 0) is None
    lib.aw_multi_destroy(None)
    for st in (lib.aw_multi_reset(None), lib.aw_multi_set_metering(None, 1), lib.aw_multi_reserve_pcm(None, 100, 0, 0),
               lib.aw_multi_process_host_pcm(None, None, 0, None, 0, 10, None), lib.aw_multi_get_levels(None, 0, 1, None),
               lib.aw_multi_set_gain(None, 1, None, 0, 0.0), lib.aw_multi_get_loudness_hops(None, 0, 0, 1, None), lib.aw_device_info(0, None)):
        assert st == AW_ERR_INVALID_ARGUMENT


def test_without_a_device_the_count_is_zero_and_creation_says_so():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present: the no-device answers are checked where there is none")
    lib = _capi.load()
    assert lib.aw_device_count() == 0 and aw.device_count() == 0
    d = _capi.DeviceInfo()
    assert lib.aw_device_info(0, ctypes.byref(d)) == AW_ERR_NO_DEVICE
    st, h, msg = _create(lib, [0, 0], 2, 5)
    assert st == AW_ERR_NO_DEVICE and not h.value and msg.startswith("shard 0 (device 0): "), (st, msg)
    try:
        aw.MultiSpatializer([0, 0], np.ones((2, 8), np.float32), 48000.0, [0, 1], [1, 0], 5)
        raise AssertionError("no error")
    except aw.AirwaveError as e:
        assert e.name == "NO_DEVICE"


def build_example():
    lib_dir = os.path.join(ROOT, "airwave_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib_dir,
                    "-lairwave_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", EXE], check=True)


def test_multi_example_is_strict_c99_without_pthreads_and_needs_a_device():
    import torch
    src = open(SRC).read()
    assert "pthread" not in src.replace("no pthreads", "")          # the threads live in the library
    build_example()
    r = subprocess.run([EXE, "x.wav", "0,a"], capture_output=True, text=True)
    assert r.returncode == 2 and "devices:" in r.stderr                # a malformed device list is said, not guessed at
    r = subprocess.run([EXE, "x.wav", ",".join(["0"] * 65)], capture_output=True, text=True)
    assert r.returncode == 2 and "1 to 64" in r.stderr
    if torch.cuda.is_available():
        return                                                      # (the no-device exit runs where there is none; the rest ran)
    r = subprocess.run([EXE, os.path.join(ROOT, "tests", "golden", "hrtf", "RoomSH1.0.wav"), "0,0", "5", "0.5"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
