"""CPU-side checks of the converter's PCM entries (aw_pcm_rateconv_*, include/airwave_hip.h): declaration, export and types of the seven
names, the refusals that need no handle, the record's layout from a C99 program, and the dither's key rule — pair 0 of a converter is the
spatializer's key, so a stereo frame gets the spatializer's noise at the same position; pair j >= 1 gets K + j * 0xA0761D6478BD642F —
against the numpy restatement of the documented dither (tests/test_pcm_dither_host.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402
import emu_rateconv_pcm as pcm  # noqa: E402
from airwave_amd import _capi  # noqa: E402
from test_pcm_dither_host import np_dither, np_encode_dithered, np_key, np_splitmix64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "airwave_hip.h")
AW_ERR_INVALID_ARGUMENT = 1
U64 = np.uint64
NAMES = ["aw_pcm_rateconv_process", "aw_pcm_rateconv_flush", "aw_pcm_rateconv_set_dither", "aw_pcm_rateconv_set_gain", "aw_pcm_rateconv_set_metering",
         "aw_pcm_rateconv_get_levels", "aw_pcm_rateconv_reset_levels"]
SEED, FIRST = 0xC0FFEE1234, 5
pytestmark = pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning")          # (uint64 scalars wrap mod 2^64 on purpose)


def test_the_seven_names_are_declared_exported_and_typed():
    text = open(HEADER).read()
    declared = set(re.findall(r"AW_API\s+[\w\s\*]+?\b(aw_\w+)\s*\(", text))
    lib = _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in NAMES:
        assert name in declared and name in _capi.SIGNATURES and name in exported, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert [n for n in sorted(declared) if n.startswith("aw_pcm_rateconv_")] == sorted(NAMES)


def test_null_handle_refusals():
    lib = _capi.load()
    n = ctypes.c_int64(-7)
    buf = np.zeros(64, np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert lib.aw_pcm_rateconv_process(None, p, 1, 4, p, 1, 8, ctypes.byref(n), None) == AW_ERR_INVALID_ARGUMENT and n.value == -7
    assert lib.aw_last_error_message()
    assert lib.aw_pcm_rateconv_flush(None, p, 1, 8, ctypes.byref(n), None) == AW_ERR_INVALID_ARGUMENT and n.value == -7
    assert lib.aw_pcm_rateconv_set_dither(None, 1, 0, 0) == AW_ERR_INVALID_ARGUMENT
    g = np.ones(1, np.float32)
    assert lib.aw_pcm_rateconv_set_gain(None, 1, g.ctypes.data_as(_capi.c_float_p), 1) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_pcm_rateconv_set_metering(None, 1) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_pcm_rateconv_get_levels(None, 0, 1, p) == AW_ERR_INVALID_ARGUMENT and not buf.any()
    assert lib.aw_pcm_rateconv_reset_levels(None) == AW_ERR_INVALID_ARGUMENT
    assert all(lib.aw_rateconv_info(None, w) == -1 for w in range(11))


def test_the_record_is_32_bytes(tmp_path):
    src = tmp_path / "levels.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "airwave_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d\\n", (int)sizeof(aw_rateconv_levels), (int)offsetof(aw_rateconv_levels, peak),\n'
                   '    (int)offsetof(aw_rateconv_levels, reserved), (int)offsetof(aw_rateconv_levels, frames), (int)offsetof(aw_rateconv_levels, clipped),\n'
                   '    (int)offsetof(aw_rateconv_levels, nonfinite)); return 0; }\n')
    exe = tmp_path / "levels"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got] == [32, 0, 4, 8, 16, 24]
    assert pcm.LEVELS.itemsize == 32 and [pcm.LEVELS.fields[n][1] for n in ("peak", "reserved", "frames", "clipped", "nonfinite")] == [0, 4, 8, 16, 24]
    from airwave_amd.rateconv import RATECONV_LEVELS_DTYPE
    assert RATECONV_LEVELS_DTYPE == pcm.LEVELS


def test_the_key_of_pair_zero_is_the_spatializers_and_further_pairs_follow_the_formula():
    rng = np.random.default_rng(0)
    for seed, g in [(0, 0), (SEED, FIRST), (2 ** 64 - 1, 2 ** 40 + 3)] + [(int(a), int(b)) for a, b in rng.integers(0, 2 ** 63, (8, 2))]:
        k0 = int(np_key(seed, g))
        assert pcm.key(seed, g, 0) == pcm.key(seed, g, 1) == k0                        # both channels of pair 0: the spatializer's key
        for ch in range(2, 16):
            assert pcm.key(seed, g, ch) == (k0 + (ch >> 1) * 0xA0761D6478BD642F) % 2 ** 64, (seed, g, ch)
    assert pcm.PAIR_KEY == 0xA0761D6478BD642F


@pytest.mark.parametrize("mode", [pcm.TPDF, pcm.TPDF_HP], ids=["tpdf", "tpdf_hp"])
def test_a_stereo_frame_gets_the_spatializers_dither_and_pair_one_its_own(mode):
    """Through the composition AND the emulated kernel: the s16 code of output (stream s, frame n, channel ch) is the documented encode of
    the float32 output with the spatializer's dither of (seed, first_stream + s, n, ch & 1), the key moved by (ch >> 1) * 0xA076...."""
    pair, C, S = (48000, 96000), 4, 2
    L, M, T, D = emu.plan(*pair)
    n_in = emu.input_frames_for(emu.tile(pair[0], pair[1], C) + 5, L, M, D)
    x = pcm.random_input(np.random.default_rng(8), (S, n_in, C), pcm.F32)
    plain = pcm.Converter(pair[0], pair[1], S, C, False)
    y = pcm.from_bytes(plain.process(x, pcm.F32, pcm.F32), pcm.F32)                    # the float32 outputs, undithered
    n = np.arange(y.shape[1], dtype=U64)
    for kernel in (False, True):
        rc = pcm.Converter(pair[0], pair[1], S, C, kernel, mode, SEED, FIRST)
        got = pcm.from_bytes(rc.process(x, pcm.F32, pcm.S16), pcm.S16).astype(np.int64)
        for s in range(S):
            for ch in range(C):
                # np_dither takes (seed, global stream); a key moved by j * PAIR_KEY is restated here from its parts
                k = np_key(SEED, FIRST + s) + U64(ch >> 1) * U64(pcm.PAIR_KEY)
                if mode == pcm.TPDF:
                    h = np_splitmix64(k + U64(2) * n + U64(ch & 1))
                    d = ((h >> U64(40)).astype(np.int64) - ((h >> U64(16)) & U64(0xFFFFFF)).astype(np.int64)).astype(np.float32) * np.float32(2.0 ** -24)
                else:
                    sh = U64(16 if ch & 1 else 40)
                    r = lambda h: ((h >> sh) & U64(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)          # noqa: E731
                    d = r(np_splitmix64(k + n)) - r(np_splitmix64(k + n - U64(1)))
                if ch < 2:
                    assert np.array_equal(d, np_dither(mode, SEED, FIRST + s, n, ch & 1))          # pair 0: the spatializer's noise itself
                    assert np.array_equal(d, [np.float32(pcm.dither(mode, pcm.key(SEED, FIRST + s, ch), int(i), ch & 1)) for i in n[:64]] + list(d[64:]))
                else:
                    assert not np.array_equal(d, np_dither(mode, SEED, FIRST + s, n, ch & 1))      # pair 1: noise of its own
                want, _ = np_encode_dithered(pcm.S16, y[s, :, ch], d)
                assert np.array_equal(got[s, :, ch], want), (kernel, s, ch)


def test_the_header_states_the_rule():
    text = open(HEADER).read()
    section = text[text.index("Integer PCM in and out of the converter"):text.index("AW_API aw_status aw_pcm_rateconv_reset_levels")]
    for needle in ("0xA0761D6478BD642F", "0xD1B54A32D192ED03", "0x9E3779B97F4A7C15", "ch >> 1", "ch & 1", "first_stream + s", "BEFORE the gain",
                   "BEFORE conversion", "SAMPLE peak", "true-peak meter or limiter after the converter is not provided", "AW_GAIN_PEAK_CEILING",
                   "32 bytes", "clipped_device", "ANY byte alignment"):
        assert needle in section, needle
    assert "7 the aw_dither mode" in text and "9 metering on" in text
