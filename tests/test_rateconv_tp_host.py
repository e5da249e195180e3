"""CPU-side checks of the converter's true-peak entries (aw_tp_rateconv_*, include/airwave_hip.h): declaration, export and types of the
five names beside the unchanged lists of the two older families, the refusals that need no handle, the record's layout from a C99 program,
the measuring tile length over the standard pairs, and the rule itself (airwave_amd/csrc/device/rateconv.hpp, "true peak of the converted
output", through tests/emu/emu_rateconv_tp.cpp) on known sines: first the float64 references alone, then the sequential rule, inside
EBU Tech 3341's +0.2 / -0.4 dB."""
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
import emu_rateconv_tp as tp  # noqa: E402
import rateconv_ref  # noqa: E402
import true_peak_ref as ref  # noqa: E402
from airwave_amd import _capi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "airwave_hip.h")
AW_ERR_INVALID_ARGUMENT = 1
NAMES = ["aw_tp_rateconv_set", "aw_tp_rateconv_get", "aw_tp_rateconv_reset_records", "aw_tp_rateconv_measure", "aw_tp_rateconv_measure_flush"]
RATECONV = ["aw_rateconv_create", "aw_rateconv_destroy", "aw_rateconv_filter", "aw_rateconv_flush", "aw_rateconv_info", "aw_rateconv_output_frames",
            "aw_rateconv_plan", "aw_rateconv_process", "aw_rateconv_reset"]
PCM_RATECONV = ["aw_pcm_rateconv_flush", "aw_pcm_rateconv_get_levels", "aw_pcm_rateconv_process", "aw_pcm_rateconv_reset_levels", "aw_pcm_rateconv_set_dither",
                "aw_pcm_rateconv_set_gain", "aw_pcm_rateconv_set_metering"]
RATES = (44100, 48000, 88200, 96000, 176400, 192000)
PAIRS = [(a, b) for a in RATES for b in RATES if a != b]


def test_the_five_names_are_declared_exported_and_typed():
    text = open(HEADER).read()
    declared = set(re.findall(r"AW_API\s+[\w\s\*]+?\b(aw_\w+)\s*\(", text))
    lib = _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in NAMES:
        assert name in declared and name in _capi.SIGNATURES and name in exported, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert [n for n in sorted(declared) if n.startswith("aw_tp_rateconv_")] == sorted(NAMES)
    # the two older families are what they were
    assert [n for n in sorted(declared) if n.startswith("aw_rateconv_")] == RATECONV
    assert [n for n in sorted(declared) if n.startswith("aw_pcm_rateconv_")] == PCM_RATECONV
    assert [n for n in sorted(exported) if n.startswith("aw_rateconv_")] == RATECONV
    assert [n for n in sorted(exported) if n.startswith("aw_pcm_rateconv_")] == PCM_RATECONV


def test_null_handle_refusals_write_nothing():
    lib = _capi.load()
    n = ctypes.c_int64(-7)
    buf = np.zeros(64, np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert lib.aw_tp_rateconv_set(None, 1) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_last_error_message()
    assert lib.aw_tp_rateconv_get(None, 0, 1, p) == AW_ERR_INVALID_ARGUMENT and not buf.any()
    assert lib.aw_tp_rateconv_reset_records(None) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_tp_rateconv_measure(None, p, 1, 4, ctypes.byref(n)) == AW_ERR_INVALID_ARGUMENT and n.value == -7
    assert lib.aw_tp_rateconv_measure_flush(None, ctypes.byref(n)) == AW_ERR_INVALID_ARGUMENT and n.value == -7
    assert lib.aw_rateconv_info(None, 10) == -1 and lib.aw_rateconv_info(None, 11) == -1


def test_the_record_is_16_bytes(tmp_path):
    src = tmp_path / "tp.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "airwave_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d\\n", (int)sizeof(aw_rateconv_true_peak), (int)offsetof(aw_rateconv_true_peak, true_peak),\n'
                   '    (int)offsetof(aw_rateconv_true_peak, sample_peak), (int)offsetof(aw_rateconv_true_peak, frames)); return 0; }\n')
    exe = tmp_path / "tp"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got] == [16, 0, 4, 8]
    assert tp.TRUE_PEAK.itemsize == 16 and [tp.TRUE_PEAK.fields[n][1] for n in ("true_peak", "sample_peak", "frames")] == [0, 4, 8]
    from airwave_amd.rateconv import RATECONV_TRUE_PEAK_DTYPE
    assert RATECONV_TRUE_PEAK_DTYPE == tp.TRUE_PEAK


def test_the_measuring_tile_of_the_standard_pairs():
    assert len(PAIRS) == 30
    worst = {}
    for pair in PAIRS:
        L, M, T, D = emu.plan(*pair)
        for C in range(1, 17):
            tile, tp_tile = tp.tiles(L, M, T, C)
            assert tile == emu.tile(pair[0], pair[1], C)
            assert 1 <= tp_tile <= tile, (pair, C, tile, tp_tile)
            worst.setdefault(pair, []).append(tp_tile)
    assert all(v[15] == min(v) for v in worst.values())              # 16 channels are the worst of every pair
    assert [tp.tp_tile(44100, 48000, 2), tp.tp_tile(96000, 44100, 2), tp.tp_tile(192000, 44100, 16)] == [2984, 1730, 39]
    assert [emu.tile(44100, 48000, 2), emu.tile(96000, 44100, 2), emu.tile(192000, 44100, 16)] == [2995, 1741, 50]


def test_the_measuring_tile_is_a_function_of_l_m_t_and_channels_only():
    # pairs of rates that reduce to the same (L, M) have the same tile; so has a handle of any stream count (the function does not see it)
    for a, b in (((44100, 48000), (88200, 96000)), ((96000, 44100), (192000, 88200)), ((48000, 96000), (44100, 88200))):
        assert emu.plan(*a) == emu.plan(*b)
        assert all(tp.tp_tile(a[0], a[1], C) == tp.tp_tile(b[0], b[1], C) for C in (1, 2, 3, 8, 16))
    # over every accepted reduced ratio at 1 and 16 channels: never above rc_tile, and the handles that lose their tile are few
    lost = total = 0
    from math import gcd
    for L in range(1, 641):
        for M in range(1, 641):
            if L == M or gcd(L, M) != 1:
                continue
            D = -(-48 * M // L) if M > L else 48
            for C in (1, 16):
                tile, tp_tile = tp.tiles(L, M, 2 * D, C)
                assert tp_tile <= tile
                if tile >= 1:
                    total += 1
                    lost += tp_tile < 1
    print(f"handles with a tile: {total}; of them without a measuring tile: {lost} ({100.0 * lost / total:.2f} %)")
    assert 0 < lost < 0.02 * total


SINES = [(pair, freq, phase) for pair in ((44100, 48000), (48000, 44100), (96000, 44100)) for freq, phase in (("out/4", 0.0), ("out/4", 45.0), (997.0, 0.0))]


@pytest.mark.parametrize("pair,freq,phase", SINES, ids=lambda v: str(v).replace(" ", ""))
def test_known_sines_read_their_amplitude_behind_the_converter(pair, freq, phase):
    """A 0.5-amplitude sine generated at the input rate, so the time-aligned output has the stated phase at the output rate.  First the
    references alone (rateconv_ref.convert64, then true_peak_ref.measure, both float64), then the sequential rule over the composition's
    float32 outputs: both inside EBU Tech 3341's +0.2 / -0.4 dB of the amplitude; at 45 degrees the sample peak under-reads by 3 dB."""
    amp = 0.5
    f = pair[1] / 4.0 if freq == "out/4" else freq
    x = ref.faded_sine(pair[0], f, phase, amp)                       # [frames][2] float32
    L, M, T, D = rateconv_ref.plan(*pair)
    y64 = rateconv_ref.convert64(x, L, M, D, rateconv_ref.coefficients(L, M), flushed=True)
    want = ref.measure(y64.astype(np.float32), ref.coefficients())
    d = ref.db(want["peak"][0]) - ref.db(amp)
    print(f"{pair} {f} Hz at {phase} deg: the references read {ref.db(want['peak'][0]):.3f} dBTP ({d:+.3f})")
    assert -0.4 <= d <= 0.2
    # the rule: decode -> awrc::sequential -> awrc::true_peak_sequential
    q = tp.Composition(pair[0], pair[1], 1, 2)
    q.process(pcm.to_bytes(x[None], pcm.F32), pcm.F32, pcm.F32)
    q.flush(pcm.F32)
    got, sample = float(q.records["true_peak"][0]), float(q.records["sample_peak"][0])
    d = ref.db(got) - ref.db(amp)
    print(f"    the rule reads {ref.db(got):.3f} dBTP ({d:+.3f}), sample peak {ref.db(sample):.3f} dBFS, {int(q.records['frames'][0])} frames")
    assert -0.4 <= d <= 0.2
    assert int(q.records["frames"][0]) == y64.shape[0] == -(-x.shape[0] * L // M)
    assert got >= sample
    if freq == "out/4" and phase == 45.0:
        assert -3.1 <= ref.db(sample) - ref.db(amp) <= -2.9


def test_the_ceiling_gain_formula():
    c = np.float32(0.891)
    for t in (0.0, 0.5, 0.891, 0.8910001, 1.0, 1.7, 3.0e-3):
        t = np.float32(t)
        want = np.float32(c / t) if t > c else np.float32(1.0)
        assert tp.ceiling_gain(t, c) == want
    assert np.abs(tp.filter36().astype(np.float64).reshape(3, 12)).sum(axis=1).max() < 4.0
    assert np.array_equal(tp.filter36(), ref.coefficients().astype(np.float32).reshape(-1))


def test_the_header_states_the_rule_and_points_to_it():
    text = open(HEADER).read()
    old = text[text.index("Integer PCM in and out of the converter"):text.index("AW_API aw_status aw_pcm_rateconv_reset_levels")]
    assert "true-peak meter or limiter after the converter is not provided" in old and "True peak of the converted output" in old
    new = text[text.index("/* True peak of the converted output"):text.index("AW_API aw_status aw_tp_rateconv_measure_flush")]
    for needle in ("BEFORE gain, dither and encode", "v[n] = 0 for n < 0", "v[n-11]", "aw_true_peak_filter", "NOT seen by the meter", "c / true_peak_s",
                   "AW_GAIN_FIXED", "stay refused", "16 bytes", "not flushed", "one device allocation"):
        assert needle in new, needle
    assert "10 true-peak measuring on" in text and "11 output" in text
