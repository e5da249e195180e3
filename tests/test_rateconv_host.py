"""CPU-side checks of the batch sample-rate converter (aw_rateconv_*; rules: airwave_amd/csrc/device/rateconv.hpp): the plan of nine rate
pairs and the refusals through the C ABI, the float32 table against the numpy formula (tests/rateconv_ref.py), the quality of the header's
sequential rule in float32 on sines in the passband and in the stopband, and the entries' declaration, export and types."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402
import rateconv_ref as ref  # noqa: E402
from airwave_amd import _capi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "airwave_hip.h")
AW_ERR_INVALID_ARGUMENT = 1
NAMES = ["aw_rateconv_plan", "aw_rateconv_filter", "aw_rateconv_create", "aw_rateconv_destroy", "aw_rateconv_info", "aw_rateconv_output_frames",
         "aw_rateconv_process", "aw_rateconv_flush", "aw_rateconv_reset"]

# in, out -> L, M, T, D
PLANS = {
    (44100, 48000): (160, 147, 96, 48),
    (48000, 44100): (147, 160, 106, 53),
    (48000, 96000): (2, 1, 96, 48),
    (96000, 48000): (1, 2, 192, 96),
    (96000, 44100): (147, 320, 210, 105),
    (44100, 96000): (320, 147, 96, 48),
    (192000, 44100): (147, 640, 418, 209),
    (44100, 192000): (640, 147, 96, 48),
    (88200, 48000): (80, 147, 178, 89),
}
DOWNWARD = [p for p in PLANS if p[0] > p[1]]


def c_plan(in_rate, out_rate):
    v = [ctypes.c_int32() for _ in range(4)]
    st = _capi.load().aw_rateconv_plan(in_rate, out_rate, *[ctypes.byref(x) for x in v])
    return st, tuple(x.value for x in v)


def c_filter(in_rate, out_rate):
    L, _, T, _ = PLANS[(in_rate, out_rate)]
    c = np.zeros((L, T), np.float32)
    assert _capi.load().aw_rateconv_filter(in_rate, out_rate, c.ctypes.data_as(_capi.c_float_p), c.size) == 0
    return c


@pytest.mark.parametrize("pair", sorted(PLANS))
def test_plan_of_the_nine_pairs(pair):
    st, got = c_plan(*pair)
    assert st == 0 and got == PLANS[pair]
    assert ref.plan(*pair) == PLANS[pair] == emu.plan(*pair)


@pytest.mark.parametrize("pair", [(48000, 48000), (44100.5, 48000), (48000, 44100.5), (0, 48000), (48000, 0), (-44100, 48000), (48000, -1),
                                  (48000, 44101), (float("nan"), 48000), (float("inf"), 48000)])
def test_refusals(pair):
    lib = _capi.load()
    st, _ = c_plan(*pair)
    assert st == AW_ERR_INVALID_ARGUMENT and lib.aw_last_error_message()
    c = np.zeros(8, np.float32)
    assert lib.aw_rateconv_filter(pair[0], pair[1], c.ctypes.data_as(_capi.c_float_p), c.size) == AW_ERR_INVALID_ARGUMENT
    assert not c.any()
    assert emu.plan(*pair) is None


def test_filter_capacity_and_null_are_refused():
    lib = _capi.load()
    c = np.zeros(2 * 96, np.float32)
    assert lib.aw_rateconv_filter(48000, 96000, c.ctypes.data_as(_capi.c_float_p), c.size - 1) == AW_ERR_INVALID_ARGUMENT and not c.any()
    assert lib.aw_rateconv_filter(48000, 96000, None, c.size) == AW_ERR_INVALID_ARGUMENT
    assert lib.aw_rateconv_filter(48000, 96000, c.ctypes.data_as(_capi.c_float_p), c.size) == 0 and c.any()


@pytest.mark.parametrize("pair", sorted(PLANS))
def test_filter_equals_the_numpy_formula(pair):
    L, M, T, D = PLANS[pair]
    c = c_filter(*pair)
    want = ref.coefficients(L, M)
    assert want.shape == (L, T)
    err = np.abs(c.astype(np.float64) - want).max()
    print(f"{pair}: largest coefficient {np.abs(want).max():.6f}, largest difference {err:.3e}")
    assert err <= 2.0 ** -23 * np.abs(want).max()
    assert np.array_equal(c, emu.filter_table(*pair))               # the library's table is the header's
    # unity gain at DC, phase by phase, and a symmetric prototype
    assert np.abs(want.sum(axis=1) - 1.0).max() < 1e-4
    assert np.allclose(want[0, 1:], want[0, 1:][::-1], atol=1e-15)


def sequential32(x, pair):
    """One mono stream through the header's sequential rule in float32: process, no flush."""
    rc = emu.Converter(pair[0], pair[1], 1, 1, kernel=False)
    return rc.process(np.asarray(x, np.float32).reshape(1, -1, 1))[0, :, 0]


def residue_db(pair, freq, passband):
    """RMS of (output - ideal sine at the output rate) for a passband tone, of the output itself for a stopband tone, over the output
    without 2 T L / M + 8 frames at each end, relative to the tone's RMS."""
    L, M, T, D = PLANS[pair]
    N, amp = 16384, 0.5
    x = (amp * np.sin(2.0 * np.pi * freq / pair[0] * np.arange(N))).astype(np.float32)
    y = sequential32(x, pair).astype(np.float64)
    assert y.size == ref.output_count(N, L, M, D)
    skip = 2 * T * L // M + 8
    n = np.arange(y.size)[skip:y.size - skip]
    assert n.size > 1000
    ideal = amp * np.sin(2.0 * np.pi * freq / pair[0] * (n * M / L)) if passband else 0.0          # output n sits at input time n M / L
    err = y[n] - ideal
    return 20.0 * np.log10(np.sqrt(np.mean(err * err)) / (amp / np.sqrt(2.0)))


@pytest.mark.parametrize("pair", sorted(PLANS))
def test_passband_error_of_the_sequential_rule(pair):
    low_nyquist = min(pair) / 2.0
    for freq in (997.0, 0.85 * low_nyquist):
        db = residue_db(pair, freq, passband=True)
        print(f"{pair} {freq:.1f} Hz: {db:.1f} dB")
        assert db <= -104.0, (pair, freq, db)


@pytest.mark.parametrize("pair", sorted(DOWNWARD))
def test_stopband_residue_of_the_sequential_rule(pair):
    assert len(DOWNWARD) == 5
    low_nyquist = pair[1] / 2.0
    for freq in (low_nyquist + 1.0, min(1.2 * low_nyquist, 0.98 * pair[0] / 2.0)):
        db = residue_db(pair, freq, passband=False)
        print(f"{pair} {freq:.1f} Hz: {db:.1f} dB")
        assert db <= -95.0, (pair, freq, db)


def test_the_float32_rule_stays_within_its_bound_of_the_float64_evaluation():
    rng = np.random.default_rng(11)
    for pair in [(44100, 48000), (192000, 44100)]:
        L, M, T, D = PLANS[pair]
        x = rng.standard_normal((3000, 1)).astype(np.float32)
        y = sequential32(x[:, 0], pair)
        y64, bound = ref.convert64(x, L, M, D, c_filter(*pair), with_bound=True)
        assert y.shape == y64[:, 0].shape and np.all(np.abs(y - y64[:, 0]) <= bound[:, 0])


def test_the_refusal_boundary_of_the_tile():
    """Every accepted plan (coprime L, M <= 640, T = 2 ceil(48 max(1, M / L))) at 1 .. 16 channels: where the header's rc_tile is 0
    (aw_rateconv_create refuses), 1 .. 11 (created, aw_tp_rateconv_set refuses) or 12 (the smallest with a measuring tile), and the three
    handles tests/rateconv_cases.py pins there by name.  The header's tile is asked wherever a tile of 13 outputs does not fit by a margin
    of one segment (no smaller tile can come from anywhere else), and must equal the formula restated in Python on all of those."""
    from math import gcd
    import emu_rateconv_tp as tp
    import rateconv_cases as geo
    by_tile = {}
    for L in range(1, 641):
        for M in range(1, 641):
            if L == M or gcd(L, M) != 1:
                continue
            D = -(-ref.Z * M // L) if M > L else ref.Z
            T = 2 * D
            for C in range(1, 17):
                span = -(-13 * M // L) + T
                if ((span - 1) // 32 + 2) * 35 * C + 3 * C + 3 + 13 * C <= 12288:          # 13 outputs fit with a segment to spare
                    continue
                tile, tp_tile = tp.tiles(L, M, T, C)
                assert tile == geo.tile_by_the_formula(L, M, T, C) and tp_tile == tile - 11, (L, M, T, C)
                by_tile.setdefault(tile, []).append((L, M, T, C))
    assert set(range(0, 13)) <= set(by_tile)                                         # every tile length from 0 to 12 exists
    # L = 1, M = 640 has no tile at any channel count: 61 440 taps alone are five times the LDS
    assert all((1, 640, 61440, C) in by_tile[0] for C in range(1, 17))
    n_refused_by_set = sum(len(by_tile[t]) for t in range(1, 12))
    print(f"no tile: {len(by_tile[0])} handles; a tile of 1 .. 11: {n_refused_by_set}; a tile of 12: {len(by_tile[12])}")
    assert (len(by_tile[0]), n_refused_by_set) == (150012, 18718)                    # (DESIGN.md §4.7 quotes them) of 3 985 184
    assert all(M > 6 * L for t in range(12) for L, M, T, C in by_tile[t])             # all of them lower the rate more than sixfold
    for handle, want in geo.BOUNDARY_TILES.items():
        (in_rate, out_rate), C = handle
        L, M, T, D = emu.plan(in_rate, out_rate)
        assert (L, M, T, C) in by_tile[want] and emu.tile(in_rate, out_rate, C) == want, handle
    assert geo.BOUNDARY_TILES == {geo.NO_TILE: 0, geo.TINY_TILE: 7, geo.SMALLEST_MEASURING: 12}
    L, M, T, _ = emu.plan(*geo.SMALLEST_MEASURING[0])
    assert tp.tiles(L, M, T, geo.SMALLEST_MEASURING[1]) == (12, 1) and tp.tiles(L, M, T, geo.TINY_TILE[1]) == (7, -4)


def test_the_entries_are_declared_exported_and_typed():
    text = open(HEADER).read()
    declared = set(re.findall(r"AW_API\s+[\w\s\*]+?\b(aw_\w+)\s*\(", text))
    lib = _capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in NAMES:
        assert name in declared and name in _capi.SIGNATURES and name in exported, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert [n for n in sorted(declared) if n.startswith("aw_rateconv_")] == sorted(NAMES)
    # no handle: every info index says so, and so do the calls
    assert all(lib.aw_rateconv_info(None, w) == -1 for w in range(8)) and lib.aw_rateconv_output_frames(None, 5) == -1
    n = ctypes.c_int64(-7)
    assert lib.aw_rateconv_process(None, None, 0, None, 0, ctypes.byref(n)) == AW_ERR_INVALID_ARGUMENT and n.value == -7
    assert lib.aw_rateconv_flush(None, None, 0, None) == AW_ERR_INVALID_ARGUMENT and lib.aw_rateconv_reset(None) == AW_ERR_INVALID_ARGUMENT
    lib.aw_rateconv_destroy(None)
    h = ctypes.c_void_p()
    assert lib.aw_rateconv_create(None, 44100.0, 48000.0, 1, 2, ctypes.byref(h)) == 4 and not h.value          # AW_ERR_NO_DEVICE: no CPU fallback
    # the header cites what the reference resamples and says why audio does not take that path
    section = text[text.index("batch sample-rate converter"):text.index("typedef struct aw_rateconv")]
    assert "Resampler.swift:31-68" in section and "-30 dB" in section


def test_the_package_exports_the_converter():
    import airwave_amd as aw
    assert aw.rateconv_plan(44100, 48000) == {"L": 160, "M": 147, "taps": 96, "latency": 48}
    assert np.array_equal(aw.rateconv_filter(48000, 96000), c_filter(48000, 96000))
    with pytest.raises(aw.AirwaveError) as e:
        aw.rateconv_plan(48000, 48000)
    assert e.value.name == "INVALID_ARGUMENT"
    assert callable(aw.convert) and isinstance(aw.RateConverter, type)
