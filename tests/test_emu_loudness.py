"""CPU thread emulation of the loudness kernels (the code hipcc compiles, airwave_amd/csrc/device/loudness_scan.hpp) against the
sequential float64 recurrence of loudness_ref.py: calls shorter than a chunk, partial spans, tails, chunks that straddle a hop edge
(44.1 kHz), state and a hop carried over a call boundary, a NaN in the middle of a chunk."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_loudness  # noqa: E402
import loudness_ref as ref  # noqa: E402

# Hop energies differ from the sequential recurrence by Float64 reassociation only (the chunk scan, the table powers, the order of the
# hop sums).  Measured over every case below: 1.16e-13 relative (44.1 kHz, the one-frame hop that ends a 4411-frame call: a single
# sample, small against the filter state it rides on; every other case stays below 1e-14).  The bound allows 8 x that for the device's
# different FMA contraction.  An error above 1e-9 would mean that the table powers of the 38 Hz section are no longer formed in
# double-double: a bug, not something to widen this for.
MEASURED = 1.16e-13
BOUND = 8 * MEASURED

FRAMES = [5, 31, 32, 4409, 4410, 4411, 8192 + 3 * 32 + 7, 2 * 8192 + 32]
RATES = [44100, 48000, 96000]
SECOND = 333


def reference(calls, rate):
    """Hop energies (complete and partial hops alike) and non-finite count of the concatenated calls: [streams][frames][2] each."""
    y = np.concatenate(calls, axis=1)
    hop = rate // 10
    v, bad = ref.sanitize(y)
    k, _ = ref.k_weight_loop(np.moveaxis(v, 1, -1), rate)          # [streams][2][frames]
    sq = (k ** 2).sum(axis=1)
    n_hops = -(-y.shape[1] // hop)
    pad = np.zeros((y.shape[0], n_hops * hop))
    pad[:, : y.shape[1]] = sq
    return pad.reshape(y.shape[0], n_hops, hop).sum(axis=2), bad


def rel_error(got, want):
    assert np.all(want > 0)
    return float(np.max(np.abs(got - want) / want))


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("frames", FRAMES)
def test_hop_energies_match_sequential_recurrence(frames, rate):
    rng = np.random.default_rng(frames + rate)
    x = rng.uniform(-0.5, 0.5, (1, frames, 2)).astype(np.float32)
    x2 = rng.uniform(-0.5, 0.5, (1, SECOND, 2)).astype(np.float32)
    cap = 8
    m = emu_loudness.Meter(1, rate, cap)
    m.process(x)
    first = m.hops.copy()
    m.process(x2)                                                   # the stream continues: state, and a hop across the call boundary
    assert m.hop == rate // 10 and m.frames == frames + SECOND
    want1, _ = reference([x], rate)
    want, bad = reference([x, x2], rate)
    n1, n = want1.shape[1], want.shape[1]
    e1, e = rel_error(first[:, :n1], want1), rel_error(m.hops[:, :n], want)
    print(f"frames {frames} rate {rate}: relative error of the hop energies {e1:.3e} (first call) {e:.3e} (both)")
    assert e1 <= BOUND and e <= BOUND
    assert not first[:, n1:].any() and not m.hops[:, n:].any() and bad == 0 and not m.nonfinite.any()


@pytest.mark.parametrize("rate", RATES)
def test_a_nan_enters_as_zero_and_is_counted(rate):
    rng = np.random.default_rng(rate)
    frames = 8192 + 4411
    x = rng.uniform(-0.5, 0.5, (2, frames, 2)).astype(np.float32)
    x[0, 4410 + 17, 1] = np.nan                                     # the middle of a chunk, next to a 44.1 kHz hop edge
    x[1, 8192 + 4400, 0] = np.inf                                   # the sequential tail
    x[1, 100, :] = [-np.inf, np.nan]
    m = emu_loudness.Meter(2, rate, 4)
    m.process(x)
    want, _ = reference([x], rate)
    n = want.shape[1]
    e = rel_error(m.hops[:, :n], want)
    print(f"NaN case, rate {rate}: relative error of the hop energies {e:.3e}")
    assert e <= BOUND
    assert m.nonfinite.tolist() == [1, 3]


def test_capacity_drops_later_hops_only():
    rate, frames = 48000, 3 * 4800 + 100
    x = np.random.default_rng(9).uniform(-0.5, 0.5, (1, frames, 2)).astype(np.float32)
    full, short = emu_loudness.Meter(1, rate, 4), emu_loudness.Meter(1, rate, 2)
    full.process(x)
    short.process(x)
    assert np.array_equal(short.hops, full.hops[:, :2]) and full.hops[0, 3] > 0


def test_table_powers_of_both_sections_are_exact():
    """The 38 Hz high-pass has a double pole next to z = 1: its table powers up to M^2048 need double-double (tests/test_emu_eq.py)."""
    from fractions import Fraction
    for rate in RATES:
        coef, tab, plane = emu_loudness.tables(rate)
        assert np.array_equal(coef, ref.k_coefficients(rate)[:, [0, 1, 2, 4, 5]]) or np.max(np.abs(coef - ref.k_coefficients(rate)[:, [0, 1, 2, 4, 5]])) < 1e-13
        for k in range(2):
            a1, a2 = Fraction(float(tab[k, 3])), Fraction(float(tab[k, 4]))
            M = ((-a1, Fraction(1)), (-a2, Fraction(0)))

            def mul(a, b):
                return ((a[0][0] * b[0][0] + a[0][1] * b[1][0], a[0][0] * b[0][1] + a[0][1] * b[1][1]),
                        (a[1][0] * b[0][0] + a[1][1] * b[1][0], a[1][0] * b[0][1] + a[1][1] * b[1][1]))
            P = ((Fraction(1), Fraction(0)), (Fraction(0), Fraction(1)))
            for _ in range(32):
                P = mul(M, P)
            Pl = P
            for m_ in range(64):
                ex = np.array([[float(v) for v in row] for row in Pl]).reshape(-1)
                assert np.max(np.abs(plane[k, m_] - ex)) <= 4e-16 * np.max(np.abs(ex)), (rate, k, m_)
                Pl = mul(P, Pl)
