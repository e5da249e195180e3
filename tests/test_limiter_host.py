"""The limiter's rule (airwave_amd/csrc/device/limiter.hpp), compiled by plain g++: sequential() against an independent numpy
restatement, the bound g[n] <= r[k], the sample-peak bound, transparency below the ceiling, the true peak of a limited fs/4 burst, and
cutting the input into calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emu_limiter as emu  # noqa: E402
import limiter_ref as ref  # noqa: E402

C = 0.891
CONFIGS = [(16, 0), (64, 128), (512, 1024)]
N = 3001


def loud(seed, n=N, streams=1):
    return np.random.default_rng(seed).uniform(-2.5, 2.5, (streams, n, 2)).astype(np.float32)


def run_whole(y, L, H, gains=None):
    lim = emu.Limiter(y.shape[0], L, H, C, gains)
    z = lim.process(y)
    return lim, z


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("L,H", CONFIGS)
def test_sequential_equals_the_numpy_restatement_bit_for_bit(L, H):
    y = loud(L + H)
    gains = np.array([0.75], np.float32)
    lim, z = run_whole(y, L, H, gains)
    g, zr = ref.limiter(y[0], gains[0], L, H, C, lim.p[0])
    assert np.array_equal(bits(lim.g[0]), bits(g))
    assert np.array_equal(bits(z[0]), bits(zr))
    assert lim.min_gain[0] == bits(g).min() and lim.limited[0] == np.count_nonzero(g < 1.0) and lim.nonfinite[0] == 0
    assert g.min() < 0.6 and lim.limited[0] > N // 2


@pytest.mark.parametrize("L,H", CONFIGS)
def test_the_gain_is_at_most_what_every_window_near_the_delayed_frame_asks_for(L, H):
    y = loud(100 + L)
    lim, _ = run_whole(y, L, H)
    g, r = lim.g[0], ref.required_gain(lim.p[0], C)
    D = emu.delay(L)
    n = np.arange(N)
    for o in range(-D - H, -D + 12):
        k = n + o
        ok = (k >= 0) & (k < N)
        assert np.all(g[ok] <= r[k[ok]]), o


@pytest.mark.parametrize("L,H", CONFIGS)
def test_no_sample_exceeds_the_ceiling_by_more_than_two_roundings(L, H):
    """z = fl(u * g) with g <= r = fl(c / p) and |u| <= p: |z| <= c (1 + 2^-24)^2 < c (1 + 2^-23) in float64."""
    y = loud(200 + L)
    _, z = run_whole(y, L, H)
    assert np.abs(z.astype(np.float64)).max() <= float(np.float32(C)) * (1.0 + 2.0 ** -23)


@pytest.mark.parametrize("L,H", CONFIGS)
def test_below_the_ceiling_the_limiter_is_a_delay(L, H):
    rng = np.random.default_rng(300 + L)
    y = rng.uniform(-0.4, 0.4, (1, N, 2)).astype(np.float32)           # true peak of u <= 0.42 * sum |c| < 0.86 < c
    gains = np.array([1.05], np.float32)
    lim, z = run_whole(y, L, H, gains)
    D = emu.delay(L)
    u = (y[0] * gains[0]).astype(np.float32)
    assert np.array_equal(bits(z[0, D:]), bits(u[:N - D])) and not z[0, :D].any()
    assert lim.min_gain[0] == emu.ONE_BITS and lim.limited[0] == 0


def fs4_burst(n=800, start=200, length=400, amp=1.2):
    """A sine at a quarter of the sample rate sampled at 45 degrees (its samples under-read its peak by 3 dB), under a Hann envelope."""
    y = np.zeros((1, n, 2), np.float64)
    i = np.arange(length)
    y[0, start:start + length, :] = (amp * (0.5 - 0.5 * np.cos(2 * np.pi * i / length)) * np.sin(np.pi / 2 * i + np.pi / 4))[:, None]
    return y.astype(np.float32)


@pytest.mark.parametrize("L,H", CONFIGS)
def test_an_isolated_burst_comes_out_at_the_ceiling(L, H):
    """With eps = 2^-24: across the twelve frames of the peak's window the gain is flat, g <= r = fl(c / p) <= (c / p)(1 + eps), and each
    z_k = u_k g (1 + d_k), |d_k| <= eps.  The interpolated output is a chain of one product and eleven fmaf (twelve roundings) over
    sum c_k z_k = g sum c_k u_k + sum c_k u_k g d_k, and the input's own chain gave p with the same twelve roundings.  With
    A = sum |c_k| of the phase and |u_k| <= p, to first order
        |t_z| <= g p + g (12 eps A p) + eps A g p + 12 eps A g p <= c (1 + eps (1 + 25 A)).
    A is at most 2.04 for these coefficients, so the allowance is 52 eps; the issue's 64 eps covers it."""
    y = fs4_burst()
    D = emu.delay(L)
    y = np.concatenate([y, np.zeros((1, D, 2), np.float32)], axis=1)                # flush the delay
    lim, z = run_whole(y, L, H)
    coef = np.zeros(36, np.float32)
    emu.lib().emu_limiter_filter(coef.ctypes.data)
    A = np.abs(coef.astype(np.float64)).reshape(3, 12).sum(axis=1).max()
    allowance = (1.0 + 25.0 * A) * 2.0 ** -24
    assert allowance <= 64 * 2.0 ** -24
    tp_in, tp_out = float(emu.true_peak(y[0])), float(emu.true_peak(z[0]))
    print(f"L={L} H={H}: input true peak {tp_in:.6f}, output true peak / c = {tp_out / float(np.float32(C)):.9f}, allowance {1 + allowance:.9f}")
    assert tp_in > 1.15 and lim.limited[0] > 0
    assert tp_out <= float(np.float32(C)) * (1.0 + allowance)
    assert tp_out >= float(np.float32(C)) * (1.0 - 1e-3)


@pytest.mark.parametrize("L,H", CONFIGS)
def test_cutting_the_input_into_calls_changes_no_bit(L, H):
    y = loud(400 + L, n=2 * emu.halo(L, H) + 301, streams=2)
    y[1, 37, 0] = np.nan
    n = y.shape[1]
    gains = np.array([1.0, 0.5], np.float32)
    whole, z = run_whole(y, L, H, gains)
    D = emu.delay(L)
    cut = emu.Limiter(2, L, H, C, gains)
    sizes, parts, at, i = [1, 7, D - 1, D, D + 1], [], 0, 0
    while at < n:
        k = min(sizes[i % len(sizes)], n - at)
        parts.append(cut.process(y[:, at:at + k]))
        at += k
        i += 1
    zc = np.concatenate(parts, axis=1)
    assert np.array_equal(bits(z), bits(zc))
    assert all(np.array_equal(a, b) for a, b in zip(whole.records(), cut.records()))
    assert np.array_equal(bits(whole.history()), bits(cut.history()))
    assert whole.nonfinite.tolist() == [0, 1]
