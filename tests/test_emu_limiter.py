"""CPU thread emulation of the limiter kernel (the code hipcc compiles, airwave_amd/csrc/device/limiter_tile.hpp) against the sequential
rule of limiter.hpp, bit for bit — z, records and carried history: calls shorter than the delay, ragged and whole tiles, a tile that ends
inside the next one's halo, three streams (every other one 8 bytes off a 16-byte boundary when the frame count is odd), buffers that
start on any float, a second call of 7 frames, every extreme of (attack, hold), a NaN at a tile's first frame and an inf at a tile's last."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_limiter as emu  # noqa: E402

T = emu.tile()
C = 0.891
CONFIGS = [(16, 0), (64, 128), (512, 1024)]
STREAMS, SECOND = 3, 7
GAINS = np.array([1.0, 0.8, 1.25], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def both(y_calls, L, H, shift=0, gains=GAINS):
    k, s = emu.Limiter(STREAMS, L, H, C, gains, kernel=True), emu.Limiter(STREAMS, L, H, C, gains)
    for y in y_calls:
        zk, zs = k.process(y, shift), s.process(y)
        assert np.array_equal(bits(zk), bits(zs))
        assert np.array_equal(bits(k.history()), bits(s.history()))
        assert all(np.array_equal(a, b) for a, b in zip(k.records(), s.records()))
    return k, s


def test_tile_is_what_the_cases_assume():
    assert T == 1024 and emu.halo(512, 1024) == 2069 and emu.delay(16) == 27


def frame_counts(L, H):
    D = emu.delay(L)
    return [1, 5, D - 1, D, D + 1, T - 1, T, T + 1, T + emu.halo(L, H), 2 * T + 3]


@pytest.mark.parametrize("L,H", CONFIGS)
@pytest.mark.parametrize("case", range(10))
def test_kernel_equals_the_sequential_rule_bit_for_bit(L, H, case):
    frames = frame_counts(L, H)[case]
    rng = np.random.default_rng(1000 * L + frames)
    y = rng.uniform(-2.0, 2.0, (STREAMS, frames, 2)).astype(np.float32)
    y2 = rng.uniform(-2.0, 2.0, (STREAMS, SECOND, 2)).astype(np.float32)
    k, _ = both([y, y2], L, H, shift=frames % 4)
    assert not k.nonfinite.any()
    if frames > emu.delay(L):
        assert (k.min_gain < emu.ONE_BITS).all() and k.limited.all()


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_non_finite_samples_at_tile_edges_and_every_alignment(shift):
    L, H = 64, 128
    rng = np.random.default_rng(40 + shift)
    y = rng.uniform(-2.0, 2.0, (STREAMS, T + 13, 2)).astype(np.float32)
    y[0, T, 0] = np.nan                        # the second tile's first frame
    y[1, T - 1, 1] = np.inf                    # a tile's last frame: in the next tile's halo, counted once
    y[2, 0, :] = [-np.inf, np.nan]
    k, _ = both([y, y[:, 1:1 + SECOND]], L, H, shift)
    assert k.nonfinite.tolist() == [1, 1, 2]


def test_without_pre_gains_every_stream_has_gain_one():
    y = np.random.default_rng(50).uniform(-2.0, 2.0, (STREAMS, 300, 2)).astype(np.float32)
    both([y], 16, 0, gains=None)
