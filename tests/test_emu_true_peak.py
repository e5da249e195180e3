"""CPU thread emulation of the true-peak kernel (the code hipcc compiles, airwave_amd/csrc/device/truepeak_tile.hpp) against the
sequential rule of truepeak.hpp, bit for bit — records and carried history: calls shorter than the history, ragged and whole tiles, a
tile that ends inside the next one's halo, three streams (every other one 8 bytes off a 16-byte boundary when the frame count is odd),
buffers that start on any float, a second call of 7 frames, a NaN at a tile's first frame."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_true_peak as emu  # noqa: E402

T = emu.tile()
FRAMES = [1, 5, 11, 12, 13, T - 1, T, T + 1, T + 11, T + 12, 2 * T + 3]
STREAMS, SECOND = 3, 7


def both(y_calls, shift=0):
    k, s = emu.Meter(STREAMS, True), emu.Meter(STREAMS, False)
    for y in y_calls:
        k.process(y, shift)
        s.process(y)
        assert np.array_equal(k.call, s.call)
        assert np.array_equal(k.history().view(np.uint32), s.history().view(np.uint32))
    assert np.array_equal(k.tp, s.tp) and np.array_equal(k.nonfinite, s.nonfinite)
    return k, s


def test_tile_is_what_the_cases_assume():
    assert T == 2048


@pytest.mark.parametrize("frames", FRAMES)
def test_kernel_equals_the_sequential_rule_bit_for_bit(frames):
    rng = np.random.default_rng(frames)
    y = rng.uniform(-1.0, 1.0, (STREAMS, frames, 2)).astype(np.float32)
    y2 = rng.uniform(-1.0, 1.0, (STREAMS, SECOND, 2)).astype(np.float32)
    k, _ = both([y, y2], shift=frames % 4)
    assert k.tp.all() and not k.nonfinite.any()
    assert np.all(k.tp.view(np.float32) >= np.abs(np.concatenate([y, y2], axis=1)).max(axis=1))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_a_nan_at_a_tiles_first_frame_and_every_alignment(shift):
    rng = np.random.default_rng(40 + shift)
    y = rng.uniform(-1.0, 1.0, (STREAMS, T + 13, 2)).astype(np.float32)
    y[0, T, 0] = np.nan                        # the second tile's first frame: the halo of nothing, the window of the next 11 frames
    y[1, T - 1, 1] = np.inf                    # a tile's last frame: in the next tile's halo, counted once
    y[2, 0, :] = [-np.inf, np.nan]
    k, _ = both([y, y[:, 1:1 + SECOND]], shift)
    assert k.nonfinite.tolist() == [1, 1, 2] and np.isfinite(k.tp.view(np.float32)).all()


def test_call_local_peak_alone_leaves_the_records():
    y = np.random.default_rng(50).uniform(-1.0, 1.0, (STREAMS, 300, 2)).astype(np.float32)
    k, s = emu.Meter(STREAMS, True, records=False), emu.Meter(STREAMS, False)
    k.process(y)
    s.process(y)
    assert np.array_equal(k.call, s.call) and not k.tp.any() and not k.nonfinite.any()
