"""The sample-rate converter's kernel (airwave_amd/csrc/device/rateconv_tile.hpp) on emulated workgroups, on exactly the grid
launch_rateconv makes, against the sequential rule of rateconv.hpp: outputs, both history slots and the counts must agree bit for bit,
whatever the call lengths, the channel count and the alignment of the caller's buffers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402
import rateconv_cases as geo  # noqa: E402

PAIRS = [(48000, 96000), (96000, 48000), (44100, 48000), (48000, 44100), (192000, 44100)]
CHANNELS = [1, 2, 7, 16]
STREAMS = 3                      # odd lengths and channel counts put streams 1 and 2 off the 16-byte boundaries


def lengths(pair, channels):
    """Input lengths around the handle's own boundaries."""
    L, M, T, D = emu.plan(*pair)
    tile = emu.tile(pair[0], pair[1], channels)
    fill = emu.input_frames_for(tile, L, M, D)               # the fewest input frames that fill one tile of output
    return {"one": 1, "D": D, "D+1": D + 1, "T-1": T - 1, "T": T, "tile-1": emu.input_frames_for(tile - 1, L, M, D), "tile": fill,
            "tile+1": emu.input_frames_for(tile + 1, L, M, D), "two tiles + 3": emu.input_frames_for(2 * tile, L, M, D) + 3}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_the_tile_is_a_function_of_the_handle_and_fits_the_lds():
    for pair in PAIRS + [(96000, 44100), (44100, 192000), (88200, 48000)]:
        L, M, T, D = emu.plan(*pair)
        for C in range(1, 17):
            tile = emu.tile(pair[0], pair[1], C)
            span = -(-tile * M // L) + T

            def floats(span, tile):
                """The input image (segments of 32 frames behind a halo of 3, one halo more) and the gathered outputs."""
                return ((((span - 1) >> 5) + 1) * 35 * C + 3 * C + 3) // 4 * 4 + tile * C
            assert 1 <= tile <= 4096 and floats(span, tile) <= emu.lds_floats() == 12288                      # 48 KB, static
            assert tile == 4096 or floats(-(-(tile + 1) * M // L) + T, tile + 1) > emu.lds_floats()           # and no longer one does
    assert emu.plan(192000, 44100)[2] == 418 and emu.plan(96000, 48000)[:3] == (1, 2, 192) and emu.plan(48000, 96000)[0] == 2


def test_the_first_output_needs_d_plus_one_frames():
    for pair in PAIRS:
        L, M, T, D = emu.plan(*pair)
        rc = emu.Converter(pair[0], pair[1], 1, 1, kernel=False)
        assert rc.output_frames(D) == 0 and rc.output_frames(D + 1) == -(-L // M)           # every output at input time < 1
        assert emu.input_frames_for(1, L, M, D) == D + 1


def check_calls(pair, channels, n, i, rng, name):
    """n frames, then 7, then the flush, kernel against the sequential rule: outputs, both history slots and the counts."""
    k = emu.Converter(pair[0], pair[1], STREAMS, channels, kernel=True)
    q = emu.Converter(pair[0], pair[1], STREAMS, channels, kernel=False)
    x = rng.standard_normal((STREAMS, n, channels)).astype(np.float32)
    x7 = rng.standard_normal((STREAMS, 7, channels)).astype(np.float32)
    consumed = produced = 0
    for step, call in enumerate((x, x7)):
        before = k.history().copy()
        yk, yq = k.process(call, shift=(i + step) % 4, out_shift=(i + 2 * step + 1) % 4), q.process(call)
        consumed += call.shape[1]
        assert yk.shape[1] == available(k, consumed) - produced, (name, step)
        produced += yk.shape[1]
        assert same(yk, yq), (name, step)
        assert same(k.history(), q.history()), (name, step)                     # the slot the call wrote
        assert same(k.hist[k.cur ^ 1], before), (name, step)                    # the slot it read is as it was
        assert np.array_equal(k.counts, q.counts) and np.array_equal(k.counts, [consumed, produced]), (name, step)
        assert np.array_equal(k.dev_counts, np.tile(k.counts, (STREAMS, 1))), (name, step)
    yk, yq = k.flush(), q.flush()
    assert same(yk, yq), (name, "flush")
    assert produced + yk.shape[1] == -(-(consumed * k.L) // k.M), (name, "flush")
    assert not k.counts.any() and not k.history().any() and not k.dev_counts.any()
    return produced


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_kernel_equals_the_sequential_rule(pair, channels):
    rng = np.random.default_rng(pair[0] + 31 * channels)
    for i, (name, n) in enumerate(lengths(pair, channels).items()):
        check_calls(pair, channels, n, i, rng, name)


@pytest.mark.parametrize("pair,channels,why", geo.CASES, ids=geo.IDS)
def test_kernel_equals_the_sequential_rule_over_the_tile_geometries(pair, channels, why):
    """The shared table of tests/rateconv_cases.py, which tests/test_gpu_rateconv_geometry.py runs on the device: a case that fails here too
    is the tile's indexing, one that fails only there is the device."""
    tile = emu.tile(pair[0], pair[1], channels)
    rng = np.random.default_rng(pair[0] + 31 * channels + 1)
    for i, n in enumerate((geo.first_call_frames(pair, channels), lengths(pair, channels)["tile+1"])):
        produced = check_calls(pair, channels, n, i + channels, rng, why)
        assert produced > (2 - i) * tile


@pytest.mark.parametrize("handle", [geo.TINY_TILE, geo.SMALLEST_MEASURING], ids=str)
def test_a_tile_of_a_handful_of_outputs(handle):
    """The handles at the refusal boundary (tests/rateconv_cases.py): tiles of 7 and 12 outputs, so a call of 40 outputs is 6 or 4
    workgroups per stream, each with an input image of nearly the whole LDS."""
    pair, channels = handle
    L, M, T, D = emu.plan(*pair)
    tile = emu.tile(pair[0], pair[1], channels)
    assert tile == geo.BOUNDARY_TILES[handle] == geo.tile_by_the_formula(L, M, T, channels)
    produced = check_calls(pair, channels, emu.input_frames_for(40, L, M, D), 1, np.random.default_rng(tile), handle)
    assert 40 <= produced <= 42 and produced > 3 * tile


def available(rc, consumed):
    """Outputs that exist after `consumed` input frames: max(0, ceil((N - D) L / M))."""
    return max(0, -((consumed - rc.D) * rc.L // -rc.M))


@pytest.mark.parametrize("pair", [(44100, 48000), (192000, 44100)], ids=str)
def test_positions_past_two_to_the_31(pair):
    """A stream that has run for 3 * 2^33 + 5 frames: the counts and a history as such a stream would carry them."""
    C = 2
    n = lengths(pair, C)["tile+1"]
    rng = np.random.default_rng(2)
    x = rng.standard_normal((STREAMS, n, C)).astype(np.float32)
    k = emu.Converter(pair[0], pair[1], STREAMS, C, kernel=True)
    q = emu.Converter(pair[0], pair[1], STREAMS, C, kernel=False)
    consumed = 3 * 2 ** 33 + 5
    hist = rng.standard_normal(k.history().shape).astype(np.float32)
    for rc in (k, q):
        rc.counts[:] = [consumed, available(rc, consumed)]
        rc.history()[:] = hist
    yk, yq = k.process(x, shift=1), q.process(x)
    assert yk.shape[1] > 0 and same(yk, yq) and same(k.history(), q.history())
    assert np.array_equal(k.counts, q.counts) and int(k.counts[0]) == consumed + n and np.array_equal(k.dev_counts, np.tile(k.counts, (STREAMS, 1)))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_buffers_shifted_by_zero_to_three_floats(shift):
    pair, C = (44100, 48000), 7
    n = lengths(pair, C)["two tiles + 3"]
    x = np.random.default_rng(3).standard_normal((STREAMS, n, C)).astype(np.float32)
    q = emu.Converter(pair[0], pair[1], STREAMS, C, kernel=False)
    want = q.process(x)
    for out_shift in range(4):
        k = emu.Converter(pair[0], pair[1], STREAMS, C, kernel=True)
        assert same(k.process(x, shift=shift, out_shift=out_shift), want)
        assert same(k.history(), q.history())


@pytest.mark.parametrize("pair,channels", [(p, 2) for p in PAIRS] + [((44100, 48000), 7), ((192000, 44100), 16)], ids=str)
def test_cutting_a_stream_at_every_boundary_changes_no_bit(pair, channels):
    cuts = sorted(set(lengths(pair, channels).values()))
    x = np.random.default_rng(9).standard_normal((1, cuts[-1], channels)).astype(np.float32)
    whole = emu.Converter(pair[0], pair[1], 1, channels, kernel=True)
    y = np.concatenate([whole.process(x), whole.flush()], axis=1)
    assert y.shape[1] == -(-(cuts[-1] * whole.L) // whole.M)
    cut = emu.Converter(pair[0], pair[1], 1, channels, kernel=True)
    parts = [cut.process(x[:, a:b], shift=j % 4) for j, (a, b) in enumerate(zip([0] + cuts[:-1], cuts))]
    assert parts[0].shape[1] == 0                                              # one frame: nothing yet
    parts.append(cut.flush())
    assert same(np.concatenate(parts, axis=1), y)
    ref = emu.Converter(pair[0], pair[1], 1, channels, kernel=False)
    assert same(np.concatenate([ref.process(x), ref.flush()], axis=1), y)


@pytest.mark.parametrize("pair", [(44100, 48000), (96000, 48000), (192000, 44100)], ids=str)
def test_a_nan_reaches_exactly_the_outputs_whose_windows_hold_it(pair):
    C = 2
    L, M, T, D = emu.plan(*pair)
    tile = emu.tile(pair[0], pair[1], C)
    n = lengths(pair, C)["two tiles + 3"]
    at = tile * M // L + D - (T - 1)                                           # the first input frame of the second tile
    assert 0 < at < n
    x = np.random.default_rng(5).standard_normal((STREAMS, n, C)).astype(np.float32)
    x[1, at, 0] = np.nan
    k = emu.Converter(pair[0], pair[1], STREAMS, C, kernel=True)
    q = emu.Converter(pair[0], pair[1], STREAMS, C, kernel=False)
    yk, yq = k.process(x), q.process(x)
    assert same(yk, yq)
    o = np.arange(yk.shape[1])
    i = o * M // L
    holds = (i + D - (T - 1) <= at) & (at <= i + D)
    assert holds.sum() >= T * L // M - 1 and holds[tile] and holds[tile - 1]   # outputs of both tiles among them
    want = np.zeros(yk.shape, bool)
    want[1, holds, 0] = True
    assert np.array_equal(np.isnan(yk), want)
