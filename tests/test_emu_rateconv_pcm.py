"""The PCM form of the sample-rate converter's kernel (airwave_amd/csrc/device/rateconv_tile.hpp, rateconv_tile_pcm) on emulated workgroups,
on the grid launch_rateconv_pcm makes, against the composition of the separately tested rules (tests/emu/emu_rateconv_pcm.cpp:
awp::decode_at, awrc::sequential, the gain product, awp::encode_dithered_at with the key rule of include/airwave_hip.h): output bytes, both
history slots, the counts, the records and the clipped word must agree exactly, whatever the formats, the call lengths and the byte
alignment of the caller's buffers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402
import emu_rateconv_pcm as pcm  # noqa: E402
import rateconv_cases as geo  # noqa: E402
from emu_rateconv_pcm import F32, S16, S24, S32, NONE, TPDF, TPDF_HP  # noqa: E402

STREAMS = 3
SEED = 0x5EED0123456789AB
FIRST = 11                       # the handle's first global stream
GAINS = [0.5, 1.25, 0.8]
# name -> (input format, output format, dither, fixed gains)
FORMS = {"s16-s16 tpdf": (S16, S16, TPDF, None), "s24-s24 tpdf_hp": (S24, S24, TPDF_HP, None), "f32-s16 gain": (F32, S16, NONE, GAINS),
         "s32-f32": (S32, F32, NONE, None), "f32-s32": (F32, S32, NONE, None)}


def lengths(pair, channels):
    L, M, T, D = emu.plan(*pair)
    tile = emu.tile(pair[0], pair[1], channels)
    return {"tile+1": emu.input_frames_for(tile + 1, L, M, D), "two tiles + 3": emu.input_frames_for(2 * tile, L, M, D) + 3}


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def converters(pair, C, dither, gains, S=STREAMS, first=FIRST):
    return (pcm.Converter(pair[0], pair[1], S, C, True, dither, SEED, first, gains), pcm.Converter(pair[0], pair[1], S, C, False, dither, SEED, first, gains))


def agree(k, q, where):
    """Everything a call leaves behind, kernel against composition."""
    assert np.array_equal(fbits(k.history()), fbits(q.history())), where
    assert np.array_equal(k.counts, q.counts) and np.array_equal(k.dev_counts, np.tile(k.counts, (k.n, 1))), where
    assert k.levels.tobytes() == q.levels.tobytes(), (where, k.levels, q.levels)
    assert k.clipped[0] == q.clipped[0] == q.levels["clipped"].sum(), where


def run_three_calls(pair, C, fi, fo, dither, gains, first_frames, seed):
    """first_frames, then 7 frames, then flush, with buffers at moving byte shifts; returns the kernel's converter."""
    rng = np.random.default_rng(seed)
    k, q = converters(pair, C, dither, gains)
    for step, n in enumerate((first_frames, 7)):
        x = pcm.random_input(rng, (STREAMS, n, C), fi)
        before = k.history().copy()
        yk, yq = k.process(x, fi, fo, shift=(seed + step) % 4, out_shift=(seed + 2 * step + 1) % 4), q.process(x, fi, fo)
        assert yk.shape == yq.shape and np.array_equal(yk, yq), (pair, C, fi, fo, step, int((yk != yq).sum()))
        assert np.array_equal(fbits(k.hist[k.cur ^ 1]), fbits(before)), step             # the slot it read is as it was
        agree(k, q, (pair, C, fi, fo, step))
    produced = int(k.counts[1])
    assert produced > 0
    yk, yq = k.flush(fo), q.flush(fo)
    assert yk.shape[1] > 0 and np.array_equal(yk, yq), (pair, C, fi, fo, "flush")
    agree(k, q, (pair, C, fi, fo, "flush"))
    assert not k.counts.any() and not k.history().any()                                # n restarts at 0 ...
    assert int(k.levels["frames"][0]) == produced + yk.shape[1]                        # ... and the records stay
    return k


@pytest.mark.parametrize("fo", pcm.FORMATS, ids=lambda f: "to-" + pcm.NAMES[f])
@pytest.mark.parametrize("fi", pcm.FORMATS, ids=lambda f: pcm.NAMES[f])
def test_all_format_pairs_on_the_smallest_tile(fi, fo):
    pair, C = (192000, 44100), 16
    assert emu.tile(pair[0], pair[1], C) == 50
    run_three_calls(pair, C, fi, fo, TPDF if (fi + fo) % 2 else TPDF_HP, None, lengths(pair, C)["tile+1"], seed=4 * fi + fo)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("pair,C", [((44100, 48000), 2), ((44100, 48000), 7), ((96000, 44100), 2)], ids=str)
def test_kernel_equals_the_composition(pair, C, form):
    fi, fo, dither, gains = FORMS[form]
    run_three_calls(pair, C, fi, fo, dither, gains, lengths(pair, C)["two tiles + 3"], seed=sorted(FORMS).index(form) + C)


@pytest.mark.parametrize("form", ["s24-s24 tpdf_hp", "f32-s16 gain"])
@pytest.mark.parametrize("pair,C,why", geo.CASES, ids=geo.IDS)
def test_kernel_equals_the_composition_over_the_tile_geometries(pair, C, why, form):
    """The shared table of tests/rateconv_cases.py in the two forms tests/test_gpu_rateconv_geometry.py runs on the device (s24 with
    per-stream gains): a case that fails here too is the tile's indexing, one that fails only there is the device."""
    fi, fo, dither, _ = FORMS[form]
    k = run_three_calls(pair, C, fi, fo, dither, GAINS, geo.first_call_frames(pair, C), seed=sorted(FORMS).index(form) + C)
    assert int(k.levels["frames"][0]) > 2 * emu.tile(pair[0], pair[1], C)


def test_a_tile_of_seven_outputs():
    """The handle next to the refusal boundary (tests/rateconv_cases.py): six workgroups per stream for 40 outputs, each of which encodes
    7 * 16 elements and leaves them through the ragged-end byte stores."""
    pair, C = geo.TINY_TILE
    L, M, T, D = emu.plan(*pair)
    assert emu.tile(pair[0], pair[1], C) == 7
    fi, fo, dither, _ = FORMS["s24-s24 tpdf_hp"]
    k = run_three_calls(pair, C, fi, fo, dither, GAINS, emu.input_frames_for(40, L, M, D), seed=5)
    assert int(k.levels["frames"][0]) >= 40


def test_the_dither_is_in_the_output():
    """TPDF against plain rounding on the same input: the two encodes differ, by one LSB at the most."""
    pair, C = (44100, 48000), 2
    x = pcm.random_input(np.random.default_rng(1), (STREAMS, lengths(pair, C)["tile+1"], C), S16)
    plain, dithered = converters(pair, C, NONE, None)[0], converters(pair, C, TPDF, None)[0]
    a, b = pcm.from_bytes(plain.process(x, S16, S16), S16).astype(np.int32), pcm.from_bytes(dithered.process(x, S16, S16), S16).astype(np.int32)
    assert 0.2 < np.mean(a != b) < 0.8 and np.abs(a - b).max() == 1


@pytest.mark.parametrize("fmt", [S16, S24], ids=lambda f: pcm.NAMES[f])
def test_buffers_shifted_by_zero_to_three_bytes(fmt):
    pair, C = (44100, 48000), 7
    tile = emu.tile(pair[0], pair[1], C)
    n = lengths(pair, C)["two tiles + 3"]
    x = pcm.random_input(np.random.default_rng(3), (STREAMS, n, C), fmt)
    dither = TPDF if fmt == S16 else TPDF_HP
    q = converters(pair, C, dither, None)[1]
    want = q.process(x, fmt, fmt)
    # byte phases of the tile boundaries (stream starts and tile starts) relative to a 4-byte word, over the cases below
    n_out, b = want.shape[1], pcm.BYTES[fmt]
    assert 2 * tile < n_out < 3 * tile
    unshifted = {((s * n_out + t * tile) * C * b) % 4 for s in range(STREAMS) for t in range(3)}
    assert unshifted == ({0, 1, 2, 3} if fmt == S24 else {0, 2})                       # every byte phase (s24), both phases (s16), even unshifted
    assert {(shift + u) % 4 for shift in range(4) for u in unshifted} == {0, 1, 2, 3}
    for shift in range(4):
        for out_shift in range(4):
            k = converters(pair, C, dither, None)[0]
            got = k.process(x, fmt, fmt, shift=shift, out_shift=out_shift)             # (_run asserts the sentinels on both sides)
            assert np.array_equal(got, want), (shift, out_shift)
            agree(k, q, (shift, out_shift))


@pytest.mark.parametrize("pair,C,form", [((44100, 48000), 2, "s16-s16 tpdf"), ((44100, 48000), 7, "s24-s24 tpdf_hp"), ((192000, 44100), 16, "f32-s16 gain")], ids=str)
def test_cutting_a_stream_at_every_boundary_changes_nothing(pair, C, form):
    fi, fo, dither, gains = FORMS[form]
    L, M, T, D = emu.plan(*pair)
    tile = emu.tile(pair[0], pair[1], C)
    fill = emu.input_frames_for(tile, L, M, D)
    cuts = sorted({1, D, D + 1, T - 1, T, emu.input_frames_for(tile - 1, L, M, D), fill, emu.input_frames_for(tile + 1, L, M, D),
                   emu.input_frames_for(2 * tile, L, M, D) + 3})                        # the boundaries of tests/test_emu_rateconv.py
    g = None if gains is None else gains[:1]
    x = pcm.random_input(np.random.default_rng(9), (1, cuts[-1], C), fi)
    whole = pcm.Converter(pair[0], pair[1], 1, C, True, dither, SEED, FIRST, g)
    y = np.concatenate([whole.process(x, fi, fo), whole.flush(fo)], axis=1)
    cut = pcm.Converter(pair[0], pair[1], 1, C, True, dither, SEED, FIRST, g)
    parts = [cut.process(x[:, a:b], fi, fo, shift=j % 4, out_shift=(j + 1) % 4) for j, (a, b) in enumerate(zip([0] + cuts[:-1], cuts))]
    assert parts[0].shape[1] == 0
    parts.append(cut.flush(fo))
    assert np.array_equal(np.concatenate(parts, axis=1), y)
    assert cut.levels.tobytes() == whole.levels.tobytes() and cut.clipped[0] == whole.clipped[0]
    ref = pcm.Converter(pair[0], pair[1], 1, C, False, dither, SEED, FIRST, g)
    assert np.array_equal(np.concatenate([ref.process(x, fi, fo), ref.flush(fo)], axis=1), y) and ref.levels.tobytes() == whole.levels.tobytes()


def test_sharding_three_streams_over_two_handles_changes_nothing():
    pair, C = (44100, 48000), 7
    fi, fo, dither, _ = FORMS["s24-s24 tpdf_hp"]
    n = lengths(pair, C)["two tiles + 3"]
    x = pcm.random_input(np.random.default_rng(6), (STREAMS, n, C), fi)
    whole = pcm.Converter(pair[0], pair[1], STREAMS, C, True, dither, SEED, FIRST, GAINS)
    y = np.concatenate([whole.process(x, fi, fo), whole.flush(fo)], axis=1)
    ys, levels, clipped = [], [], 0
    for a, b in ((0, 1), (1, 3)):
        part = pcm.Converter(pair[0], pair[1], b - a, C, True, dither, SEED, FIRST + a, GAINS[a:b])
        ys.append(np.concatenate([part.process(x[a:b], fi, fo), part.flush(fo)], axis=1))
        levels.append(part.levels)
        clipped += int(part.clipped[0])
    assert np.array_equal(np.concatenate(ys, axis=0), y)
    assert np.concatenate(levels).tobytes() == whole.levels.tobytes() and clipped == int(whole.clipped[0])
    # and first_stream matters: the same streams under another first stream get other noise
    other = pcm.Converter(pair[0], pair[1], STREAMS, C, True, dither, SEED, FIRST + 1, GAINS)
    assert not np.array_equal(other.process(x, fi, fo), y[:, :other.counts[1]])


def test_clipping_counts_are_exact_per_stream():
    pair, C = (44100, 48000), 2
    n = lengths(pair, C)["two tiles + 3"]
    x = pcm.random_input(np.random.default_rng(12), (STREAMS, n, C), F32)            # sigma 0.25 of full scale
    gains = [2.0, 2.5, 3.0]                                                           # full scale at 2, 1.6 and 1.33 sigma: about 5, 11 and 18 %
    k, q = converters(pair, C, TPDF, gains)
    yk, yq = k.process(x, F32, S16), q.process(x, F32, S16)
    share = q.levels["clipped"] / (yq.shape[1] * C)
    print("clipped share of the reference per stream:", share)
    assert np.all(share > 0.01) and np.all(share < 0.5)
    assert np.array_equal(yk, yq)
    agree(k, q, "clip")
    v = pcm.from_bytes(yq, S16)
    assert np.all(q.levels["clipped"] <= ((v == 32767) | (v == -32768)).sum(axis=(1, 2)))          # clipped samples sit at the rails
    assert np.all(q.levels["nonfinite"] == 0) and np.all(q.levels["frames"] == yq.shape[1])
    # the peak is |y| before the gain: the same input without a gain has the same peak
    plain = converters(pair, C, NONE, None)[0]
    plain.process(x, F32, F32)
    assert np.array_equal(plain.levels["peak"], k.levels["peak"]) and np.all(plain.levels["clipped"] == 0)


def test_a_nan_encodes_to_zero_and_counts_where_its_window_is():
    pair, C = (44100, 48000), 2
    L, M, T, D = emu.plan(*pair)
    tile = emu.tile(pair[0], pair[1], C)
    n = lengths(pair, C)["two tiles + 3"]
    at = tile * M // L + D - (T - 1)                                                   # the first input frame of the second tile
    xf = (0.1 * np.random.default_rng(5).standard_normal((STREAMS, n, C))).astype(np.float32)          # (10 sigma to full scale: nothing else clips)
    xf[1, at, 0] = np.nan
    x = pcm.to_bytes(xf, F32)
    k, q = converters(pair, C, TPDF, None)
    yk, yq = k.process(x, F32, S16), q.process(x, F32, S16)
    assert np.array_equal(yk, yq)
    agree(k, q, "nan")
    o = np.arange(yk.shape[1])
    i = o * M // L
    holds = (i + D - (T - 1) <= at) & (at <= i + D)
    assert holds[tile] and holds[tile - 1]                                             # outputs of both tiles among them
    assert np.all(pcm.from_bytes(yk, S16)[1, holds, 0] == 0)
    assert list(k.levels["nonfinite"]) == [0, int(holds.sum()), 0] and list(k.levels["clipped"]) == [0, int(holds.sum()), 0]
    assert k.clipped[0] == holds.sum() and np.isfinite(k.levels["peak"]).all()


@pytest.mark.parametrize("pair,C", [((44100, 48000), 2), ((44100, 48000), 7), ((192000, 44100), 16)], ids=str)
def test_f32_to_f32_without_dither_or_gain_is_the_float32_path(pair, C):
    rng = np.random.default_rng(C)
    n = lengths(pair, C)["two tiles + 3"]
    x, x7 = rng.standard_normal((STREAMS, n, C)).astype(np.float32), rng.standard_normal((STREAMS, 7, C)).astype(np.float32)
    old = emu.Converter(pair[0], pair[1], STREAMS, C, kernel=True)
    new = pcm.Converter(pair[0], pair[1], STREAMS, C, True, NONE, 0, 0, None, metering=False)
    for step, call in enumerate((x, x7)):
        want = old.process(call, shift=step, out_shift=step + 1)
        got = new.process(pcm.to_bytes(call, F32), F32, F32, shift=4 * step + 1, out_shift=2)          # (any byte, too)
        assert np.array_equal(fbits(pcm.from_bytes(got, F32)), fbits(want)), step
        assert np.array_equal(fbits(new.history()), fbits(old.history())) and np.array_equal(new.dev_counts, old.dev_counts)
    assert np.array_equal(fbits(pcm.from_bytes(new.flush(F32), F32)), fbits(old.flush()))
    assert new.clipped[0] == 0
