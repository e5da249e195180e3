"""The measuring forms of the sample-rate converter's kernel (airwave_amd/csrc/device/rateconv_tile.hpp, rateconv_tile_pcm_tp and
rateconv_tile_tp_measure) on emulated workgroups, on the grid launch_rateconv_pcm_tp makes, against the composition of the separately
tested rules (tests/emu/emu_rateconv_tp.py: awp::decode_at -> awrc::sequential -> awrc::true_peak_sequential, element by element): every
field of the true-peak records and the carried v history must agree bit for bit, and the output bytes, the levels, the clip counts, the
input history and the counts must be those of the present PCM kernel with measuring off.

The call sequence is: two measuring tiles + 5 outputs, about 7 outputs, a call that produces none, the flush.  Output counts that a ratio
cannot produce are replaced by the nearest it can (48 -> 96 kHz produces even counts only), and a converter that raises the rate produces
at least one frame per input frame once it has started, so there the call without outputs leads the sequence."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402
import emu_rateconv_pcm as pcm  # noqa: E402
import emu_rateconv_tp as tp  # noqa: E402
import rateconv_cases as geo  # noqa: E402
from emu_rateconv_pcm import F32, S16, S24, NONE, TPDF  # noqa: E402

STREAMS = 2
SEED = 0x5EED0123456789AB
FIRST = 11
GAINS = [0.5, 1.25]
SHAPES = [((44100, 48000), 2), ((96000, 44100), 2), ((48000, 96000), 3), ((192000, 44100), 16)]
SHORT = ((48000, 8000), 16)                               # a measuring tile of 5 outputs: a tile's predecessors span two earlier tiles and the history
FORMS = {"f32-f32": (F32, F32, NONE, None), "s16-s24 tpdf gain": (S16, S24, TPDF, GAINS)}


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def available(N, L, M, D):
    return max(0, -((N - D) * L // -M))


def call_lengths(pair, C):
    """Input frames of the calls: (none, two measuring tiles + 5, about 7, none-first?) -> list of (frames, lo, hi) with the bounds on the outputs."""
    L, M, T, D = emu.plan(*pair)
    tile = tp.tp_tile(pair[0], pair[1], C)
    calls, N = [], 0
    if L > M:                                             # every later input frame produces: the call without outputs comes first
        calls.append((1, 0, 0))
        N = 1
    n1 = emu.input_frames_for(2 * tile + 5, L, M, D) - N
    calls.append((n1, 2 * tile + 5, 2 * tile + 10))
    N += n1
    for n2 in range(1, 64):                               # 7 .. 10 outputs, and (lowering the rate) a frame behind it that produces nothing
        made = available(N + n2, L, M, D) - available(N, L, M, D)
        if 7 <= made <= 10 and (L > M or available(N + n2 + 1, L, M, D) == available(N + n2, L, M, D)):
            break
    else:                                                 # the ratio makes no such count (8 -> 48 kHz: six a frame): the most below 7 it can
        assert L > M, "no call of 7 .. 10 outputs"
        n2 = max(n for n in range(1, 64) if available(N + n, L, M, D) - available(N, L, M, D) < 7)
        made = available(N + n2, L, M, D) - available(N, L, M, D)
        assert 1 <= made < 7
        calls.append((n2, made, made))
        return calls
    calls.append((n2, 7, 10))
    if L < M:
        calls.append((1, 0, 0))
    return calls


def agree(k, q, where, plain=None):
    """Everything a call leaves behind: the kernel against the composition, and against the PCM kernel with measuring off."""
    assert k.records.tobytes() == q.records.tobytes(), (where, k.records, q.records)
    assert np.array_equal(fbits(k.tp_history()), fbits(q.tp_history())), where
    assert np.array_equal(fbits(k.history()), fbits(q.history())), where
    assert np.array_equal(k.counts, q.counts) and np.array_equal(k.dev_counts, np.tile(k.counts, (k.n, 1))), where
    assert k.levels.tobytes() == q.levels.tobytes() and k.clipped[0] == q.clipped[0], where
    if plain is not None:
        assert np.array_equal(fbits(k.history()), fbits(plain.history())) and np.array_equal(k.dev_counts, plain.dev_counts), where
        assert k.levels.tobytes() == plain.levels.tobytes() and k.clipped[0] == plain.clipped[0], where


def trio(pair, C, dither, gains, S=STREAMS, first=FIRST):
    g = None if gains is None else gains[:S]
    return (tp.Kernel(pair[0], pair[1], S, C, dither, SEED, first, g), tp.Composition(pair[0], pair[1], S, C, dither, SEED, first, g),
            pcm.Converter(pair[0], pair[1], S, C, True, dither, SEED, first, g))


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("pair,C", SHAPES + [SHORT], ids=str)
def test_kernel_equals_the_composition_and_leaves_the_bytes_alone(pair, C, form):
    tile = tp.tp_tile(pair[0], pair[1], C)
    assert tile == 5 if (pair, C) == SHORT else tile >= 39
    check_calls(pair, C, form, call_lengths(pair, C))


@pytest.mark.parametrize("pair,C,why", geo.CASES, ids=geo.IDS)
def test_kernel_equals_the_composition_over_the_tile_geometries(pair, C, why):
    """The shared table of tests/rateconv_cases.py, which tests/test_gpu_rateconv_geometry.py runs on the device, through process and
    through measure: a case that fails here too is the tile's indexing, one that fails only there is the device."""
    assert tp.tp_tile(pair[0], pair[1], C) == emu.tile(pair[0], pair[1], C) - tp.HISTORY >= 1
    xs, q = check_calls(pair, C, "s16-s24 tpdf gain", call_lengths(pair, C))
    measure_equals_the_composition(pair, C, xs, q)


def test_a_measuring_tile_of_one_output():
    """The smallest tile that leaves a measuring tile (tests/rateconv_cases.py: 12 outputs, so 1): every workgroup computes its 11
    predecessors again for one output of its own, and the first 11 take theirs from the carried history."""
    pair, C = geo.SMALLEST_MEASURING
    L, M, T, D = emu.plan(*pair)
    assert tp.tiles(L, M, T, C) == (12, 1) and tp.tiles(L, M, T, geo.TINY_TILE[1]) == (7, -4)
    lengths = [(emu.input_frames_for(14, L, M, D), 14, 14), (emu.input_frames_for(23, L, M, D) - emu.input_frames_for(14, L, M, D), 9, 9), (1, 0, 0)]
    xs, q = check_calls(pair, C, "s16-s24 tpdf gain", lengths)
    measure_equals_the_composition(pair, C, xs, q)


def measure_equals_the_composition(pair, C, xs, q):
    """measure and measure_flush over the calls xs of check_calls leave the records q.records that process and flush left."""
    fi, _, dither, gains = FORMS["s16-s24 tpdf gain"]
    k = tp.Kernel(pair[0], pair[1], STREAMS, C, dither, SEED, FIRST, gains)
    total = sum(k.measure(x, fi, shift=(i + 1) % 4) for i, x in enumerate(xs))
    total += k.measure_flush()
    assert k.records.tobytes() == q.records.tobytes() and np.all(k.records["frames"] == total), (pair, C, k.records, q.records)
    assert not k.levels.view(np.uint8).any() and k.clipped[0] == 0 and not k.counts.any() and not k.tp_history().any()


def check_calls(pair, C, form, lengths):
    """The calls `lengths` (call_lengths) and the flush through the measuring kernel, the composition and the PCM kernel with measuring
    off; returns the calls' inputs and the composition."""
    fi, fo, dither, gains = FORMS[form]
    rng = np.random.default_rng(pair[0] + C + len(form))
    k, q, plain = trio(pair, C, dither, gains)
    tile = tp.tp_tile(pair[0], pair[1], C)
    total, xs = 0, []
    for step, (n, lo, hi) in enumerate(lengths):
        x = pcm.random_input(rng, (STREAMS, n, C), fi)
        xs.append(x)
        before, slot = k.tp_history().copy(), k.tp_cur
        yk, yq, yp = k.process(x, fi, fo, shift=step % 4, out_shift=(2 * step + 1) % 4), q.process(x, fi, fo), plain.process(x, fi, fo)
        assert lo <= yk.shape[1] <= hi, (step, yk.shape[1], lo, hi)
        assert yk.shape == yq.shape and np.array_equal(yk, yq) and np.array_equal(yk, yp), (pair, C, form, step)
        if yk.shape[1] == 0:                              # a call without outputs leaves the carried v where and as it is
            assert k.tp_cur == slot
        else:
            assert k.tp_cur == slot ^ 1 and np.array_equal(fbits(k.tp_hist[slot]), fbits(before))          # the slot it read is as it was
        if 0 < yk.shape[1] < tp.HISTORY:                  # fewer than 11 outputs: old frames move up, new ones follow
            assert np.array_equal(fbits(k.tp_history()[:, :tp.HISTORY - yk.shape[1]]), fbits(before[:, yk.shape[1]:]))
        agree(k, q, (pair, C, form, step), plain)
        total += yk.shape[1]
    assert total > 2 * tile and np.all(k.records["frames"] == total) and np.all(k.records["true_peak"] >= k.records["sample_peak"])
    assert np.array_equal(k.records["sample_peak"], k.levels["peak"])                  # both meters saw the same calls
    yk, yq, yp = k.flush(fo), q.flush(fo), plain.flush(fo)
    assert yk.shape[1] > 0 and np.array_equal(yk, yq) and np.array_equal(yk, yp)
    agree(k, q, (pair, C, form, "flush"), plain)
    assert not k.counts.any() and not k.history().any() and not k.tp_history().any()   # n restarts at 0 and v = 0 before it ...
    assert np.all(k.records["frames"] == total + yk.shape[1])                          # ... and the records stay
    return xs, q


def exact_cuts(pair, C, chunks):
    """Input cut points after which the output counts grow by `chunks` exactly, from some start; None where the ratio cannot."""
    L, M, T, D = emu.plan(*pair)
    for start in range(D + 1, D + 400):
        cuts, ok = [start], True
        for c in chunks:
            want = available(cuts[-1], L, M, D) + c
            N = emu.input_frames_for(want, L, M, D)          # the fewest input frames after which `want` outputs exist
            if available(N, L, M, D) != want:
                ok = False
                break
            cuts.append(N)
        if ok:
            return cuts
    return None


@pytest.mark.parametrize("pair,C", SHAPES + [SHORT], ids=str)
def test_cutting_a_stream_at_ragged_points_changes_no_bit(pair, C):
    fi, fo, dither, gains = FORMS["s16-s24 tpdf gain"]
    L, M, T, D = emu.plan(*pair)
    tile = tp.tp_tile(pair[0], pair[1], C)
    chunks = [1, 10, 11, 12, tile - 1]
    if pair == (48000, 96000):                            # even counts only
        chunks = [2, 10, 12, 12, tile - 1 + (tile - 1) % 2]
    cuts = exact_cuts(pair, C, chunks)
    assert cuts is not None, (pair, chunks)
    cuts = [0, 1] + cuts + [cuts[-1] + emu.input_frames_for(tile + 3, L, M, D)]
    x = pcm.random_input(np.random.default_rng(9 + C), (1, cuts[-1], C), fi)
    whole = tp.Kernel(pair[0], pair[1], 1, C, dither, SEED, FIRST, gains[:1])
    y = np.concatenate([whole.process(x, fi, fo), whole.flush(fo)], axis=1)
    cut = tp.Kernel(pair[0], pair[1], 1, C, dither, SEED, FIRST, gains[:1])
    parts = [cut.process(x[:, a:b], fi, fo, shift=j % 4, out_shift=(j + 1) % 4) for j, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
    assert [p.shape[1] for p in parts[2:2 + len(chunks)]] == chunks and parts[0].shape[1] == 0
    parts.append(cut.flush(fo))
    assert np.array_equal(np.concatenate(parts, axis=1), y)
    assert cut.records.tobytes() == whole.records.tobytes() and cut.levels.tobytes() == whole.levels.tobytes()
    ref = tp.Composition(pair[0], pair[1], 1, C, dither, SEED, FIRST, gains[:1])
    assert np.array_equal(np.concatenate([ref.process(x, fi, fo), ref.flush(fo)], axis=1), y) and ref.records.tobytes() == whole.records.tobytes()


def test_sharding_streams_over_two_handles_changes_no_bit():
    pair, C = (44100, 48000), 2
    fi, fo, dither, _ = FORMS["s16-s24 tpdf gain"]
    gains = [0.5, 1.25, 0.8]
    n = call_lengths(pair, C)[1][0]
    x = pcm.random_input(np.random.default_rng(6), (3, n, C), fi)
    whole = tp.Kernel(pair[0], pair[1], 3, C, dither, SEED, FIRST, gains)
    y = np.concatenate([whole.process(x, fi, fo), whole.flush(fo)], axis=1)
    ys, recs = [], []
    for a, b in ((0, 1), (1, 3)):
        part = tp.Kernel(pair[0], pair[1], b - a, C, dither, SEED, FIRST + a, gains[a:b])
        ys.append(np.concatenate([part.process(x[a:b], fi, fo), part.flush(fo)], axis=1))
        recs.append(part.records)
    assert np.array_equal(np.concatenate(ys, axis=0), y) and np.concatenate(recs).tobytes() == whole.records.tobytes()


@pytest.mark.parametrize("pair,C", [((44100, 48000), 2), ((192000, 44100), 16)], ids=str)
def test_nan_and_inf_enter_as_zero(pair, C):
    L, M, T, D = emu.plan(*pair)
    tile = tp.tp_tile(pair[0], pair[1], C)
    n = emu.input_frames_for(2 * tile + 5, L, M, D)
    xf = (0.1 * np.random.default_rng(5).standard_normal((STREAMS, n, C))).astype(np.float32)
    at = (tile - 1) * M // L + D - 3                      # inside the windows of the first tile's last output and of the second tile's recomputed predecessors
    xf[1, at, 0], xf[1, at + 1, C - 1], xf[0, 5, 0] = np.nan, np.inf, -np.inf
    x = pcm.to_bytes(xf, F32)
    k, q, plain = trio(pair, C, NONE, None)
    yk, yq = k.process(x, F32, F32), q.process(x, F32, F32)
    assert np.array_equal(yk, yq) and np.array_equal(yk, plain.process(x, F32, F32))
    y = pcm.from_bytes(yk, F32)
    bad = ~np.isfinite(y)
    assert bad[1, tile - 1, 0] and bad[1, tile, 0] and bad[0, 0, 0] and not bad[0, :, 1:].any()          # both tiles of stream 1 hold the NaN
    agree(k, q, "nan", plain)
    assert np.isfinite(k.records["true_peak"]).all() and np.isfinite(k.records["sample_peak"]).all() and np.isfinite(k.tp_history()).all()
    # ... and what they read is what the cleaned outputs alone give
    clean = np.zeros(STREAMS, tp.TRUE_PEAK)
    tp.rule(np.where(bad, np.float32(0), y), np.zeros((STREAMS, tp.HISTORY, C), np.float32), clean)
    assert clean.tobytes() == k.records.tobytes()
    assert np.array_equal(k.records["sample_peak"], k.levels["peak"]) and list(k.levels["nonfinite"]) == [int(bad[0].sum()), int(bad[1].sum())]


@pytest.mark.parametrize("pair,C", [((96000, 44100), 2), ((48000, 96000), 3)], ids=str)
def test_measure_moves_what_process_moves_and_writes_nothing(pair, C):
    fi, fo, dither, gains = FORMS["s16-s24 tpdf gain"]
    rng = np.random.default_rng(C)
    lens = [n for n, _, _ in call_lengths(pair, C)]
    xs = [pcm.random_input(rng, (STREAMS, n, C), fi) for n in lens]
    k, q, plain = trio(pair, C, dither, gains)
    for step, x in enumerate(xs[:-1]):                    # (Kernel._run asserts that measure leaves the output buffer alone)
        assert k.measure(x, fi, shift=step + 1) == q.measure(x, fi) == plain.process(x, fi, fo).shape[1]
        assert not k.levels.view(np.uint8).any() and k.clipped[0] == 0                 # no levels record, no clip count
        assert k.records.tobytes() == q.records.tobytes() and np.array_equal(fbits(k.tp_history()), fbits(q.tp_history()))
        assert np.array_equal(fbits(k.history()), fbits(plain.history())) and np.array_equal(k.dev_counts, plain.dev_counts)
    # process behind measure writes what process behind process writes
    plain.levels[:] = 0
    plain.clipped[:] = 0
    yk, yp = k.process(xs[-1], fi, fo), plain.process(xs[-1], fi, fo)
    assert np.array_equal(yk, yp) and k.levels.tobytes() == plain.levels.tobytes() and k.clipped[0] == plain.clipped[0]
    q.process(xs[-1], fi, fo)
    assert k.records.tobytes() == q.records.tobytes()
    # measure_flush is the flush without bytes, and ends with the reset: the second pass is the first pass
    assert k.measure_flush() == q.measure_flush() == plain.flush(fo).shape[1] > 0
    assert k.records.tobytes() == q.records.tobytes() and not k.counts.any() and not k.tp_history().any() and not k.history().any()
    first_pass = k.records.copy()
    k.records[:] = 0
    for x in xs:
        k.process(x, fi, fo)
    k.flush(fo)
    assert k.records.tobytes() == first_pass.tobytes()
