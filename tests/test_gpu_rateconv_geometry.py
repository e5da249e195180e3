"""Every form of the sample-rate converter's kernel over its tile geometries on the device: the shared table of tests/rateconv_cases.py (the
4-channel block with one, three and four work items per output, one channel, a tile shorter than L, one coefficient row for a whole wave,
M = 640, tap counts that run every loop of rc_output, an upward pair with M = 1) through aw_rateconv_kernel, aw_rateconv_pcm_kernel and the
two measuring kernels, with the helpers and the references of tests/test_gpu_rateconv.py, _pcm.py and _tp.py: the sequential rule and the
composition bit for bit.  The emulated suite runs the same table (tests/test_emu_rateconv*.py): a case that fails there too is the tile's
indexing, one that fails only here is the device (its 16-byte loads, the compiler's contraction, LDS, alignment).

The float64 truth of the float32 cases shares nothing with the library: tests/rateconv_ref.py's numpy coefficients and its float64
evaluation.  Its bound is derived: the float32 result makes T roundings on the way (the products are fused, so one per tap) and the
library's coefficient is the formula's rounded once more, so |y - y64| <= (T + 1) * 2^-24 * sum_k |c[p][k]| |x[i + D - k]| per sample,
the bound of tests/test_gpu_rateconv.py with T + 1 in place of T.

The refusal boundary (tests/rateconv_cases.py; searched on the CPU by tests/test_rateconv_host.py): a pair without a tile is refused by
aw_rateconv_create, a tile of 7 outputs converts and refuses aw_tp_rateconv_set, a tile of 12 measures with a measuring tile of 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402
import emu_rateconv_pcm as pcm  # noqa: E402
import emu_rateconv_tp as tp  # noqa: E402
import rateconv_cases as geo  # noqa: E402
import rateconv_ref as ref  # noqa: E402
import test_gpu_rateconv as f32  # noqa: E402
import test_gpu_rateconv_pcm as gp  # noqa: E402
import test_gpu_rateconv_tp as gt  # noqa: E402
from emu_rateconv_pcm import S16, S24, TPDF  # noqa: E402
from test_gpu_rateconv import G  # noqa: E402,F401  (the module's fixture: torch, the package and a context on torch's stream)

pytestmark = pytest.mark.gpu

STREAMS = 3
PCM_FORMS = {"s24-s24 tpdf_hp": gp.GAINS, "f32-s16 gain": "form"}          # form -> the gains of gp.case: per stream in both
SHIFTED = [((44100, 48000), 12), ((192000, 44100), 4)]                     # frames 48 bytes apart; rows of 418 taps
SHORT_CALLS = [geo.SHORT_TILE, geo.ONE_ROW]
assert all(c in geo.CB4 for c in SHIFTED)


def refusal(G, fn, *args):
    """(name, message) of the AirwaveError that fn(*args) raises, or None; caught here, for the reason gp.refused gives."""
    try:
        fn(*args)
    except G.aw.AirwaveError as err:
        return err.name, str(err)
    return None


@pytest.mark.parametrize("pair,C,why", geo.CASES, ids=geo.IDS)
def test_float32_kernel_equals_the_sequential_rule_and_stays_within_the_float64_bound(G, pair, C, why):
    L, M, T, D = emu.plan(*pair)
    worst = f32.check_three_calls(G, pair, C, c=ref.coefficients(L, M), roundings=T + 1)          # (prints the ratio; the tile; the sentinels)
    assert worst <= 1.0


@pytest.mark.parametrize("form", sorted(PCM_FORMS))
@pytest.mark.parametrize("pair,C,why", geo.CASES, ids=geo.IDS)
def test_pcm_kernel_equals_the_composition(G, pair, C, why, form):
    gp.check_three_calls(G, pair, C, form, gains=PCM_FORMS[form])


@pytest.mark.parametrize("pair,C,why", geo.CASES, ids=geo.IDS)
def test_measuring_kernels_equal_the_composition(G, pair, C, why):
    assert tp.tp_tile(pair[0], pair[1], C) >= 1
    gt.check_process_and_measure(G, pair, C)


@pytest.mark.parametrize("pair,C", SHIFTED, ids=str)
def test_a_float32_buffer_shifted_by_one_to_three_floats_changes_no_bit(G, pair, C):
    x, _, want = f32.case(pair, C)
    for shift in (1, 2, 3):
        rc = G.aw.RateConverter(pair[0], pair[1], x.shape[0], C, ctx=G.ctx)
        assert f32.same(f32.process(G, rc, x, shift=shift), want[0]), shift


def short_cuts(pair, n):
    """Cut points of n input frames: 1 frame, D frames (the first outputs), 5 more outputs' worth, 11 outputs' worth, the rest; and the
    outputs of each call.  The two calls in the middle produce fewer than 11 outputs and then at least 11."""
    L, M, T, D = emu.plan(*pair)
    available = lambda N: max(0, -((N - D) * L // -M))          # noqa: E731
    a = 1 + D
    b = emu.input_frames_for(available(a) + 5, L, M, D)
    c = emu.input_frames_for(available(b) + 11, L, M, D)
    cuts = [0, 1, a, b, c, n]
    made = [available(hi) - available(lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert c < n and made[0] == 0 and 1 <= made[1] < 11 and 5 <= made[2] < 11 and 11 <= made[3] < 22 and made[4] > 22, (cuts, made)
    return cuts, made


def in_calls(x, cuts):
    return [np.ascontiguousarray(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("pair,C", SHORT_CALLS, ids=str)
def test_short_calls_change_no_bit_in_any_kernel(G, pair, C):
    # the float32 kernel
    x, _, want = f32.case(pair, C)
    cuts, made = short_cuts(pair, x.shape[1])
    rc = G.aw.RateConverter(pair[0], pair[1], STREAMS, C, ctx=G.ctx)
    parts = [f32.process(G, rc, part) for part in in_calls(x, cuts)]
    assert [p.shape[1] for p in parts[:-1]] == made[:-1] and f32.same(np.concatenate(parts, axis=1), want[0])
    # the PCM kernel
    form = "s24-s24 tpdf_hp"
    fi, fo, dither, _ = gp.FORMS[form]
    x, _, want, levels, _ = gp.case(pair, C, form, gains=gp.GAINS)
    assert x.shape[1] == cuts[-1]
    rc = gp.converter(G, pair, STREAMS, C, dither, gp.GAINS)
    parts = [gp.process(G, rc, part, fi, fo, shift=i % 4, out_shift=(i + 3) % 4) for i, part in enumerate(in_calls(x, cuts))]
    assert np.array_equal(np.concatenate(parts, axis=1), want[0]) and gp.same_levels(rc.levels(), levels[0])
    # the measuring kernels: through process, then through measure
    xs, _, _, _ = gt.case(pair, C)
    big = max(xs, key=lambda a: a.shape[1])
    cuts, made = short_cuts(pair, big.shape[1])
    q = tp.Composition(pair[0], pair[1], STREAMS, C, TPDF, gt.SEED, gt.FIRST, gt.GAINS)
    whole = q.process(big, S16, S24)
    rc = gt.converter(G, pair, STREAMS, C, TPDF, gt.GAINS)
    parts = [gp.process(G, rc, part, S16, S24, shift=(i + 1) % 4, out_shift=i % 4) for i, part in enumerate(in_calls(big, cuts))]
    assert [p.shape[1] for p in parts[:-1]] == made[:-1]
    assert np.array_equal(np.concatenate(parts, axis=1), whole) and gt.same(rc.true_peak(), q.records) and gt.same(rc.levels(), q.levels)
    rc.close()
    rc = gt.converter(G, pair, STREAMS, C, TPDF, gt.GAINS)
    assert [gt.measure(G, rc, part, S16, shift=i % 4) for i, part in enumerate(in_calls(big, cuts))] == made
    assert gt.same(rc.true_peak(), q.records) and not rc.levels().view(np.uint8).any()
    rc.close()


def test_create_refuses_a_converter_without_a_tile(G):
    aw = G.aw
    (in_rate, out_rate), C = geo.NO_TILE
    assert aw.rateconv_plan(in_rate, out_rate) == {"L": 1, "M": 640, "taps": 61440, "latency": 30720}          # the plan itself is accepted
    meter = aw.Spatializer(aw.HRIR(np.ones((2, 8), np.float32), 48000.0, ctx=G.ctx), [0, 1], [1, 0], 1, ctx=G.ctx)
    a0 = meter.info()["device_allocs"]
    for channels in (C, 16):
        name, message = refusal(G, lambda: aw.RateConverter(in_rate, out_rate, 2, channels, ctx=G.ctx))
        assert name == "INVALID_ARGUMENT" and "no tile" in message, (name, message)
    assert meter.info()["device_allocs"] == a0


def test_a_tile_of_seven_outputs_converts_and_refuses_to_measure(G):
    """40 outputs through tiles of 7: six workgroups per stream and call, each with an input image of 670 frames of 16 channels, nearly
    the whole LDS, in float32 and in s24 -> s24 with dither and per-stream gains; aw_tp_rateconv_set(on) in between is refused and leaves
    the handle as it was."""
    pair, C = geo.TINY_TILE
    L, M, T, D = emu.plan(*pair)
    n = emu.input_frames_for(40, L, M, D)
    rng = np.random.default_rng(7)
    # float32
    x, x7 = rng.standard_normal((STREAMS, n, C)).astype(np.float32), rng.standard_normal((STREAMS, 7, C)).astype(np.float32)
    q = emu.Converter(pair[0], pair[1], STREAMS, C, kernel=False)
    want = [q.process(x), q.process(x7), q.flush()]
    assert want[0].shape[1] == 40 and want[2].shape[1] > 40
    rc = G.aw.RateConverter(pair[0], pair[1], STREAMS, C, ctx=G.ctx)
    info = rc.info()
    assert info["tile"] == geo.BOUNDARY_TILES[geo.TINY_TILE] == 7 == emu.tile(pair[0], pair[1], C) and info["true_peak_tile"] == 0
    got = [f32.process(G, rc, x)]
    name, message = refusal(G, rc.set_true_peak, True)
    assert name == "INVALID_ARGUMENT" and "leaves none" in message and "tile of 7" in message, (name, message)
    assert rc.info()["true_peak"] == 0 and rc.info()["frames_produced"] == 40 and refusal(G, rc.true_peak)[0] == "INVALID_ARGUMENT"
    got += [f32.process(G, rc, x7, shift=1), f32.flush(G, rc)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert f32.same(g, w), (i, int((f32.bits(g) != f32.bits(w)).sum()))
    rc.close()
    # s24 -> s24, high-passed TPDF, per-stream gains
    fi, fo, dither, _ = gp.FORMS["s24-s24 tpdf_hp"]
    x, x7 = pcm.random_input(rng, (STREAMS, n, C), fi), pcm.random_input(rng, (STREAMS, 7, C), fi)
    q = pcm.Converter(pair[0], pair[1], STREAMS, C, False, dither, gp.SEED, gp.FIRST, gp.GAINS)
    rc = gp.converter(G, pair, STREAMS, C, dither, gp.GAINS)
    word = G.torch.zeros(1, dtype=G.torch.int64, device="cuda")
    assert np.array_equal(gp.process(G, rc, x, fi, fo, shift=1, out_shift=3, clipped_ptr=word.data_ptr()), q.process(x, fi, fo))
    assert gp.same_levels(rc.levels(), q.levels)
    assert refusal(G, rc.set_true_peak, True)[0] == "INVALID_ARGUMENT"
    assert np.array_equal(gp.process(G, rc, x7, fi, fo, shift=2, out_shift=1, clipped_ptr=word.data_ptr()), q.process(x7, fi, fo))
    assert np.array_equal(gp.flush(G, rc, fo, clipped_ptr=word.data_ptr()), q.flush(fo))
    assert gp.same_levels(rc.levels(), q.levels) and int(word.item()) == int(q.clipped[0]) == int(q.levels["clipped"].sum())
    assert int(q.levels["frames"][0]) == sum(w.shape[1] for w in want)
    rc.close()


def test_a_tile_of_twelve_outputs_measures_one_output_per_workgroup(G):
    """The smallest tile that leaves a measuring tile: every workgroup computes 11 predecessors again for the one output it owns."""
    pair, C = geo.SMALLEST_MEASURING
    L, M, T, _ = emu.plan(*pair)
    assert tp.tiles(L, M, T, C) == (12, 1)
    gt.check_process_and_measure(G, pair, C)
