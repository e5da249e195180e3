"""CPU thread emulation of a target change of the equalizer stage (device/eq_cascade.hpp: eq_stage_fade_stream / eq_stage_fade_sequential,
the code hipcc compiles; the cuts: host/eq_fade_plan.hpp) against the oracle's ParametricEqualizerProcessor, one per stream, fed the same
input in pieces of at most 4096 frames and drained after each.

Bounds, with ULP = 6e-8 as in tests/test_gpu_eq_stage.py: each rendering is within ULP of the oracle's; on the frames of a fade the output
is a convex mix of two such values (within ULP) rounded to float32 once more (another ULP at |y| < 1): 2 ULP there, ULP elsewhere.  The
input level 0.15 keeps |y| < 1 for every preset used.  A stream that never takes part (KEEP) equals the emulated plain stage fed the
call's pieces as calls, bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_eq_fade  # noqa: E402
import emu_eq_stage  # noqa: E402

ULP = 6e-8
LEVEL = 0.15
A = (-2.56, [(1, 105.0, -2.8, 0.7), (0, 65.3, 1.0, 1.68), (0, 1000.0, 6.0, 0.707), (2, 10000.0, -5.2, 0.7), (0, 20.0, 3.0, 4.0)])      # test_gpu_eq.FILTERS
B = (-6.0, [(i % 3, 100.0 + 300.0 * i, ((i % 5) - 2) * 1.5, 0.5 + 0.1 * i) for i in range(64)])                                            # its 64-filter set
C = (6.0, [])                                                                                                                              # preamp only
PRESETS = [A, B, C]
KEEP = -2


def _definition(oracle, entry):
    if entry < 0:
        return None
    preamp, filters = PRESETS[entry]
    return oracle.EqualizerDefinition(preamp, [oracle.EqualizerFilter(1, None, True, t, f, g, q) for t, f, g, q in filters])


def _run(oracle, rate, calls, publications, installed, ear_split=False):
    """publications: {call index: [entry per stream]}, made before that call; installed: the map before the first call.  A stream is a
    KEEP stream when no publication names it; the others start at -1, as the oracle's processor does."""
    S = len(installed)
    assert emu_eq_fade.keep() == KEEP
    T = emu_eq_fade.fade_length(rate)
    assert T == max(1, int(np.floor(rate * 0.020 + 0.5)))
    stage = emu_eq_fade.FadeStage(PRESETS, installed, rate, ear_split=ear_split)
    keeps = [s for s in range(S) if all(p[s] == KEEP for p in publications.values())]
    assert all(installed[s] == -1 for s in range(S) if s not in keeps)
    plain = {s: emu_eq_stage.Stage(PRESETS, [installed[s]], rate, ear_split=ear_split) for s in keeps}
    procs = {s: oracle.ParametricEqualizerProcessor(rate) for s in range(S) if s not in keeps}
    rng = np.random.default_rng(int(rate) + sum(calls))
    all_segs = []
    for i, n in enumerate(calls):
        if i in publications:
            stage.set_target(publications[i])
            for s, proc in procs.items():
                if publications[i][s] != KEEP:
                    proc.set_target(_definition(oracle, publications[i][s]))
        x = rng.uniform(-LEVEL, LEVEL, (S, n, 2)).astype(np.float32)
        y, segs = stage.process(x)
        all_segs.append(segs)
        fading = np.zeros(n, bool)
        for first, count, t0, fade, begins, ends in segs:
            if fade:
                fading[first:first + count] = True
        for s in keeps:
            want = np.concatenate([plain[s].process(x[s:s + 1, first:first + count])[0] for first, count, *_ in segs])
            assert np.array_equal(y[s], want), (i, s)
        for s, proc in procs.items():
            ref = np.empty((n, 2), np.float32)
            for at in range(0, n, 4096):
                ref[at:at + 4096, 0], ref[at:at + 4096, 1] = proc.process(x[s, at:at + 4096, 0], x[s, at:at + 4096, 1])
                proc.drain_retired_states()
            err = np.max(np.abs(y[s].astype(np.float64) - ref), axis=1)
            e_fade, e_rest = (err[fading].max() if fading.any() else 0.0), (err[~fading].max() if (~fading).any() else 0.0)
            print(f"rate {rate} call {i} ({n}) stream {s}: fade frames {int(fading.sum())} err {e_fade:.3e}, other frames err {e_rest:.3e}, peak {np.max(np.abs(y[s])):.3f}")
            assert np.max(np.abs(y[s])) < 1.0
            assert e_fade <= 2 * ULP and e_rest <= ULP, (i, s, e_fade, e_rest)
    return stage, all_segs, T


ALL = [0, 1, 2, KEEP]          # streams 0 - 2 fade to A, B, C; stream 3 keeps the preset it was installed with
INSTALLED = [-1, -1, -1, 0]


@pytest.mark.parametrize("ear_split", [False, True])
def test_48000_no_tail(oracle, ear_split):
    stage, segs, T = _run(oracle, 48000.0, [2000], {0: ALL}, INSTALLED, ear_split)
    assert T == 960 and T % 32 == 0
    assert segs == [[(0, 960, 0, 1, 1, 1), (960, 1040, 0, 0, 0, 0)]]
    assert list(stage.map) == [0, 1, 2, 0] and stage.clock[1:] == [0, 0, 0]


@pytest.mark.parametrize("ear_split", [False, True])
def test_44100_body_and_tail(oracle, ear_split):
    stage, segs, T = _run(oracle, 44100.0, [3000], {0: ALL}, INSTALLED, ear_split)
    assert T == 882 == 27 * 32 + 18
    assert segs[0][0] == (0, 882, 0, 1, 1, 1)


def test_441000_crosses_the_span_carry(oracle):
    stage, segs, T = _run(oracle, 441000.0, [12000], {0: ALL}, INSTALLED)
    assert T == 8820 == 8192 + 19 * 32 + 20
    assert segs[0] == [(0, 8820, 0, 1, 1, 1), (8820, 3180, 0, 0, 0, 0)]


@pytest.mark.parametrize("rate,cuts", [
    (48000.0, [[(0, 500, 0, 1, 1, 0)], [(0, 460, 500, 1, 0, 1), (460, 40, 0, 0, 0, 0)], [(0, 3000, 0, 0, 0, 0)]]),
    (96000.0, [[(0, 500, 0, 1, 1, 0)], [(0, 500, 500, 1, 0, 0)], [(0, 920, 1000, 1, 0, 1), (920, 2080, 0, 0, 0, 0)]]),      # T = 1920: ends inside the third
])
def test_a_fade_over_several_calls(oracle, rate, cuts):
    stage, segs, T = _run(oracle, rate, [500, 500, 3000], {0: ALL}, INSTALLED)
    assert segs == cuts


def test_calls_shorter_than_a_chunk(oracle):
    stage, segs, T = _run(oracle, 48000.0, [7, 31, 2000], {0: ALL}, INSTALLED)
    assert segs == [[(0, 7, 0, 1, 1, 0)], [(0, 31, 7, 1, 0, 0)], [(0, 922, 38, 1, 0, 1), (922, 1078, 0, 0, 0, 0)]]


def test_a_second_target_begins_where_the_first_fade_ends(oracle):
    # published after the first call, while the fade runs: it begins at frame 460 of the second call, in its middle
    stage, segs, T = _run(oracle, 48000.0, [500, 3000], {0: ALL, 1: [1, 2, 0, KEEP]}, INSTALLED, ear_split=True)
    assert segs[1] == [(0, 460, 500, 1, 0, 1), (460, 960, 0, 1, 1, 1), (1420, 1580, 0, 0, 0, 0)]
    assert list(stage.map) == [1, 2, 0, 0]


def test_the_newest_publication_wins_per_stream(oracle):
    # two publications before the fade they wait for has ended: the later entry replaces the earlier one, KEEP leaves it
    S = 4
    stage = emu_eq_fade.FadeStage(PRESETS, INSTALLED, 48000.0)
    stage.set_target(ALL)
    x = np.zeros((S, 100, 2), np.float32)
    stage.process(x)
    stage.set_target([1, KEEP, KEEP, KEEP])
    stage.set_target([KEEP, 2, KEEP, KEEP])
    assert list(stage.pending_map) == [1, 2, KEEP, KEEP] and stage.clock == [960, 100, 1, 1]
    stage.process(np.zeros((S, 2000, 2), np.float32))
    assert list(stage.map) == [1, 2, 2, 0] and stage.clock == [960, 0, 0, 0]


def test_unity_to_a_preset_and_back(oracle):
    stage, segs, T = _run(oracle, 48000.0, [1500, 1500, 700], {0: ALL, 1: [-1, -1, -1, KEEP]}, INSTALLED)
    assert list(stage.map) == [-1, -1, -1, 0]
    assert segs[1] == [(0, 960, 0, 1, 1, 1), (960, 540, 0, 0, 0, 0)]
    # from the fade's end on a stream faded to -1 keeps its samples
    x = np.random.default_rng(5).uniform(-LEVEL, LEVEL, (4, 64, 2)).astype(np.float32)
    y, _ = stage.process(x)
    assert np.array_equal(y[:3], x[:3])
