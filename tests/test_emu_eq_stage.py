"""CPU thread emulation of the batch entries' equalizer stage (device/eq_cascade.hpp: eq_stage_stream / eq_stage_sequential, the code
hipcc compiles): one preset per stream through a map, the state [stream][kmax][4] with kmax above most presets' filter counts, both ear
forms.  Every equalized stream equals the emulated plain cascade of its own preset bit for bit, a stream mapped to -1 its input, and
every sample is within one float32 ulp of the oracle's sequential recurrence."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_eq_stage  # noqa: E402

ULP = 6e-8               # tests/test_gpu_eq.py: 2^-24
FS = 48000.0
A = (-2.56, [(1, 105.0, -2.8, 0.7), (0, 65.3, 1.0, 1.68), (0, 1000.0, 6.0, 0.707), (2, 10000.0, -5.2, 0.7), (0, 20.0, 3.0, 4.0)])      # test_gpu_eq.FILTERS
B = (-6.0, [(i % 3, 100.0 + 300.0 * i, ((i % 5) - 2) * 1.5, 0.5 + 0.1 * i) for i in range(64)])                                            # its 64-filter set
C = (6.0, [])                                                                                                                              # preamp only
PRESETS = [A, B, C]
MAP = [0, -1, 1, 0, 2]


def _oracle_state(oracle, preset):
    return oracle.eq_prepare(oracle.EqualizerDefinition(preset[0], [oracle.EqualizerFilter(1, None, True, t, f, g, q) for t, f, g, q in preset[1]]), FS)


@pytest.mark.parametrize("ear_split", [False, True])
@pytest.mark.parametrize("calls", [[31, 32, 33, 64], [8191, 8192, 8193]])
def test_every_stream_runs_its_own_preset(oracle, calls, ear_split):
    S = len(MAP)
    stage = emu_eq_stage.Stage(PRESETS, MAP, FS, ear_split=ear_split)
    assert stage.kmax == 64
    plain = [None if m < 0 else emu_eq_stage.Plain(PRESETS[m][0], PRESETS[m][1], 1, FS, ear_split=ear_split) for m in MAP]      # one stream each
    truth = [None if m < 0 else _oracle_state(oracle, PRESETS[m]) for m in MAP]
    rng = np.random.default_rng(sum(calls))
    for n in calls:
        x = rng.uniform(-0.5, 0.5, (S, n, 2)).astype(np.float32)
        y = stage.process(x)
        for s, m in enumerate(MAP):
            if m < 0:
                assert np.array_equal(y[s], x[s]), (n, s)
                continue
            assert np.array_equal(y[s], plain[s].process(x[s:s + 1])[0]), (n, s, m)
            el, er = truth[s].process(x[s, :, 0], x[s, :, 1])
            err = max(np.max(np.abs(y[s, :, 0] - el)), np.max(np.abs(y[s, :, 1] - er)))
            print(f"call {n} stream {s} preset {m}: max |y - oracle| = {err:.3e}, peak {np.max(np.abs(y[s])):.3f}")
            assert err <= ULP, (n, s, m, err)
    # the state a stream leaves is its preset's, in the first rows of its kmax: the rest was never written
    for s, m in enumerate(MAP):
        k = 0 if m < 0 else len(PRESETS[m][1])
        assert not stage.z[s, k:].any(), s
        if m >= 0:
            assert np.array_equal(stage.z[s, :k], plain[s].z[0, :k]), s
