"""The batch entries launch what they launched when tests/golden/batch_launch_sequences.json was recorded (tools/batch_launches.py on an
MI355X, before the entries were given one call plan and one chunk step): for every (entry, sample formats, meter / gain state, dither,
shape) the (stage name, launches) list of stage_times() after one profiled call is the recorded one.  A case that either side lacks is a
failure.  The bytes, clip counts and records of these paths are held to numpy by test_gpu_pcm.py, test_gpu_pcm_dither.py and
test_gpu_levels.py."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("process", "process_host", "process_pcm", "process_host_pcm", "process_planar")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("_batch_launches_under_test", os.path.join(ROOT, "tools", "batch_launches.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def recorded(tool, golden_dir):
    return tool.loads(open(os.path.join(golden_dir, "batch_launch_sequences.json")).read())


def test_the_record_covers_every_case_axis(tool, recorded):
    assert set(recorded) == {tool.key(c) for c in tool.cases(later=True)}
    entry, fin, fout, state, dither, shape = (set(v) for v in zip(*recorded))
    assert entry == set(ENTRIES)
    assert {(a, b) for (_, a, b, _, _, _) in recorded} == {("f32", "f32"), ("s16", "f32"), ("f32", "s16"), ("s24", "s24"), ("f32", "s32")}
    assert state == {"off", "meter", "gain", "ceiling", "loudness", "true_peak", "true_peak_ceiling", "limiter"} and dither == {"none", "tpdf"}
    assert shape == {"one_piece", "chunked", "single", "planar", "planar_staged"}
    for e in ("process_pcm", "process_host_pcm"):           # the PCM entries: every format pair, state and dither on both kinds of path
        for sh in ("one_piece", "chunked"):                 # (the four later stages' states: without dither only)
            assert len([k for k in recorded if k[0] == e and k[5] == sh]) == 5 * 4 * 2 + 5 * 4, (e, sh)
            assert len([k for k in recorded if k[0] == e and k[5] == sh and k[3] in ("off", "meter", "gain", "ceiling")]) == 5 * 4 * 2, (e, sh)
    assert all(seq for seq in recorded.values())             # every call launched something


@pytest.mark.parametrize("entry", ENTRIES)
def test_launch_lists_are_the_recorded_ones(tool, recorded, entry):
    want = {k: v for k, v in recorded.items() if k[0] == entry}
    got = {tool.key(r): r["launches"] for r in tool.run_all(entry=entry, later=True)}
    assert set(got) == set(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    different = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not different, different
