"""Every row of every launch table (airwave_amd/csrc/device/launch_table.hpp) runs at least once: a kernel whose row is missing, or that
needs dynamic LDS and never got the attribute, fails its launch here.  Channel counts 1..16 through Spatializer.process, 2 streams of
20 000 frames (interior, boundary and ragged-tail tiles at every hop up to 8192), on each kernel path the environment can force, each
against the float64 oracle at test_gpu_parity's tolerance.  The knobs are read when a context / a spatializer is created.

Rows that other tests already run and that are not repeated here:
  - overlap-add tile, H = 7, all twelve layouts: test_gpu_ola.py::test_every_layout_of_the_overlap_add_tile_matches_truth_and_port
  - the marched CMAC and the EQ kernels have no table.
The split kernels have one table per window length (11 lengths x 16 rows: 1-8 channels narrow, 9-16 wide), so every window length runs
every layout; the merge table's rows (one per window length) run with them."""
import numpy as np
import pytest

from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
S, F = 2, 20000
ALL = list(range(1, 17))
OLA_LAYOUTS = [4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]           # ola_inst.hpp
FWD_LAYOUTS = [2, 3, 4, 5, 6, 7, 8, 12, 14, 16]                     # kernels.hip AW_FOR_EACH_VEC: forward kernels with compile-time channels

_truth, _contexts = {}, {}


def _case(oracle, channels, taps):
    """Input, HRIR, maps and the float64 truth of one (layout, HRIR length): computed once, shared by every knob set."""
    key = (channels, taps)
    if key not in _truth:
        h = oracle.synth_hrir(14, taps, seed=taps)
        lt = (np.arange(channels) % 14).astype(np.int32)
        rt = ((np.arange(channels) * 3 + 7) % 14).astype(np.int32)
        x = oracle.synth_input(S, F, channels, seed=channels)
        ref = [oracle.spatialize_f64(x[s], h, lt, rt) for s in range(S)]
        for a in (h, lt, rt, x, *ref):
            a.setflags(write=False)
        _truth[key] = (h, lt, rt, x, ref)
    return _truth[key]


def _run(oracle, monkeypatch, channels, taps, env):
    """A spatializer created under `env` on a context created under `env` (one context per knob set); returns its info after the call."""
    import airwave_amd as aw
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    key = tuple(sorted(env.items()))
    if key not in _contexts:
        _contexts[key] = aw.Context(0)
    ctx = _contexts[key]
    h, lt, rt, x, ref = _case(oracle, channels, taps)
    sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    y = sp.process(x)
    for s in range(S):
        assert oracle.peak_rel_error(y[s], ref[s]) < TOL, (channels, taps, env, s)
    return sp.info()


@pytest.mark.parametrize("channels", ALL)
def test_default_path(oracle, monkeypatch, channels):
    """8192-frame windows: vector interior kernels of 2-8 channels, one-pass wide kernels of 9-14, two passes for 15 / 16; boundary
    kernels <2 | 4 | 8, NP, false>, generic 1-4 pairs, and for 9-16 channels the 4-pair pass plus the accumulating 1-4-pair pass."""
    info = _run(oracle, monkeypatch, channels, 4320, {})
    assert info["path"] == 0 and info["fft"] == 8192 and info["overlap_add_rows"] == 0 and info["long_window_rows"] == 0


@pytest.mark.parametrize("two_pass", ["0", "1"])
@pytest.mark.parametrize("channels", [10, 11, 12, 13, 14, 15, 16])
def test_wide_layouts_two_pass_forms(oracle, monkeypatch, channels, two_pass):
    """AW_WIDE_TWO_PASS=1: the first / second pass kernels of 10, 12, 14, 15, 16 channels; =0: the run-time-loop kernels <12 | 14 | 16, 0, true>
    and <0, 0, false>, 10 channels still two passes, odd layouts all generic."""
    info = _run(oracle, monkeypatch, channels, 4320, {"AW_WIDE_TWO_PASS": two_pass})
    assert info["path"] == 0 and info["fft"] == 8192


@pytest.mark.parametrize("channels", ALL)
def test_16384_frame_windows(oracle, monkeypatch, channels):
    """Interior and boundary kernels of 1-8 channels (4, 6, 8 in their own unit), <0, 0, false> for everything of the wider layouts."""
    info = _run(oracle, monkeypatch, channels, 4320, {"AW_WINDOW": "16384", "AW_LW": "0"})
    assert info["path"] == 0 and info["fft"] == 16384 and info["long_window_rows"] == 0


@pytest.mark.parametrize("form", ["1", "2"])
@pytest.mark.parametrize("channels", [1, 9] + FWD_LAYOUTS)
def test_partitioned_forward_kernels(oracle, monkeypatch, channels, form):
    """6000 taps on 4096-frame partitions: six windows per stream, two head, three interior, one past the end; mono and 9 channels run
    everything through the generic kernel.  AW_PART_FWD=1: one pair per workgroup, 2: persistent workgroups."""
    info = _run(oracle, monkeypatch, channels, 6000, {"AW_WINDOW": "4096", "AW_PART_FWD": form, "AW_LW": "0"})
    assert info["path"] == 1 and info["partitions"] == 2 and info["long_window_rows"] == 0


@pytest.mark.parametrize("taps,rows", [(3969, 8), (5000, 6)])
@pytest.mark.parametrize("channels", OLA_LAYOUTS)
def test_overlap_add_tile_rows(oracle, monkeypatch, channels, taps, rows):
    info = _run(oracle, monkeypatch, channels, taps, {"AW_OLA": "1", "AW_OLA_MIN_BLOCKS": "0"})
    assert info["overlap_add_rows"] == rows


# (rows of the window, knobs of the rows kernel): the 16-point form, the 8-point form with one pair per batch (every pair count), and with
# two (up to four pairs; more take the one-pair form again).  Pair counts 1-8 x {even, odd channel count} are the rows tables' keys; the
# split tables of 32, 40 and 128 rows are run whole, narrow (1-8 channels) and wide (9-16).
@pytest.mark.parametrize("rows,knobs", [(32, {"AW_LW_ROWS_FORM": "16"}), (40, {"AW_LW_ROWS_FORM": "8", "AW_LW_ROWS_PB": "1"}),
                                        (128, {"AW_LW_ROWS_FORM": "8", "AW_LW_ROWS_PB": "2"})])
@pytest.mark.parametrize("channels", ALL)
def test_long_window_kernels(oracle, monkeypatch, channels, rows, knobs):
    info = _run(oracle, monkeypatch, channels, 4320, {"AW_LW": str(rows), **knobs})
    assert info["long_window_rows"] == rows


@pytest.mark.parametrize("rows", [48, 56, 64, 72, 80, 96, 112, 120])
@pytest.mark.parametrize("channels", ALL)
def test_split_kernels_of_the_other_window_lengths(oracle, monkeypatch, channels, rows):
    """The (channels, wide) rows of the remaining eight split tables, and with them the remaining rows of the merge table."""
    info = _run(oracle, monkeypatch, channels, 4320, {"AW_LW": str(rows)})
    assert info["long_window_rows"] == rows
