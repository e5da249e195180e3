"""HRIRs beyond 40 961 taps on the GPU.  The marched CMAC (device/march_kernels.hip) takes the partitions eight at a time: 12 | 13 partitions is
the first later pass of more than four (aw_part_march_kernel<8, LG, true>), 16 | 17 the first third pass, 69 633 taps run 8 + 8 + 2; the block-group
CMAC, the forward and the inverse kernels see the same partition counts.  The long-window kernels run histories of 16 and 24 partitions on 32 rows
(24: the hop is exactly a quarter of the window, the last lw_choose admits; one tap more and the call stays on the partitioned kernels) and of 32
partitions on 128 rows, with host- and device-built tables.  Last, an equalizer folded into a bundled HRIR that comes out at 57 348 taps, through
MixedRateBatch.

End-heavy HRIRs (spectral_ref.py): the last taps carry the energy, a dropped tap or partition is a gross error.  Two streams, float64 truth at
test_gpu_parity's tolerance per stream and ear; two calls against one at 3e-6 of peak.  One context per knob set (test_gpu_launch_tables.py)."""
import os

import numpy as np
import pytest

import spectral_cases as sc
from spectral_ref import TOL

pytestmark = pytest.mark.gpu
S = 2
SPLIT_TOL = 3e-6            # two calls against one (test_gpu_spectral.py::test_end_heavy_hrirs)
TABLES_TOL = 2e-6           # host-built against device-built tables (test_gpu_longwin.py::test_device_built_tables_match_the_host_builder)

PART_ENV = {"march": {"AW_WINDOW": "4096", "AW_LW": "0"}, "group": {"AW_WINDOW": "4096", "AW_LW": "0", "AW_PART_CMAC": "group"}}
CMAC_STAGE = {"march": "aw_part_march_kernel", "group": "aw_part_cmac_kernel"}
PART_CASES = [(taps, c) for taps in (49152, 49153, 65536, 65537, 69633) for c in (2, 7)] + [(65537, 14)]

_contexts, _truth = {}, {}


def _case(oracle, channels, taps, frames):
    """End-heavy HRIR, maps, input and float64 truth: computed once, kept unchanged, shared by the knob sets that run the case."""
    key = (channels, taps, frames)
    if key not in _truth:
        h, lt, rt, x = sc.end_heavy_input(oracle, channels, taps, S, frames)
        ref = [oracle.spatialize_f64(x[s], h, lt, rt) for s in range(S)]
        for a in (h, lt, rt, x, *ref):
            a.setflags(write=False)
        _truth[key] = (h, lt, rt, x, ref)
    return _truth[key]


def _spatializer(monkeypatch, env, h, lt, rt):
    import airwave_amd as aw
    for k in ("AW_WINDOW", "AW_LW", "AW_PART_CMAC", "AW_LW_TABLES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    key = tuple(sorted(env.items()))
    if key not in _contexts:
        _contexts[key] = aw.Context(0)
    ctx = _contexts[key]
    return aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)


def _worst(oracle, y, ref, label):
    worst = 0.0
    for s in range(S):
        assert not np.isnan(y[s]).any(), (label, s)
        for ear in range(2):
            worst = max(worst, oracle.peak_rel_error(y[s, :, ear], ref[s][:, ear]))
    print(f"FIGURE long-hrir {label}: peak_rel_error {worst:.2e}")
    return worst


@pytest.mark.parametrize("cmac", ["march", "group"])
@pytest.mark.parametrize("taps,channels", PART_CASES, ids=[f"{t}taps-{c}ch" for t, c in PART_CASES])
def test_partitioned_path_on_either_side_of_every_pass(oracle, monkeypatch, taps, channels, cmac):
    P = -(-taps // 4096)
    history = P * 4096
    frames = history + 10001                    # head windows, interior windows, a ragged tail, and room for a second call behind the history
    h, lt, rt, x, ref = _case(oracle, channels, taps, frames)
    sp = _spatializer(monkeypatch, PART_ENV[cmac], h, lt, rt)
    sp.set_profiling(True)
    y = sp.process(x)
    info = sp.info()
    assert (info["path"], info["partitions"], info["history"], info["long_window_rows"]) == (1, P, history, 0), info
    stages = [n for n, _, _ in sp.stage_times()]
    assert CMAC_STAGE[cmac] in stages and CMAC_STAGE["group" if cmac == "march" else "march"] not in stages, stages
    sp.set_profiling(False)
    assert _worst(oracle, y, ref, f"partitioned-{cmac} {channels}ch {taps} taps P={P}") < TOL
    # the same timeline as two calls, split one frame behind the history
    sp.reset()
    cut = history + 1
    two = np.concatenate([sp.process(np.ascontiguousarray(x[:, lo:hi])) for lo, hi in ((0, cut), (cut, frames))], axis=1)
    diff = float(np.max(np.abs(two - y)) / np.max(np.abs(y)))
    print(f"FIGURE long-hrir split partitioned-{cmac} {channels}ch {taps} taps: two calls against one {diff:.2e} of peak")
    assert diff <= SPLIT_TOL
    assert _worst(oracle, two, ref, f"partitioned-{cmac} {channels}ch {taps} taps, two calls") < TOL


def _lw_frames(rows, taps):
    history = -(-taps // 4096) * 4096
    return max(rows * 4096 - history, history) + 20000          # at least two windows, and more than the history


LW_CASES = [(32, 65536), (32, 98304), (128, 131072)]


@pytest.mark.parametrize("channels", [2, 7])
@pytest.mark.parametrize("rows,taps", LW_CASES, ids=[f"lw{r}-{t}taps" for r, t in LW_CASES])
def test_long_window_kernels_on_long_histories(oracle, monkeypatch, rows, taps, channels):
    """Histories of 16 and 24 partitions on 32 rows (24: hop = N / 4 exactly) and of 32 partitions on 128 rows, device-built tables."""
    history = -(-taps // 4096) * 4096
    assert rows * 4096 - history >= rows * 4096 // 4
    frames = _lw_frames(rows, taps)
    h, lt, rt, x, ref = _case(oracle, channels, taps, frames)
    sp = _spatializer(monkeypatch, {"AW_LW": str(rows)}, h, lt, rt)
    y = sp.process(x)
    info = sp.info()
    assert (info["path"], info["history"], info["long_window_rows"], info["long_window_rows_rest"]) == (1, history, rows, 0), info
    assert _worst(oracle, y, ref, f"lw{rows} {channels}ch {taps} taps history {history // 4096} partitions") < TOL


@pytest.mark.parametrize("channels", [2, 7])
def test_a_history_past_three_quarters_of_the_window_stays_on_the_partitioned_kernels(oracle, monkeypatch, channels):
    """98 305 taps: 25 partitions of history leave a 32-row window a hop below N / 4, lw_choose refuses it although AW_LW forces 32 rows; the
    call runs the partitioned kernels (four passes of the marched CMAC)."""
    taps = 98305
    frames = 25 * 4096 + 20000
    h, lt, rt, x, ref = _case(oracle, channels, taps, frames)
    sp = _spatializer(monkeypatch, {"AW_LW": "32"}, h, lt, rt)
    y = sp.process(x)
    info = sp.info()
    assert (info["path"], info["partitions"], info["history"], info["long_window_rows"]) == (1, 25, 25 * 4096, 0), info
    assert _worst(oracle, y, ref, f"lw32 refused, partitioned {channels}ch {taps} taps") < TOL


def test_long_history_tables_built_on_the_host_and_on_the_device(oracle, monkeypatch):
    """J = ceil(taps / 4096) = 16 in the prep kernels' loop (device/prep_kernels.hip) and in the host builder: same samples to the tables' float32
    rounding."""
    rows, taps, channels = 32, 65536, 7
    h, lt, rt, x, ref = _case(oracle, channels, taps, _lw_frames(rows, taps))
    ys = {}
    for mode in ("host", "gpu"):
        sp = _spatializer(monkeypatch, {"AW_LW": str(rows), "AW_LW_TABLES": mode}, h, lt, rt)
        ys[mode] = sp.process(x)
        assert sp.info()["long_window_rows"] == rows, sp.info()
        assert _worst(oracle, ys[mode], ref, f"lw{rows} {channels}ch {taps} taps, {mode}-built tables") < TOL
    diff = float(np.max(np.abs(ys["gpu"] - ys["host"])) / max(np.max(np.abs(r)) for r in ref))
    print(f"FIGURE long-hrir tables lw{rows} {channels}ch {taps} taps: device-built against host-built {diff:.2e} of peak")
    assert diff <= TABLES_TOL


def test_the_policy_on_its_own_at_65536_taps(oracle, monkeypatch):
    """No AW_LW: whichever kernels lw_choose picks for this call, parity holds."""
    taps, channels = 65536, 7
    h, lt, rt, x, ref = _case(oracle, channels, taps, _lw_frames(32, taps))
    sp = _spatializer(monkeypatch, {}, h, lt, rt)
    y = sp.process(x)
    info = sp.info()
    print(f"FIGURE long-hrir policy {channels}ch {taps} taps {x.shape[1]} frames: info {info}")
    assert (info["path"], info["partitions"], info["history"]) == (1, 16, 65536), info
    assert _worst(oracle, y, ref, f"policy {channels}ch {taps} taps (long_window_rows {info['long_window_rows']})") < TOL


def test_an_equalizer_folded_into_a_57348_tap_hrir(oracle, golden_dir):
    """A +6 dB bell at 20 Hz, Q 3, rings for 53 029 frames at 48 kHz (1e-7 of its peak): folded into StageSH1.0 (4320 taps) the batch host runs a
    57 348-tap HRIR, 15 partitions of history.  Against the two-effect order of test_gpu_eq_fold.py, at its tolerance; two calls."""
    import airwave_amd as aw
    from test_gpu_eq_fold import SPEAKERS7, TOL as FOLD_TOL, _reference
    from test_eq_fold_host import LONG_FOLD
    rate = 48000.0
    d = aw.EqualizerDefinition(LONG_FOLD[0], [aw.EqualizerFilter(1, 1, True, *LONG_FOLD[1])])
    od = oracle.EqualizerDefinition(LONG_FOLD[0], [oracle.EqualizerFilter(1, 1, True, *LONG_FOLD[1])])
    w = oracle.wav_load(os.path.join(golden_dir, "hrtf", "StageSH1.0.wav"))
    tracks, lt, rt = oracle.assemble_tracks(w, SPEAKERS7, target_rate=rate)
    batch = aw.MixedRateBatch(np.asarray(w.audio_data), 48000.0, aw.InputLayout(SPEAKERS7, "7 speakers"), [rate] * S, equalizer=d, fold_equalizer=True)
    b = batch.buckets[rate]
    assert b.equalizer is None and b.eq_tail_bound <= 1e-7 and b.hrir_taps == tracks.shape[1] + b.eq_response_taps - 1
    assert 49153 <= b.hrir_taps <= 65536, b.hrir_taps
    x = oracle.synth_input(S, 75000, 7, seed=48)
    cut = 15 * 4096 + 1
    y1 = b.spatializer.process(x[:, :cut])
    info = b.spatializer.info()
    assert (info["path"], info["partitions"], info["history"]) == (1, 15, 15 * 4096), info
    y = np.concatenate([y1, b.spatializer.process(x[:, cut:])], axis=1)
    worst = max(oracle.peak_rel_error(y[s], _reference(oracle, od, rate, x[s], tracks, lt, rt)) for s in range(S))
    print(f"FIGURE long-hrir fold {b.hrir_taps} taps, long_window_rows {info['long_window_rows']}: peak_rel_error {worst:.2e}")
    assert worst < FOLD_TOL
