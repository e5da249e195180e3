"""Layouts of more than 16 input channels on the GPU.  aw_spatializer_create takes any channel count; past 16 the library has no vector kernel, no
overlap-add tile and no long-window kernels, and everything runs on the run-time-loop kernels: aw_fused_ols_kernel<0, 0, false> and
aw_fused_ols2_kernel<0, 0, false> (C pseudo-pairs) for every tile, the generic forward kernel in its one-pair form plus the block-group CMAC on the
partitioned path (the marched kernel's lane groups hold eight pairs).  17, 18, 24 and 32 channels on a 14-track HRIR (every map repeats tracks), one
layout with an unmapped speaker; knobs that ask for a kernel these layouts lack (AW_OLA=1, AW_LW=32) must fall back, not fail.

Two streams of 20 000 frames against the float64 truth at test_gpu_parity's tolerance; one context per knob set (test_gpu_launch_tables.py)."""
import numpy as np
import pytest

import spectral_ref as sr
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
S, F = 2, 20000
SPLIT_TOL = 3e-6            # any split of the timeline into calls (test_gpu_spectral.py, test_gpu_longwin.py)
WIDE = [17, 18, 24, 32, "18u"]              # "18u": 18 channels, speaker 5 unmapped (skipped: HRIRManager.swift:370-372)

_truth, _contexts = {}, {}


def _maps(layout):
    channels = int(str(layout).rstrip("u"))
    lt, rt = sr.maps(channels)
    if str(layout).endswith("u"):
        lt[5] = -1
    return channels, lt, rt


def _case(oracle, layout, taps, frames=F):
    key = (layout, taps, frames)
    if key not in _truth:
        channels, lt, rt = _maps(layout)
        h = oracle.synth_hrir(14, taps, seed=taps)
        x = oracle.synth_input(S, frames, channels, seed=channels)
        ref = [oracle.spatialize_f64(x[s], h, lt, rt) for s in range(S)]
        for a in (h, lt, rt, x, *ref):
            a.setflags(write=False)
        _truth[key] = (h, lt, rt, x, ref)
    return _truth[key]


def _context(monkeypatch, env):
    import airwave_amd as aw
    for k in ("AW_WINDOW", "AW_LW", "AW_OLA", "AW_OLA_MIN_BLOCKS", "AW_PART_CMAC", "AW_PART_FWD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    key = tuple(sorted(env.items()))
    if key not in _contexts:
        _contexts[key] = aw.Context(0)
    return _contexts[key]


def _run(oracle, monkeypatch, layout, taps, env, label):
    import airwave_amd as aw
    ctx = _context(monkeypatch, env)
    h, lt, rt, x, ref = _case(oracle, layout, taps)
    sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)        # (a HIP error or a refusal raises here or in process)
    sp.set_profiling(True)
    y = sp.process(x)
    assert np.isfinite(y).all(), (layout, taps, env)
    worst = max(oracle.peak_rel_error(y[s, :, ear], ref[s][:, ear]) for s in range(S) for ear in range(2))
    print(f"FIGURE wide {label} {layout}ch {taps} taps: peak_rel_error {worst:.2e}; kernel {sp.kernel_time()[2]!r}; stages {[n for n, _, _ in sp.stage_times()]}")
    assert worst < TOL, (layout, taps, env, worst)
    return sp.info(), [n for n, _, _ in sp.stage_times()]


@pytest.mark.parametrize("layout", WIDE)
def test_default_path(oracle, monkeypatch, layout):
    """4320 taps, no knob: the 8192-frame tile, every tile through the run-time-loop kernel."""
    info, _ = _run(oracle, monkeypatch, layout, 4320, {}, "default")
    assert (info["path"], info["fft"], info["hop"], info["history"]) == (0, 8192, 3840, 4352), info
    assert info["overlap_add_rows"] == 0 and info["overlap_add_rows_policy"] == 0 and info["long_window_rows"] == 0, info


@pytest.mark.parametrize("layout", WIDE)
def test_16384_frame_windows(oracle, monkeypatch, layout):
    """AW_WINDOW=16384: C pseudo-pairs (17 - 32) through aw_fused_ols2_kernel<0, 0, false>."""
    info, _ = _run(oracle, monkeypatch, layout, 4320, {"AW_WINDOW": "16384"}, "16384")
    assert (info["path"], info["fft"], info["hop"], info["history"]) == (0, 16384, 12032, 4352) and info["long_window_rows"] == 0, info


@pytest.mark.parametrize("taps", [6000, 9000])
@pytest.mark.parametrize("layout", WIDE)
def test_partitioned_path(oracle, monkeypatch, layout, taps):
    """From 16 channels and 6000 taps on the policy itself takes the partitioned path: 2 and 3 partitions, more than eight pairs, so the generic forward
    kernel in its one-pair form and the block-group CMAC."""
    info, stages = _run(oracle, monkeypatch, layout, taps, {}, "partitioned")
    P = -(-taps // 4096)
    assert (info["path"], info["partitions"], info["history"], info["long_window_rows"]) == (1, P, P * 4096, 0), info
    assert "aw_part_cmac_kernel" in stages and "aw_part_march_kernel" not in stages and "aw_part_forward1_kernel<generic>" in stages, stages


@pytest.mark.parametrize("form", ["1", "2"])
@pytest.mark.parametrize("layout", [17, 24])
def test_partitioned_forward_forms(oracle, monkeypatch, layout, form):
    """AW_PART_FWD: one pair per workgroup (the default for more than four pairs) and persistent workgroups that walk all 9 / 12 pairs."""
    info, stages = _run(oracle, monkeypatch, layout, 6000, {"AW_WINDOW": "4096", "AW_PART_FWD": form}, f"partitioned-fwd{form}")
    assert (info["path"], info["partitions"]) == (1, 2), info
    assert ("aw_part_forward1_kernel<generic>" if form == "1" else "aw_part_forward_kernel<generic>") in stages, stages


@pytest.mark.parametrize("env", [{"AW_OLA": "1", "AW_OLA_MIN_BLOCKS": "0"}, {"AW_LW": "32"}, {"AW_LW": "32", "AW_WINDOW": "4096"}],
                         ids=["ola", "lw32", "lw32-partitioned"])
@pytest.mark.parametrize("layout", [17, 24, 32])
def test_knobs_for_kernels_these_layouts_lack_fall_back(oracle, monkeypatch, layout, env):
    """There is no overlap-add tile and no long-window kernel for more than 16 channels: the knobs that force them are ignored, the call runs the
    path's own kernels and the result is within tolerance (asserted in _run, with finiteness), whatever info() reports — and it reports neither."""
    info, _ = _run(oracle, monkeypatch, layout, 4320, env, "fallback-" + "-".join(f"{k}={v}" for k, v in sorted(env.items())))
    assert info["overlap_add_rows"] == 0 and info["overlap_add_rows_policy"] == 0 and info["long_window_rows"] == 0, info
    assert info["path"] == (1 if env.get("AW_WINDOW") == "4096" else 0), info


def test_ragged_calls_on_the_partitioned_path(oracle, monkeypatch):
    """18 channels, 9000 taps: calls of 1, 4095, 4097, 807, ... frames (shorter than a block, one frame either side of it, head and interior windows)
    against the one call."""
    import airwave_amd as aw
    ctx = _context(monkeypatch, {})
    h, lt, rt, x, ref = _case(oracle, 18, 9000)
    sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    whole = sp.process(x)
    assert sp.info()["path"] == 1 and sp.info()["partitions"] == 3
    sp.reset()
    calls = [1, 4095, 4097, 807, 8192, 2, 2806]
    assert sum(calls) == F
    parts, at = [], 0
    for n in calls:
        parts.append(sp.process(np.ascontiguousarray(x[:, at:at + n])))
        at += n
    two = np.concatenate(parts, axis=1)
    diff = float(np.max(np.abs(two - whole)) / np.max(np.abs(whole)))
    worst = max(oracle.peak_rel_error(two[s], ref[s]) for s in range(S))
    print(f"FIGURE wide ragged 18ch 9000 taps: {len(calls)} calls against one {diff:.2e} of peak; peak_rel_error {worst:.2e}")
    assert diff <= SPLIT_TOL and worst < TOL


def test_pcm_s16_in_s24_out_at_24_channels(oracle):
    """The PCM entry on a wide layout: s16 input decodes to an exact float32 input, so the float32 output equals the float entry's bits on the decoded
    input and is within tolerance of the truth; the s24 output is numpy's encode (round half to even, saturate) of those bits, clips counted."""
    import torch
    import airwave_amd as aw
    from test_gpu_pcm import F32, S16, S24, context, decode, encode, make_pcm, run_f32_device, run_pcm_device
    ctx = context(aw, torch)
    C, frames = 24, 12001
    h = oracle.synth_hrir(14, 4320, seed=22)
    lt, rt = sr.maps(C)
    x_pcm = make_pcm(np.random.default_rng(24), S16, (S, frames, C), level=0.02)
    x = decode(S16, x_pcm)

    def spatializer():
        return aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    yf = run_f32_device(aw, torch, spatializer(), x, (frames,))
    got_f = run_pcm_device(aw, torch, spatializer(), x_pcm, S16, F32, (frames,))
    assert np.array_equal(got_f.view(np.uint32), yf.view(np.uint32))
    worst = max(oracle.peak_rel_error(yf[s], oracle.spatialize_f64(x[s], h, lt, rt)) for s in range(S))
    print(f"FIGURE wide pcm 24ch s16 -> f32: peak_rel_error {worst:.2e}; peak {np.abs(yf).max():.3f}")
    assert worst < TOL
    sp = spatializer()
    clip_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = run_pcm_device(aw, torch, sp, x_pcm, S16, S24, (frames,), clip_t)
    want, n_clip = encode(S24, yf)
    assert sp.info()["path"] == 0 and sp.info()["fft"] == 8192, sp.info()
    assert np.array_equal(got, want) and int(clip_t.item()) == n_clip
