"""GPU parity resolved by frequency band, by transform bin and by HRIR tap (tests/spectral_ref.py), through aw.Spatializer.process on every
kernel family: the 8192- and 16384-frame overlap-save tiles, the overlap-add tile, the partitioned kernels (marched and block-group CMAC) and the
long-window kernels (32, 40 and 128 rows; the 8-point rows kernel; host- and device-built tables).  The other parity tests feed white noise
through a decaying HRIR and take one peak-relative maximum, which a filter-table entry wrong to three digits passes and which a dropped last tap of
a long HRIR fails by no margin (test_spectral_ref.py); here the same tolerance holds per band, per tone and for HRIRs whose last taps carry the energy.

Two streams per case.  Each case asserts the kernel path it ran on (info()), so that a policy change cannot quietly move it to another kernel.
The knobs are read when a context / a spatializer is created: one context per knob set, as in test_gpu_launch_tables.py."""
import numpy as np
import pytest

import spectral_cases as sc
import spectral_ref as sr
from spectral_ref import TOL

pytestmark = pytest.mark.gpu
S = 2

# knob set -> (family, environment, frames of a call)
PATHS = {
    "ols8192": ("ols8192", {}, 20011),
    "ols16384": ("ols16384", {"AW_WINDOW": "16384", "AW_LW": "0"}, 20011),
    "ola": ("ola", {"AW_OLA": "1", "AW_OLA_MIN_BLOCKS": "0"}, 20011),
    "part-march": ("part", {"AW_WINDOW": "4096", "AW_LW": "0"}, 30000),
    "part-group": ("part", {"AW_WINDOW": "4096", "AW_LW": "0", "AW_PART_CMAC": "group"}, 30000),
    "lw32": ("lw32", {"AW_LW": "32"}, 150000),                      # two windows
    "lw40": ("lw40", {"AW_LW": "40"}, 150000),                      # two windows
    "lw128": ("lw128", {"AW_LW": "128"}, 60000),                    # a short call in a long window
    "lw32-rows8": ("lw32", {"AW_LW": "32", "AW_LW_ROWS_FORM": "8"}, 150000),
    "lw32-host-tables": ("lw32", {"AW_LW": "32", "AW_LW_TABLES": "host"}, 150000),
    "lw32-device-tables": ("lw32", {"AW_LW": "32", "AW_LW_TABLES": "gpu"}, 150000),
}

_contexts, _truth = {}, {}


def _fused_history(window, taps):
    """Frames a path-0 spatializer keeps between calls: the window minus its hop, the hop rounded down to 64 frames (DESIGN: line-aligned tiles)."""
    hop = window - (taps - 1 if window == 8192 else 2 * (taps // 2))
    return window - (hop - hop % 64 if hop > 16 * 64 else hop)


def _expected_info(path, channels, taps):
    family = PATHS[path][0]
    want = {"overlap_add_rows": 0, "long_window_rows": 0}
    if family.startswith("ols") or family == "ola":
        window = 16384 if family == "ols16384" else 8192
        want.update(path=0, fft=window, partitions=1, history=_fused_history(window, taps))
        if family == "ola":
            want["overlap_add_rows"] = min(8, (8192 - want["history"]) // 512)
    else:
        want.update(path=1, fft=8192, partitions=-(-taps // 4096), history=-(-taps // 4096) * 4096)
        if family.startswith("lw"):
            want["long_window_rows"] = int(family[2:])
    return want


def _truth_of(oracle, make, shared_as=None):
    """The inputs and the float64 truth of a case.  shared_as: the key under which it is computed once, kept unchanged and shared by every knob set
    that runs the case (the noise cases); a case that only one knob set runs is not kept."""
    if shared_as is not None and shared_as in _truth:
        return _truth[shared_as]
    h, lt, rt, x = make()
    ref = [oracle.spatialize_f64(x[s], h, lt, rt) for s in range(x.shape[0])]
    for a in (h, lt, rt, x, *ref):
        a.setflags(write=False)
    if shared_as is not None:
        _truth[shared_as] = (h, lt, rt, x, ref)
    return h, lt, rt, x, ref


def _spatializer(monkeypatch, path, h, lt, rt):
    import airwave_amd as aw
    env = PATHS[path][1]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    key = tuple(sorted(env.items()))
    if key not in _contexts:
        _contexts[key] = aw.Context(0)
    ctx = _contexts[key]
    return aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)


def _check_info(sp, path, channels, taps):
    info = sp.info()
    want = _expected_info(path, channels, taps)
    assert {k: info[k] for k in want} == want, (path, channels, taps, info)


# ---- white noise, error per band
NOISE = ([(p, c, None) for p in ("ols8192", "ols16384", "part-march", "part-group", "lw32", "lw40", "lw128") for c in sc.GPU_CHANNELS] +
         [("ola", c, None) for c in sc.GPU_OLA_CHANNELS] +
         [("lw32-rows8", 7, None), ("lw32-host-tables", 7, 32768), ("lw32-device-tables", 7, 32768)])


@pytest.mark.parametrize("path,channels,taps", NOISE, ids=[f"{p}-{c}ch" for p, c, _ in NOISE])
def test_error_per_band(oracle, monkeypatch, path, channels, taps):
    family, _, frames = PATHS[path]
    taps = sc.FAMILIES[family].taps if taps is None else taps
    h, lt, rt, x, ref = _truth_of(oracle, lambda: sc.noise_input(oracle, family, channels, S, frames, taps), shared_as=(family, channels, frames, taps))
    sp = _spatializer(monkeypatch, path, h, lt, rt)
    y = sp.process(x)
    _check_info(sp, path, channels, taps)
    for s in range(S):
        err, f, ear = sr.worst_band(y[s], ref[s], sc.FAMILIES[family].L)
        peak = oracle.peak_rel_error(y[s], ref[s])
        print(f"FIGURE band {path} {channels}ch stream {s}: band_rel_error {err:.2e} at bin {f} of ear {ear}; peak_rel_error {peak:.2e}")
        assert err < TOL and peak < TOL, (err, f, ear, peak)


# ---- single tones, one case per bin
TONES = [(p, t) for p in ("ols8192", "ols16384", "ola", "part-march", "part-group", "lw32", "lw40", "lw128") for t in sc.gpu_tones(PATHS[p][0])]


@pytest.mark.parametrize("path,t", TONES, ids=[sc.tone_id(t, p) for p, t in TONES])
def test_single_tones(oracle, monkeypatch, path, t):
    family, _, frames = PATHS[path]
    assert frames >= sc.FAMILIES[family].emu_frames            # the level check (test_spectral_ref.py) covers a prefix of this call
    h, lt, rt, x, ref = _truth_of(oracle, lambda: sc.tone_input(oracle, t, S, frames))
    sp = _spatializer(monkeypatch, path, h, lt, rt)
    y = sp.process(x)
    _check_info(sp, path, t.channels, sc.FAMILIES[family].taps)
    for s in range(S):
        for ear in range(2):
            err = oracle.peak_rel_error(y[s, :, ear], ref[s][:, ear])
            print(f"FIGURE tone {path} {sc.tone_id(t, path)} stream {s} ear {ear}: peak_rel_error {err:.2e}")
            assert err < TOL, (err, s, ear)


# ---- end-heavy HRIRs at the tap counts each kernel owns; on the kernels that carry a tail between calls also as two calls
END_HEAVY = [(p, c, taps) for p, edges in (("ols8192", "ols8192"), ("ols16384", "ols16384"), ("ola", "ola"), ("part-march", "part"), ("part-group", "part"),
                                           ("lw32", "lw"), ("lw40", "lw"), ("lw128", "lw"))
             for taps in sc.END_HEAVY_TAPS[edges] for c in (sc.GPU_OLA_CHANNELS if p == "ola" else sc.GPU_CHANNELS)]


@pytest.mark.parametrize("path,channels,taps", END_HEAVY, ids=[f"{p}-{c}ch-{t}taps" for p, c, t in END_HEAVY])
def test_end_heavy_hrirs(oracle, monkeypatch, path, channels, taps):
    family, _, frames = PATHS[path]
    carried = family == "part" or family.startswith("lw")
    history = -(-taps // 4096) * 4096
    if carried and frames < history + 5001:
        frames = history + 10001                                # room for a second call behind the split
    h, lt, rt, x, ref = _truth_of(oracle, lambda: sc.end_heavy_input(oracle, channels, taps, S, frames))
    sp = _spatializer(monkeypatch, path, h, lt, rt)
    y = sp.process(x)
    _check_info(sp, path, channels, taps)
    for s in range(S):
        for ear in range(2):
            err = oracle.peak_rel_error(y[s, :, ear], ref[s][:, ear])
            print(f"FIGURE end-heavy {path} {channels}ch {taps} taps stream {s} ear {ear}: peak_rel_error {err:.2e}")
            assert err < TOL, (err, s, ear)
    if not carried:
        return
    # the same timeline as two calls, split one frame behind the history: the carried tail is where `taps - 1` against `taps` would show
    assert sp.info()["history"] == history
    sp.reset()
    cut = history + 1
    parts = []
    for lo, hi in ((0, cut), (cut, frames)):
        parts.append(sp.process(np.ascontiguousarray(x[:, lo:hi])))
        _check_info(sp, path, channels, taps)
    two = np.concatenate(parts, axis=1)
    diff = float(np.max(np.abs(two - y)) / np.max(np.abs(y)))
    print(f"FIGURE split {path} {channels}ch {taps} taps: two calls against one {diff:.2e} of peak")
    assert diff <= 3e-6
    for s in range(S):
        assert oracle.peak_rel_error(two[s], ref[s]) < TOL
