"""The three instruments of spectral_ref.py on the code the GPU runs: every kernel family's device source under thread emulation (tests/emu/)
against the float64 truth, measured per frequency band (white noise), per transform bin (single tones through an HRIR with a unit first tap) and
per HRIR tap (HRIRs whose last taps carry the energy, at the tap counts where a window, block or partition count changes).  The existing
emulation tests (test_emu_tile.py, test_emu_ola.py, test_emu_lw.py) use white noise, decaying HRIRs and one peak-relative maximum, which a filter
table entry wrong to three digits passes and which a dropped last tap of a long HRIR fails or passes by the luck of that tap's draw
(test_spectral_ref.py shows both).  One stream per case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
import spectral_cases as sc  # noqa: E402
import spectral_ref as sr  # noqa: E402
from spectral_ref import TOL  # noqa: E402

# kernel -> (family, emulated call, frames of a noise call).  Frame counts as in test_emu_tile.py / test_emu_ola.py / test_emu_lw.py: head, interior
# and ragged last tiles of the on-chip kernels; one window of 32 rows filled to three quarters, the larger windows as short calls.
KERNELS = {
    "ols-v1": ("ols8192", lambda x, h, lt, rt, hist: emu.fused_ols(x, h, lt, rt, variant=1), 16500),
    "ols-v5": ("ols8192", lambda x, h, lt, rt, hist: emu.fused_ols(x, h, lt, rt, variant=5), 16500),       # the two-pass form of the wide layouts
    "ols-v2": ("ols16384", lambda x, h, lt, rt, hist: emu.fused_ols(x, h, lt, rt, variant=2), 16500),
    "ola": ("ola", lambda x, h, lt, rt, hist: emu.fused_ola(x, h, lt, rt, workgroups=2), 16500),
    "part-march": ("part", lambda x, h, lt, rt, hist: emu.partitioned(x, h, lt, rt, hist=hist, cmac="march"), 16500),
    "part-group": ("part", lambda x, h, lt, rt, hist: emu.partitioned(x, h, lt, rt, hist=hist, cmac="group"), 16500),
    "lw32-pb2": ("lw32", lambda x, h, lt, rt, hist: emu.longwin(x, h, lt, rt, R=32, rows_pb=2, hist=hist), 100000),
    "lw32-pb16": ("lw32", lambda x, h, lt, rt, hist: emu.longwin(x, h, lt, rt, R=32, rows_pb=16, hist=hist), 100000),
    "lw40": ("lw40", lambda x, h, lt, rt, hist: emu.longwin(x, h, lt, rt, R=40, rows_pb=16, hist=hist), 30000),
    "lw128": ("lw128", lambda x, h, lt, rt, hist: emu.longwin(x, h, lt, rt, R=128, rows_pb=2, hist=hist), 20000),
}
# the emulation costs 0.1 - 0.3 s per tile and channel pair and 0.6 - 2.5 s per long window: the tone cases, which probe bins and not tile positions, run on
# short calls (spectral_cases.FAMILIES: emu_frames) and on the narrowest layout the kernel has


def _run(oracle, kernel, h, lt, rt, x, hist_len=0):
    """One stream of x through the emulated kernel, the first hist_len frames as the history of an earlier call; (y, truth) of the frames behind them."""
    hist = x[:, :hist_len].copy() if hist_len else None
    y = KERNELS[kernel][1](x[:, hist_len:], h, lt, rt, hist)
    assert not np.isnan(y).any()
    return y[0], oracle.spatialize_f64(x[0], h, lt, rt)[hist_len:]


# ---- white noise, error per band: one odd and one even channel count per kernel (the overlap-add tile: of its narrow and of its wide kernels)
NOISE = [("ols-v1", 7), ("ols-v1", 8), ("ols-v5", 13), ("ols-v5", 14), ("ols-v2", 5), ("ols-v2", 8), ("ola", 7), ("ola", 8), ("ola", 13), ("ola", 14),
         ("part-march", 7), ("part-march", 8), ("part-group", 5), ("part-group", 8), ("lw32-pb2", 7), ("lw32-pb2", 8), ("lw32-pb16", 7),
         ("lw32-pb16", 8), ("lw40", 3), ("lw40", 2), ("lw128", 1), ("lw128", 2)]


@pytest.mark.parametrize("kernel,channels", NOISE, ids=[f"{k}-{c}ch" for k, c in NOISE])
def test_emulated_kernels_error_per_band(oracle, kernel, channels):
    family, _, frames = KERNELS[kernel]
    y, ref = _run(oracle, kernel, *sc.noise_input(oracle, family, channels, 1, frames))
    err, f, ear = sr.worst_band(y, ref, sc.FAMILIES[family].L)
    print(f"band_rel_error {kernel} {channels}ch: {err:.2e} at bin {f} of ear {ear}")
    assert err < TOL, (err, f, ear)


# ---- single tones, one case per bin: a failure names its bin
TONE_KERNELS = {("ols8192", 3): "ols-v1", ("ols8192", 10): "ols-v5", ("ols16384", 2): "ols-v2", ("ola", 8): "ola", ("ola", 14): "ola",
                ("part", 3): "part-march", ("part", 2): "part-group", ("lw32", 1): "lw32-pb2", ("lw32", 2): "lw32-pb16", ("lw40", 1): "lw40",
                ("lw128", 2): "lw128"}
TONES = [t for family in sc.FAMILIES for t in sc.emu_tones(family)]


@pytest.mark.parametrize("t", TONES, ids=[sc.tone_id(t, TONE_KERNELS[t.family, t.channels]) for t in TONES])
def test_emulated_kernels_single_tones(oracle, t):
    kernel = TONE_KERNELS[t.family, t.channels]
    y, ref = _run(oracle, kernel, *sc.tone_input(oracle, t, 1, sc.FAMILIES[t.family].emu_frames))
    for ear in range(2):
        err = oracle.peak_rel_error(y[:, ear], ref[:, ear])
        print(f"tone peak_rel_error {sc.tone_id(t, kernel)} ear {ear}: {err:.2e}")
        assert err < TOL, (err, ear)


# ---- end-heavy HRIRs at the tap counts each kernel owns.  The last tap only multiplies frames that are `taps - 1` old: the kernels that carry a tail
# between calls get one as long as they keep it (noise, the head of the same timeline), and a call behind it of three blocks / of one window.
END_HEAVY = ([("ols-v1", 7, taps) for taps in sc.END_HEAVY_TAPS["ols8192"]] + [("ols-v5", 14, taps) for taps in sc.END_HEAVY_TAPS["ols8192"]] +
             [("ols-v2", 5, taps) for taps in sc.END_HEAVY_TAPS["ols16384"]] + [("ola", c, taps) for c in (8, 14) for taps in sc.END_HEAVY_TAPS["ola"]] +
             [(k, 3, taps) for k in ("part-march", "part-group") for taps in sc.END_HEAVY_TAPS["part"]] +
             [(k, c, taps) for k, c in (("lw32-pb2", 3), ("lw32-pb16", 2)) for taps in sc.END_HEAVY_TAPS["lw"]] + [("lw40", 3, 20481), ("lw128", 2, 32769)])


@pytest.mark.parametrize("kernel,channels,taps", END_HEAVY, ids=[f"{k}-{c}ch-{t}taps" for k, c, t in END_HEAVY])
def test_emulated_kernels_end_heavy_hrirs(oracle, kernel, channels, taps):
    family, _, frames = KERNELS[kernel]
    hist_len = 0
    if family == "part":
        hist_len, frames = -(-taps // 4096) * 4096, 9000
    elif family.startswith("lw"):
        hist_len = taps - 1                                      # emu.longwin: hop = N - (taps - 1)
        frames = min(frames, int(family[2:]) * 4096 - hist_len)  # one window
    y, ref = _run(oracle, kernel, *sc.end_heavy_input(oracle, channels, taps, 1, hist_len + frames), hist_len=hist_len)
    for ear in range(2):
        err = oracle.peak_rel_error(y[:, ear], ref[:, ear])
        print(f"end-heavy peak_rel_error {kernel} {channels}ch {taps} taps ear {ear}: {err:.2e}")
        assert err < TOL, (err, ear)
