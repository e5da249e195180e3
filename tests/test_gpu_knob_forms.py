"""The kernel forms behind five documented knobs that no other test sets, on the GPU:

  AW_HOP_ALIGN        hops that are odd or no multiple of 64 on the 8192-frame tile, the 16384-frame tile and the overlap-add tile
  AW_PART_HERM=0      the partitioned path storing the redundant half of an odd layout's last pair too
  AW_LW_ROWS16_WGS    the 16-point rows kernel's persistent grid at 1, 2 and 4 workgroups per CU: the same tiles dealt differently
  AW_EQ_EAR_SPLIT     aw_eq_cascade_kernel<2> (both ears in one workgroup) below 384 streams, <1> (one workgroup per ear) above
  AW_HOST_OUT_ASYNC=0 the host entry copying a chunk's output on the driver thread

Float64 truth at test_gpu_parity's tolerance per stream and ear; two calls against one, and one kernel form against another, at 3e-6 of peak; forms
that only re-deal tiles or move a copy to another thread must give the same bits.  One context per knob set (test_gpu_launch_tables.py)."""
import numpy as np
import pytest

import spectral_ref as sr
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
S = 2
SPLIT_TOL = 3e-6
KNOBS = ("AW_WINDOW", "AW_LW", "AW_OLA", "AW_OLA_MIN_BLOCKS", "AW_PART_CMAC", "AW_PART_HERM", "AW_HOP_ALIGN", "AW_LW_ROWS16_WGS", "AW_EQ_EAR_SPLIT",
         "AW_HOST_OUT_ASYNC", "AW_HOST_CHUNK_MB")

_truth, _contexts, _outputs = {}, {}, {}


def _case(oracle, channels, taps, streams, frames):
    key = (channels, taps, streams, frames)
    if key not in _truth:
        h = oracle.synth_hrir(14, taps, seed=taps)
        lt, rt = sr.maps(channels)
        x = oracle.synth_input(streams, frames, channels, seed=channels)
        ref = [oracle.spatialize_f64(x[s], h, lt, rt) for s in range(streams)]
        for a in (h, lt, rt, x, *ref):
            a.setflags(write=False)
        _truth[key] = (h, lt, rt, x, ref)
    return _truth[key]


def _context(monkeypatch, env, **kw):
    import airwave_amd as aw
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    key = tuple(sorted(env.items())) + tuple(sorted(kw.items()))
    if key not in _contexts:
        _contexts[key] = aw.Context(0, **kw)
    return _contexts[key]


def _worst(oracle, y, ref):
    assert np.isfinite(y).all()
    return max(oracle.peak_rel_error(y[s, :, ear], ref[s][:, ear]) for s in range(y.shape[0]) for ear in range(2))


# ---- AW_HOP_ALIGN
def align_hop(hop_align, hop):
    """host/path_policy.hpp restated: below 2 the rounding is off, a hop of at most 16 hop_align frames is left alone."""
    return hop - hop % hop_align if hop_align > 1 and hop > 16 * hop_align else hop


TILES = {"ols8192": (8192, {"AW_WINDOW": "8192", "AW_OLA": "0", "AW_LW": "0"}),
         "ols16384": (16384, {"AW_WINDOW": "16384", "AW_LW": "0"}),
         "ola": (8192, {"AW_OLA": "1", "AW_OLA_MIN_BLOCKS": "0", "AW_LW": "0"})}
HOP_CASES = ([("ols8192", 4320, c, a) for c in (2, 7, 14) for a in (1, 32, 128)] +
             [("ols16384", taps, c, a) for taps in (4320, 8640) for c in (2, 7) for a in (1, 32, 128)] +
             [("ols16384", 4320, c, 3) for c in (2, 7)] +          # an odd alignment: plan_create keeps this tile's hop even (12 063 -> 12 062)
             [("ola", 4320, c, a) for c in (8, 14) for a in (1, 32, 128)])


@pytest.mark.parametrize("tile,taps,channels,hop_align", HOP_CASES, ids=[f"{t}-{n}taps-{c}ch-align{a}" for t, n, c, a in HOP_CASES])
def test_hop_alignments(oracle, monkeypatch, tile, taps, channels, hop_align):
    import airwave_amd as aw
    window, env = TILES[tile]
    natural = window - (taps - 1) if window == 8192 else window - 2 * (taps // 2)
    hop = align_hop(hop_align, natural)
    if window == 16384:
        hop -= hop % 2
    frames = 20011 if window == 8192 else 30011
    ctx = _context(monkeypatch, {**env, "AW_HOP_ALIGN": str(hop_align)})
    h, lt, rt, x, ref = _case(oracle, channels, taps, S, frames)
    sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    y = sp.process(x)
    info = sp.info()
    assert (info["path"], info["fft"], info["hop"], info["history"], info["long_window_rows"]) == (0, window, hop, window - hop, 0), info
    assert info["overlap_add_rows"] == (7 if tile == "ola" else 0), info
    worst = _worst(oracle, y, ref)
    print(f"FIGURE knob hop-align {tile} {channels}ch {taps} taps AW_HOP_ALIGN={hop_align} hop {hop}: peak_rel_error {worst:.2e}")
    assert worst < TOL
    sp.reset()
    cut = hop + hop // 2 + 3 if tile != "ola" else 3584 + 1795              # no multiple of the hop (overlap-add: of its 3584-frame block either)
    assert cut % hop and cut % 3584 and cut < frames
    two = np.concatenate([sp.process(np.ascontiguousarray(x[:, lo:hi])) for lo, hi in ((0, cut), (cut, frames))], axis=1)
    diff = float(np.max(np.abs(two - y)) / np.max(np.abs(y)))
    print(f"FIGURE knob hop-align split {tile} {channels}ch {taps} taps AW_HOP_ALIGN={hop_align}: two calls against one {diff:.2e} of peak")
    assert diff <= SPLIT_TOL and _worst(oracle, two, ref) < TOL


# ---- AW_PART_HERM=0
@pytest.mark.parametrize("cmac", ["march", "group"])
@pytest.mark.parametrize("channels", [1, 3, 7, 13])
def test_partitioned_path_without_the_hermitian_store(oracle, monkeypatch, channels, cmac):
    """Odd layouts, 9000 taps (3 partitions): the last pair is one real channel, whose spectrum the default form stores by half."""
    import airwave_amd as aw
    base = {"AW_WINDOW": "4096", "AW_LW": "0", **({"AW_PART_CMAC": "group"} if cmac == "group" else {})}
    h, lt, rt, x, ref = _case(oracle, channels, 9000, S, 20011)
    ys = {}
    for herm in (None, "0"):
        ctx = _context(monkeypatch, {**base, **({"AW_PART_HERM": herm} if herm else {})})       # (read when the spatializer is created)
        sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
        ys[herm] = sp.process(x)
        assert (sp.info()["path"], sp.info()["partitions"], sp.info()["long_window_rows"]) == (1, 3, 0), sp.info()
        worst = _worst(oracle, ys[herm], ref)
        print(f"FIGURE knob part-herm {cmac} {channels}ch AW_PART_HERM={herm or 'default'}: peak_rel_error {worst:.2e}")
        assert worst < TOL
    diff = float(np.max(np.abs(ys["0"] - ys[None])) / np.max(np.abs(ys[None])))
    print(f"FIGURE knob part-herm {cmac} {channels}ch: whole store against half store {diff:.2e} of peak")
    assert diff <= SPLIT_TOL


# ---- AW_LW_ROWS16_WGS
def _lw_run(oracle, monkeypatch, rows, channels, streams, wgs):
    import airwave_amd as aw
    key = (rows, channels, streams, wgs)
    if key not in _outputs:
        taps = 4320
        frames = rows * 4096 - 4352 + 20000                                   # two windows (history of a 4320-tap spatializer: 4352 frames)
        h, lt, rt, x, ref = _case(oracle, channels, taps, streams, frames)
        ctx = _context(monkeypatch, {"AW_LW": str(rows), **({"AW_LW_ROWS16_WGS": str(wgs)} if wgs else {})})
        sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=streams, ctx=ctx)
        y = sp.process(x)
        assert sp.info()["long_window_rows"] == rows and sp.info()["long_window_rows_rest"] == 0, sp.info()
        worst = _worst(oracle, y, ref)
        print(f"FIGURE knob rows16-wgs lw{rows} {channels}ch {streams} streams AW_LW_ROWS16_WGS={wgs or 'default'}: peak_rel_error {worst:.2e}")
        assert worst < TOL
        y.setflags(write=False)
        _outputs[key] = y
    return _outputs[key]


@pytest.mark.parametrize("wgs", [1, 2, 4])
@pytest.mark.parametrize("streams", [3, 5])
@pytest.mark.parametrize("channels", [7, 14])
@pytest.mark.parametrize("rows", [32, 40])
def test_rows_kernel_grid_sizes_give_the_same_bits(oracle, monkeypatch, rows, channels, streams, wgs):
    """16 / 20 row pairs x (3 | 5 streams x 2 windows) tiles over 1, 2 or 4 workgroups per CU: which workgroup computes a tile changes, the
    tile's arithmetic does not."""
    y = _lw_run(oracle, monkeypatch, rows, channels, streams, wgs)
    assert np.array_equal(y.view(np.uint32), _lw_run(oracle, monkeypatch, rows, channels, streams, None).view(np.uint32))


# ---- AW_EQ_EAR_SPLIT
@pytest.fixture
def both_ears(monkeypatch):
    """A context whose EQ kernel takes both ears of a stream in one workgroup (the automatic rule splits the ears up to 384 streams)."""
    return _context(monkeypatch, {"AW_EQ_EAR_SPLIT": "0"})


@pytest.mark.parametrize("calls", [[1, 15, 16, 17], [31, 32, 33, 64], [4095, 4096, 4097], [8191, 8192, 8193], [10000, 3, 70000], [8192, 8192]])
def test_both_ears_kernel_over_ragged_calls(oracle, both_ears, calls):
    import airwave_amd as aw
    import test_gpu_eq as t
    t.check_state_batch_over_ragged_calls(aw, oracle, calls, ctx=both_ears)           # S = 5 there


def test_both_ears_kernel_sixty_four_filters_and_other_rates(oracle, both_ears):
    import airwave_amd as aw
    import test_gpu_eq as t
    t.check_sixty_four_filters_and_other_rates(aw, oracle, S=5, ctx=both_ears)


def test_both_ears_kernel_crossfade(oracle, both_ears):
    import airwave_amd as aw
    import test_gpu_eq as t
    t.check_processor_batch_crossfade(aw, oracle, S=5, ctx=both_ears)


def test_both_ears_kernel_low_frequency_cascade(oracle, both_ears, golden_dir):
    import airwave_amd as aw
    import test_gpu_eq as t
    t.check_low_frequency_cascade(aw, oracle, golden_dir, S=5, ctx=both_ears)


def test_one_workgroup_per_ear_above_384_streams(oracle, monkeypatch):
    """390 streams x 4097 frames with AW_EQ_EAR_SPLIT=1: the stream mapping (b >> 4) * 8 + (b & 7) past the automatic rule's last batch, a last group
    of six streams; the first, a middle and the last stream against the oracle at test_gpu_eq's one unit in the last place."""
    import airwave_amd as aw
    import test_gpu_eq as t
    n_streams, frames = 390, 4097
    ctx = _context(monkeypatch, {"AW_EQ_EAR_SPLIT": "1"})
    st = aw.ParametricEqualizerState(t.adef(aw, -2.56, t.FILTERS), 48000.0, n_streams=n_streams, ctx=ctx)
    x = np.random.default_rng(390).uniform(-0.5, 0.5, (n_streams, frames, 2)).astype(np.float32)
    y = st.process_batch(x)
    assert np.isfinite(y).all()
    worst = 0.0
    for s in (0, 199, n_streams - 1):
        el, er = oracle.eq_prepare(t.odef(oracle, -2.56, t.FILTERS), 48000.0).process(x[s, :, 0], x[s, :, 1])
        worst = max(worst, float(np.max(np.abs(y[s, :, 0] - el))), float(np.max(np.abs(y[s, :, 1] - er))))
    print(f"FIGURE knob eq-ear-split=1 {n_streams} streams x {frames} frames: max abs error {worst:.2e} (bound {t.ULP:.0e})")
    assert worst <= t.ULP


# ---- AW_HOST_OUT_ASYNC=0
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_host_entry_output_copy_on_the_driver_thread(oracle, monkeypatch, fmt):
    """Pageable buffers, 8 MB chunks (37 streams: several chunks and a ragged last one), two calls: where a chunk's output is copied from does
    not change a bit of it."""
    import airwave_amd as aw
    from test_gpu_pcm import S16, make_pcm
    streams, channels, splits = 37, 8, (40001, 36003)           # (a call is chunked from twice the chunk size on: 21 MB of s16 in the shorter one)
    h = oracle.synth_hrir(14, 4320, seed=3)
    lt, rt = sr.maps(channels)
    if fmt == "f32":
        x_all = oracle.synth_input(streams, sum(splits), channels, seed=99)
    else:
        x_all = make_pcm(np.random.default_rng(13), S16, (streams, sum(splits), channels), level=0.3)
    got = {}
    for mode in (None, "0"):
        ctx = _context(monkeypatch, {"AW_HOST_CHUNK_MB": "8", **({"AW_HOST_OUT_ASYNC": mode} if mode else {})})
        sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=streams, ctx=ctx)
        outs, at = [], 0
        for n in splits:
            x = np.ascontiguousarray(x_all[:, at:at + n])
            y = np.full((streams, n, 2), np.nan, np.float32) if fmt == "f32" else np.zeros((streams, n, 2), np.int16)
            if fmt == "f32":
                sp.process_host_into(x, y)
            else:
                sp.process_host_into(x, y, in_format="s16", out_format="s16")
            outs.append(y)
            at += n
        assert 0 < sp.info()["host_chunk_streams"] < streams, sp.info()
        got[mode] = np.concatenate(outs, axis=1)
    assert np.array_equal(got["0"].view(np.uint8), got[None].view(np.uint8))
    if fmt == "f32":
        worst = max(oracle.peak_rel_error(got["0"][s, :20000], oracle.spatialize_f64(x_all[s, :20000], h, lt, rt)) for s in (0, streams - 1))
        print(f"FIGURE knob host-out-async=0 f32 {streams} streams: peak_rel_error {worst:.2e}; bit-identical to the default")
        assert worst < TOL
    else:
        print(f"FIGURE knob host-out-async=0 s16 {streams} streams: bit-identical to the default, {int(np.count_nonzero(got['0']))} non-zero samples")
        assert np.count_nonzero(got["0"]) > got["0"].size // 2
