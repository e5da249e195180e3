"""Per-stream BS.1770 integrated loudness of the batch entries on the MI355X (aw_spatializer_set_loudness / _get_loudness /
_get_loudness_hops).  The reference everywhere is loudness_ref.py: the float64 recurrence, `reshape` hop sums and the gating in numpy,
applied to known signals or to the float32 output the same call wrote.  Chunking, sample formats and sharding must not change a bit of
any hop energy; with loudness off a handle writes what it always has."""
import numpy as np
import pytest

import loudness_ref as ref
from test_emu_loudness import BOUND
from test_gpu_pcm_dither import F32, S16, NAME, context, from_dev, layout, out_host, to_dev

pytestmark = pytest.mark.gpu

TAPS, RATE = 4320, 48000


def delta_spatializer(aw, ctx, rate, streams):
    """2 input channels -> 2 ears through a unit impulse (and a silent track for the crossed paths): the output is the input, up to the
    convolution's own float32 rounding."""
    h = np.zeros((2, 256), np.float32)
    h[0, 0] = 1.0
    lt, rt = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    return aw.Spatializer(aw.HRIR(h, sample_rate=float(rate), ctx=ctx), lt, rt, n_streams=streams, ctx=ctx)


def real_spatializer(aw, ctx, oracle, streams, seed=51):
    lt, rt = layout(7)
    return aw.Spatializer(aw.HRIR(oracle.synth_hrir(14, TAPS, seed=seed), sample_rate=float(RATE), ctx=ctx), lt, rt, n_streams=streams, ctx=ctx)


def host_call(sp, x, fout=F32):
    y = out_host(fout, x.shape[0], x.shape[1])
    sp.process_host_into(np.ascontiguousarray(x), y, out_format=NAME[fout])
    return y


def device_call(torch, sp, x, fout=F32):
    yo = out_host(fout, x.shape[0], x.shape[1])
    xd, yd = to_dev(torch, x), torch.empty(yo.nbytes, dtype=torch.uint8, device="cuda")
    if fout == F32:
        sp.process_device(xd.data_ptr(), yd.data_ptr(), x.shape[1])
    else:
        sp.process_pcm_device(xd.data_ptr(), "f32", yd.data_ptr(), NAME[fout], x.shape[1])
    torch.cuda.synchronize()
    return from_dev(yd, yo)


def all_hops(sp, n):
    return np.stack([sp.loudness_hops(s, 0, n) for s in range(sp.n_streams)])


def reference_hops(y, rate):
    """Complete-hop energies [S][hops] and non-finite counts [S] of float32 output y [S, F, 2], by the frame-by-frame recurrence."""
    hop = rate // 10
    v = np.asarray(y, np.float64)
    bad = ~np.isfinite(v)
    v = np.where(bad, 0.0, v)
    k, _ = ref.k_weight_loop(np.moveaxis(v, 1, -1), rate)
    return np.stack([ref.hop_energies(k[s, 0], k[s, 1], hop) for s in range(y.shape[0])]), bad.sum(axis=(1, 2))


def check_against_reference(ld, hops, want_hops, rate, what, skip=None):
    """Hop energies within the reassociation bound, integrated loudness within 4.35 x bound LU (10 log10(1 + d)), counts equal.
    skip: a mask of hops left out of the first comparison."""
    hop = rate // 10
    n = want_hops.shape[1]
    rel = np.abs(hops[:, :n] - want_hops) / want_hops
    err = float(np.max(rel if skip is None else np.where(skip, 0.0, rel)))
    print(f"{what}: relative error of the hop energies {err:.3e} (bound {BOUND:.3e})")
    assert err <= BOUND, (what, err)
    for s in range(want_hops.shape[0]):
        g = ref.gate(want_hops[s], hop)
        assert (ld["blocks"][s], ld["blocks_above_absolute"][s], ld["blocks_gated"][s]) == (g["blocks"], g["above_absolute"], g["gated"]), (what, s, ld[s], g)
        for got, want in ((ld["integrated_lufs"][s], g["integrated"]), (ld["relative_threshold_lufs"][s], g["relative_threshold"])):
            print(f"{what}: stream {s}: {got:.12f} LUFS, reference {want:.12f}")
            assert (got == want) if np.isinf(want) else abs(got - want) <= 4.35 * BOUND, (what, s, got, want)


# ---- 1. known answers: EBU Tech 3341, stereo 1 kHz sine -------------------------------------------------------------------------------------

def ebu_signal(case, rate):
    """[frames][2] float32: (level dBFS, seconds) sections of a stereo 1 kHz sine."""
    sections = {1: [(-23, 20)], 2: [(-33, 20)], 3: [(-36, 10), (-23, 60), (-36, 10)], 4: [(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)],
                5: [(-26, 20), (-20, 20.1), (-26, 20)]}[case]
    amp = np.concatenate([np.full(int(round(sec * rate)), 10.0 ** (db / 20.0)) for db, sec in sections])
    s = (amp * np.sin(2 * np.pi * 1000.0 / rate * np.arange(amp.size))).astype(np.float32)
    return np.stack([s, s], axis=1)


EBU = [(1, 48000, -23.0), (2, 48000, -33.0), (3, 48000, -23.0), (4, 48000, -23.0), (5, 48000, -23.0), (1, 44100, -23.0), (1, 96000, -23.0)]


@pytest.mark.parametrize("case,rate,target", EBU)
def test_ebu_tech_3341_known_answers(case, rate, target):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    x = ebu_signal(case, rate)[None]
    sp = delta_spatializer(aw, ctx, rate, 1)
    sp.set_loudness(True, x.shape[1] / rate)
    assert sp.info()["loudness"] == 1
    y = host_call(sp, x)
    ld = sp.loudness()[0]
    want = ref.measure(y[0], rate)
    print(f"case {case} at {rate} Hz: {ld['integrated_lufs']:.4f} LUFS (reference {want['integrated']:.4f}), blocks "
          f"{ld['blocks']} / {ld['blocks_above_absolute']} / {ld['blocks_gated']}")
    assert abs(ld["integrated_lufs"] - target) <= 0.1 and abs(want["integrated"] - target) <= 0.1
    assert (ld["blocks"], ld["blocks_above_absolute"], ld["blocks_gated"]) == (want["blocks"], want["above_absolute"], want["gated"])
    if case == 3:
        assert (want["blocks"], want["above_absolute"], want["gated"]) == (797, 797, 603)
    if case == 4:
        assert (want["blocks"], want["above_absolute"], want["gated"]) == (997, 803, 603)
    assert ld["frames"] == x.shape[1] and ld["frames_dropped"] == 0 and ld["nonfinite"] == 0
    assert abs(aw.loudness_gain(ld["integrated_lufs"], -16.0) - 10 ** ((-16.0 - ld["integrated_lufs"]) / 20)) < 1e-6


# ---- 2. parity on a real layout -------------------------------------------------------------------------------------------------------

def parity_input():
    """3 streams x (2 s + 777 frames) x 7 channels of seeded noise.  Stream 1 falls, after 0.7 s, to -20 dB for 0.3 s (blocks that only
    the relative gate removes) and then to a tail of 1 s near -80 dBFS at the output (blocks below the absolute gate)."""
    F = 2 * RATE + 777
    x = np.random.default_rng(52).uniform(-0.5, 0.5, (3, F, 7)).astype(np.float32)
    x[1, F - RATE - 3 * (RATE // 10): F - RATE] *= np.float32(0.1)
    x[1, F - RATE:] *= np.float32(1e-4)
    return x


def test_parity_with_numpy_on_a_real_layout(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    x = parity_input()
    sp = real_spatializer(aw, ctx, oracle, 3)
    sp.set_loudness(True, 3.0)
    y = device_call(torch, sp, x)
    hop = RATE // 10
    want_hops, _ = reference_hops(y, RATE)
    # the reference itself must exercise both gates, away from their edges, or the comparison below shows nothing
    z, l = ref.block_loudness(want_hops[1], hop)
    g = ref.gate(want_hops[1], hop)
    assert np.count_nonzero(l <= -70.0) >= 2 and np.count_nonzero((l > -70.0) & (l <= g["relative_threshold"])) >= 2
    tail = y[1, -RATE + TAPS:].astype(np.float64)                   # (past the HRIR's length: the louder frames before it have rung out)
    assert -86.0 < 10 * np.log10(np.mean(tail ** 2)) < -74.0
    for s in range(3):
        zs, ls = ref.block_loudness(want_hops[s], hop)
        gs = ref.gate(want_hops[s], hop)
        assert np.min(np.abs(10 ** ((ls + 70.0) / 10) - 1)) > 1e-6 and np.min(np.abs(10 ** ((ls - gs["relative_threshold"]) / 10) - 1)) > 1e-6
    ld = sp.loudness()
    check_against_reference(ld, all_hops(sp, want_hops.shape[1]), want_hops, RATE, "real layout")
    assert np.all(ld["frames"] == x.shape[1]) and not ld["frames_dropped"].any() and not ld["nonfinite"].any() and not ld["reserved"].any()
    assert 0 < ld["blocks_gated"][1] < ld["blocks_above_absolute"][1] < ld["blocks"][1] == 17


# ---- 3. invariances -------------------------------------------------------------------------------------------------------------------

def test_chunking_formats_and_sharding_change_no_bit(oracle):
    import torch
    import airwave_amd as aw
    S, F = 5, RATE // 2 + 777
    x = np.random.default_rng(53).uniform(-0.5, 0.5, (S, F, 7)).astype(np.float32)
    x[2] *= np.float32(0.01)
    n = -(-F // (RATE // 10))
    ctx = context(aw, torch, chunk_mb=64)

    def measured(c, streams, first, run):
        sp = real_spatializer(aw, c, oracle, streams)
        sp.set_loudness(True, 1.0)
        run(sp, x[first:first + streams])
        return all_hops(sp, n), sp

    kept = {}
    one, _ = measured(ctx, S, 0, lambda sp, xs: kept.update(y=device_call(torch, sp, xs)))
    assert np.all(one[:, : F // (RATE // 10)] > 0)
    small = context(aw, torch, chunk_mb=1)
    chunked, sp_c = measured(small, S, 0, lambda sp, xs: host_call(sp, xs))
    assert 0 < sp_c.info()["host_chunk_streams"] < S
    assert np.array_equal(chunked, one)
    pinned_x = small.pinned_empty(x.shape, x.dtype)
    pinned_x[...] = x
    pinned, _ = measured(small, S, 0, lambda sp, xs: sp.process_host_into(pinned_x, small.pinned_empty((S, F, 2), np.float32)))
    assert np.array_equal(pinned, one)
    for run in (lambda sp, xs: host_call(sp, xs, S16), lambda sp, xs: device_call(torch, sp, xs, S16)):
        for c in (ctx, small):
            got, _ = measured(c, S, 0, run)
            assert np.array_equal(got, one)
    shards = [measured(ctx, k, first, lambda sp, xs: device_call(torch, sp, xs))[0] for first, k in ((0, 1), (1, 2), (3, 2))]
    assert np.array_equal(np.concatenate(shards), one)
    # A timeline split at 4411 frames changes the hop energies by Float64 summation order only — of the SAME float32 output.  The
    # convolution kernels themselves round differently when a call is split (other windows: on this shape the two outputs differ by
    # 1e-7 of the peak, and the hop energies of the two runs by 2.4e-8), so the split run is held to the bound against the recurrence
    # over the output IT wrote, which asks more than agreement with the other run; against the one-call run it is held to the bound
    # wherever the two outputs are the same bits.
    sp = real_spatializer(aw, ctx, oracle, S)
    sp.set_loudness(True, 1.0)
    y_split = np.concatenate([device_call(torch, sp, x[:, :4411]), device_call(torch, sp, x[:, 4411:])], axis=1)
    split = all_hops(sp, n)
    same_y = np.array_equal(y_split, kept["y"])
    dy = float(np.max(np.abs(y_split.astype(np.float64) - kept["y"])) / np.max(np.abs(kept["y"])))
    err_runs = float(np.max(np.abs(split - one) / one))
    want_hops, _ = reference_hops(y_split, RATE)
    err = float(np.max(np.abs(split[:, : want_hops.shape[1]] - want_hops) / want_hops))
    print(f"timeline split at 4411: outputs identical {same_y} (largest difference {dy:.3e} of the peak); hop energies: {err:.3e} from the "
          f"recurrence over the split run's output, {err_runs:.3e} from the one-call run (bound {BOUND:.3e})")
    assert err <= BOUND
    assert err_runs <= BOUND or not same_y
    ld = sp.loudness()
    assert np.all(ld["frames"] == F) and np.all(ld["blocks"] == F // (RATE // 10) - 3)


def test_single_stream_callback_path_is_measured():
    """One stream, callback-sized calls of the host entry: the kernels write page-locked memory, and the loudness kernels read it."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    calls = [4096, 4096, 1023, 4096, 31]
    x = np.random.default_rng(54).uniform(-0.5, 0.5, (1, sum(calls), 2)).astype(np.float32)
    sp = delta_spatializer(aw, ctx, 44100, 1)
    sp.reserve_host(4096)
    sp.set_loudness(True, 1.0)
    ys, at = [], 0
    for c in calls:
        ys.append(host_call(sp, x[:, at:at + c]))
        at += c
    assert sp.info()["host_chunk_streams"] == 0
    y = np.concatenate(ys, axis=1)
    want_hops, _ = reference_hops(y, 44100)
    n = want_hops.shape[1]
    assert n == 3
    err = float(np.max(np.abs(all_hops(sp, n) - want_hops) / want_hops))
    print(f"callback path: relative error of the hop energies {err:.3e}")
    assert err <= BOUND and sp.loudness()["frames"][0] == sum(calls)


# ---- 4. off means off -----------------------------------------------------------------------------------------------------------------

def test_outputs_do_not_depend_on_the_measurement(oracle):
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    x = np.random.default_rng(55).uniform(-0.5, 0.5, (3, 20011, 7)).astype(np.float32)
    for fout in (F32, S16):
        plain, measured = real_spatializer(aw, ctx, oracle, 3), real_spatializer(aw, ctx, oracle, 3)
        measured.set_loudness(True, 1.0)
        assert plain.info()["loudness"] == 0 and measured.info()["loudness"] == 1
        for run in (lambda sp: device_call(torch, sp, x, fout), lambda sp: host_call(sp, x, fout)):
            a, b = run(plain), run(measured)
            assert a.tobytes() == b.tobytes()
        allocs = measured.info()["device_allocs"]
        measured.set_loudness(False)
        measured.set_loudness(True, 1.0)                              # the same capacity: the records and the allocation stay
        assert measured.info()["device_allocs"] == allocs and measured.loudness()["frames"][0] == 2 * 20011


# ---- 5. capacity, reset, non-finite samples ---------------------------------------------------------------------------------------------

def test_capacity_reset_and_nonfinite():
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    F = RATE + RATE // 2
    x = np.random.default_rng(56).uniform(-0.5, 0.5, (2, F, 2)).astype(np.float32)
    x[1] *= np.float32(0.05)
    sp = delta_spatializer(aw, ctx, RATE, 2)
    sp.set_loudness(True, 1.0)
    y = host_call(sp, x)
    want_hops, _ = reference_hops(y, RATE)
    ld = sp.loudness()
    assert np.all(ld["frames"] == F) and np.all(ld["frames_dropped"] == RATE // 2)
    check_against_reference(ld, all_hops(sp, 10), want_hops[:, :10], RATE, "capacity of 1 s")      # the first 10 hops only
    assert np.all(ld["blocks"] == 7)
    with pytest.raises(aw.AirwaveError):
        sp.loudness_hops(0, 0, 11)
    sp.reset_levels()
    ld = sp.loudness()
    assert not all_hops(sp, 10).any() and not ld["frames"].any() and not ld["blocks"].any() and np.all(np.isneginf(ld["integrated_lufs"]))
    y2 = host_call(sp, x[:, : RATE // 2])                            # the filter state and the frame count started over too
    want2, _ = reference_hops(y2, RATE)
    assert float(np.max(np.abs(all_hops(sp, 5) - want2) / want2)) <= BOUND and sp.loudness()["frames_dropped"][0] == 0
    sp.reset()
    assert not all_hops(sp, 10).any() and sp.loudness()["frames"][0] == 0
    # a NaN: whatever the convolution makes of it in y is counted and enters the filters as 0; the hops after it are the reference's
    sp = delta_spatializer(aw, ctx, RATE, 2)
    sp.set_loudness(True, 2.0)
    xn = x.copy()
    xn[0, 20000, 1] = np.nan
    yn = host_call(sp, xn)
    want_hops, want_bad = reference_hops(yn, RATE)
    ld = sp.loudness()
    assert want_bad[0] > 0 and want_bad[1] == 0 and np.array_equal(ld["nonfinite"].astype(np.int64), want_bad)
    assert np.isfinite(yn[0, -RATE // 2:]).all()
    # (hops that hold non-finite samples may be nothing but the filters' decay after the last finite sample: compared through the
    # loudness and the counts only; every other hop, the later ones among them, within the bound)
    holed = ~np.isfinite(yn).all(axis=2)[:, : 15 * (RATE // 10)].reshape(2, 15, RATE // 10).all(axis=2)
    assert holed[0].any() and not holed[0, -5:].any() and not holed[1].any()
    check_against_reference(ld, all_hops(sp, 15), want_hops, RATE, "NaN frame", skip=holed)


# ---- 6. another capacity on a live handle ------------------------------------------------------------------------------------------------

def test_another_capacity_on_a_live_handle_makes_new_empty_records(oracle):
    """aw_spatializer_set_loudness with another max_seconds on a handle that has measured: the stream goes idle, the old records are
    freed, new ones of the new capacity are made, and the measurement starts over (filter state and frame count too)."""
    import torch
    import airwave_amd as aw
    ctx = context(aw, torch)
    rate, hop = 10000, 1000
    h = oracle.synth_hrir(2, 64, seed=57)
    lt, rt = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    sp = aw.Spatializer(aw.HRIR(h, sample_rate=float(rate), ctx=ctx), lt, rt, n_streams=2, ctx=ctx)
    x = np.random.default_rng(57).uniform(-0.5, 0.5, (2, 4000, 2)).astype(np.float32)
    allocs = sp.info()["device_allocs"]
    sp.set_loudness(True, 0.1)                                         # one hop per stream
    y1 = host_call(sp, x[:, :1000])
    want1, _ = reference_hops(y1, rate)
    assert want1.shape == (2, 1) and np.all(sp.loudness()["frames"] == 1000)
    check_against_reference(sp.loudness(), all_hops(sp, 1), want1, rate, "capacity of one hop")
    with pytest.raises(aw.AirwaveError):
        sp.loudness_hops(0, 0, 2)
    sp.set_loudness(True, 0.5)                                         # five hops: new records, nothing measured yet
    assert sp.info()["loudness"] == 1 and not sp.loudness()["frames"].any() and not all_hops(sp, 5).any()
    y2 = host_call(sp, x[:, 1000:])
    want2, _ = reference_hops(y2, rate)                                # (from silent filters: the state started over with the records)
    ld = sp.loudness()
    assert want2.shape == (2, 3) and np.all(ld["frames"] == 3000) and not ld["frames_dropped"].any() and not ld["nonfinite"].any()
    check_against_reference(ld, all_hops(sp, 5), want2, rate, "capacity of five hops")
    assert not all_hops(sp, 5)[:, 3:].any()
    y = np.concatenate([y1, y2], axis=1)
    for s in range(2):
        assert oracle.peak_rel_error(y[s], oracle.spatialize_f64(x[s], h, lt, rt)) < 1e-5
    delta = sp.info()["device_allocs"] - allocs
    print(f"device allocations of the sequence: {delta}")
    # Measured once on the library as it was before the buffers got an owning type (not derived from the new code): the records twice,
    # the float staging in and out for 1000 frames and again for 3000.
    assert delta == 6
