"""The instruments of spectral_ref.py are themselves sharp, and the measure the suite had is not: faults injected into a plain float64 numpy
convolution (no kernel runs here).  A filter bin wrong by 1e-4 passes `peak_rel_error < 1e-5` on white noise through a decaying HRIR, and the
last tap of a 32768-tap HRIR dropped lands on either side of it by the luck of one draw; the per-band measure, a tone on the bin and an end-heavy
HRIR see them clearly."""
import numpy as np
import pytest
import scipy.fft

import spectral_cases as sc
import spectral_ref as sr
from spectral_ref import TOL

N, TAPS, HOP, BIN = 8192, 4320, 3840, 1234


def _overlap_save(x, h, scale_bin=None, scale=1.0):
    """float64 overlap-save of one channel through one track, N-point windows every HOP frames; scale_bin: that bin of the filter's spectrum
    and its mirror times `scale`."""
    H = np.fft.fft(np.asarray(h, np.float64), N)
    if scale_bin is not None:
        H[scale_bin] *= scale
        H[N - scale_bin] *= scale
    hist = N - HOP
    xp = np.concatenate([np.zeros(hist), np.asarray(x, np.float64), np.zeros(HOP)])
    out = np.empty(x.size + HOP)
    for t in range(0, x.size, HOP):
        out[t:t + HOP] = np.fft.ifft(np.fft.fft(xp[t:t + N]) * H).real[hist:]
    return out[:x.size]


@pytest.fixture(scope="module")
def noise(oracle):
    x = oracle.synth_input(1, 30000, 1)[0, :, 0]
    h = oracle.synth_hrir(1, TAPS)[0]
    return x, h, oracle.direct_conv_f64(x, h)


def test_the_plain_overlap_save_is_exact(oracle, noise):
    x, h, ref = noise
    y = _overlap_save(x, h)
    assert oracle.peak_rel_error(y, ref) < 1e-12
    assert sr.band_rel_error(y, ref, N)[0] < 1e-12


def test_one_filter_bin_wrong_by_1e_4_passes_the_peak_measure_and_fails_the_band_measure(oracle, noise):
    x, h, ref = noise
    y = _overlap_save(x, h, BIN, 1.0 + 1e-4)
    assert oracle.peak_rel_error(y, ref) < TOL                 # the blind spot
    err, f = sr.band_rel_error(y, ref, N)
    assert err > TOL and abs(f - BIN) <= 2, (err, f)


def test_a_tone_on_the_wrong_bin_fails_the_peak_measure(oracle, noise):
    _, h, _ = noise
    x = sr.tones(30000, 1, N, [BIN])[:, 0]
    ref = oracle.direct_conv_f64(x, h)
    assert np.max(np.abs(ref)) >= 0.2 * sr.TONE_AMPLITUDE
    assert oracle.peak_rel_error(_overlap_save(x, h), ref) < 1e-12
    assert oracle.peak_rel_error(_overlap_save(x, h, BIN, 1.0 + 1e-3), ref) > TOL


def test_tones_are_what_they_say(oracle):
    x = sr.tones(4 * N, 3, N, [0]).astype(np.float64)
    assert np.all(x == x[:1]) and np.all(np.abs(x[0]) >= 0.7 * sr.TONE_AMPLITUDE * (1 - 1e-6))           # k = 0: a constant
    x = sr.tones(4 * N, 3, N, [N // 2]).astype(np.float64)
    assert np.all(x[1:] == -x[:-1]) and np.all(np.abs(x[0]) >= 0.7 * sr.TONE_AMPLITUDE * (1 - 1e-6))     # k = N/2: +-alternation
    for half in (False, True):
        x = sr.tones(2 * N, 2, N, [15, 513], half).astype(np.float64)
        assert np.max(np.abs(x)) <= sr.TONE_AMPLITUDE * (1 + 1e-6)
        spec = np.abs(np.fft.fft(x[:2 * N, 0]))                # 2N points: bin 2k (+1 with half)
        top = sorted(int(i) for i in np.argsort(spec[:N])[-2:])
        assert top == [2 * 15 + half, 2 * 513 + half], top
        assert not np.array_equal(x[:, 0], x[:, 1])            # another phase per channel
    assert sr.tones(100, 2, N, [7]).dtype == np.float32


def test_a_dropped_last_tap_passes_with_the_decaying_envelope_and_fails_with_the_end_heavy_one(oracle):
    """One channel through each of the 14 tracks of a 32768-tap HRIR, the track's last tap lost.

    This differs from the issue on purpose.  The issue says `peak_rel_error` is below TOL with the decaying envelope and above 100 TOL with the
    end-heavy one.  That premise depended on which random tap was drawn: the lost tap is one normal draw (times e^-6 of the first tap's scale under
    the decaying envelope), and over these 14 tracks 8 decaying ones are ABOVE TOL (4e-7 .. 4e-5) and 3 end-heavy ones are below 1e-3
    (1.5e-4 .. 1.6e-2).  So the existing measure neither reliably sees nor reliably misses the fault, and this weaker form is the honest one:
    some decaying tracks pass and none fails by a clear margin (all under 10 TOL); the same draw under the end-heavy envelope is more than 100 times
    larger for every track, its median above 100 TOL; and the strict bound of the issue, above 100 TOL, is asserted where seven lost taps add up, on
    the 7-speaker downmix.  No bound of a kernel test hangs on this: those assert `< TOL` throughout."""
    x = oracle.synth_input(1, 40000, 1)[0, :, 0]
    errs = {}
    for name, h in (("decaying", oracle.synth_hrir(14, 32768, seed=1234)), ("end-heavy", sr.end_heavy_hrir(oracle, 14, 32768, seed=1234))):
        errs[name] = [oracle.peak_rel_error(oracle.direct_conv_f64(x, t[:-1]), oracle.direct_conv_f64(x, t)) for t in h]
        print(name, " ".join(f"{e:.1e}" for e in errs[name]))
    assert min(errs["decaying"]) < TOL and max(errs["decaying"]) < 10 * TOL          # the blind spot: tracks pass, none fails by a clear margin
    assert all(e > 100 * d for e, d in zip(errs["end-heavy"], errs["decaying"]))     # the same draws under the other envelope
    assert np.median(errs["end-heavy"]) > 100 * TOL
    # the headline layout (7 speakers, both ears of each on tracks of their own): seven lost taps per ear
    lt, rt = np.array([0, 8, 6, 4, 12, 2, 10], np.int32), np.array([1, 7, 13, 5, 11, 3, 9], np.int32)
    x7 = oracle.synth_input(1, 40000, 7)[0]
    h = sr.end_heavy_hrir(oracle, 14, 32768, seed=1234)
    cut = h.copy()
    cut[:, -1] = 0.0
    ref = oracle.spatialize_f64(x7, h, lt, rt)
    for y, r in zip(oracle.spatialize_f64(x7, cut, lt, rt).T, ref.T):
        assert oracle.peak_rel_error(y, r) > 100 * TOL


def test_hrir_shapes(oracle):
    h = sr.end_heavy_hrir(oracle, 3, 6000, seed=5)
    assert h.dtype == np.float32 and h.shape == (3, 6000)
    assert np.allclose((h.astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-6)
    assert (h[:, -1000:].astype(np.float64) ** 2).sum() > 0.8 * 3          # the last sixth carries 1 - e^-2 of the energy
    d = sr.direct_hrir(oracle, 3, 6000, seed=5)
    assert np.allclose((d.astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-6)
    assert np.all(d[:, 0] > 0.65)                                          # 1 / sqrt(1 + the energy of the other taps)
    rest = oracle.synth_hrir(3, 6000, seed=5)
    assert np.allclose(d[:, 1:] / d[:, :1], rest[:, 1:], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("taps", [4320, 32768])
def test_the_float32_port_of_the_reference_stays_inside_the_band_bound(oracle, taps):
    """oracle.spatialize_f32 (512-frame uniform partitions in float32, the reference's arithmetic) against the float64 truth: the bound is
    not one that only float64 could meet."""
    h, lt, rt, x = sc.noise_input(oracle, "ols8192", 7, 1, 20011, taps=taps)
    y = oracle.spatialize_f32(x[0], h, lt, rt)
    ref = oracle.spatialize_f64(x[0], h, lt, rt)
    err, f, ear = sr.worst_band(y, ref, 8192)
    print(f"float32 port, {taps} taps: band_rel_error {err:.2e} at bin {f}")
    assert err < TOL, (err, f, ear)


def _downmix_f64(x, H, lt, rt, n):
    """float64 FFT convolution of x [frames][C] with the track spectra H [tracks][n/2 + 1], summed per ear: [2][frames]."""
    X = scipy.fft.rfft(x.astype(np.float64), n, axis=0, workers=4)
    return np.stack([scipy.fft.irfft(np.einsum("fc,cf->f", X, H[tr]), n)[:x.shape[0]] for tr in (lt, rt)])


def test_every_tone_comes_out_at_a_usable_level(oracle):
    """Every tone case of test_emu_spectral.py / test_gpu_spectral.py: the float64 reference's peak per ear is at least 0.2 of the input
    amplitude, or the case would measure rounding noise against a null.  Checked on the first frames of the timeline, never more than the
    shortest call that runs the case (the emulated one, FAMILIES[...].emu_frames): the peak only grows with more frames.  A case that fails
    here gets another seed in spectral_cases.tone()."""
    low, spectra = [], {}
    for t in sc.all_tones():
        taps = sc.FAMILIES[t.family].taps
        frames = min(taps + 4096, sc.FAMILIES[t.family].emu_frames)
        n = 1 << int(np.ceil(np.log2(frames + taps)))
        h, lt, rt, x = sc.tone_input(oracle, t, 2, frames)
        if (taps, t.seed) not in spectra:
            spectra[taps, t.seed] = np.fft.rfft(h.astype(np.float64), n, axis=1)
        for s in range(2):
            peak = np.max(np.abs(_downmix_f64(x[s], spectra[taps, t.seed], lt, rt, n)), axis=1)
            if peak.min() < 0.2 * sr.TONE_AMPLITUDE:
                low.append((sc.tone_id(t), s, peak.tolist()))
    assert not low, low


def test_the_fft_downmix_of_the_level_check_is_the_oracles_truth(oracle):
    t = sc.emu_tones("ols8192")[3]
    h, lt, rt, x = sc.tone_input(oracle, t, 1, 9000)
    y = _downmix_f64(x[0], np.fft.rfft(h.astype(np.float64), 16384, axis=1), lt, rt, 16384)
    assert oracle.peak_rel_error(y.T, oracle.spatialize_f64(x[0], h, lt, rt)) < 1e-12
