"""TEST-ONLY: three instruments that resolve a convolution error by frequency band and by HRIR tap (test_spectral_ref.py,
test_emu_spectral.py, test_gpu_spectral.py).  White noise through a decaying HRIR under `peak_rel_error` spreads a fault over every bin and
every tap and then takes one maximum: a filter-table entry wrong to three digits stays under 1e-5, a dropped last tap of a long HRIR lands at
about 1e-5, on either side of it.

  band_rel_error   the error's Welch spectrum against the reference's MEAN band power: one wrong bin stands out of the rounding floor
  tones            inputs whose whole energy sits on chosen bins of the kernel's transform: one wrong bin is the whole answer
  end_heavy_hrir   an HRIR whose last taps carry the energy: a lost tap is a gross error under the existing measure
  direct_hrir      an HRIR with a unit first tap, so that a tone does not fall into a spectral null of the noise

Nothing here calls the code under test."""
import numpy as np

TOL = 1e-5          # north star: <= 1e-5 of peak — here per band as well as per call
TONE_AMPLITUDE = 0.4


def _segments(v, L):
    """[n_seg][L] float64: Hann segments of length L, hop L/2, over the whole of v (zero fill behind its end, so that every sample is in)."""
    v = np.asarray(v, np.float64)
    hop = L // 2
    n_seg = max(1, -(-(v.size - L) // hop) + 1)
    pad = np.zeros((n_seg - 1) * hop + L)
    pad[:v.size] = v
    idx = np.arange(L)[None, :] + hop * np.arange(n_seg)[:, None]
    return pad[idx] * np.hanning(L + 1)[:L]            # the periodic window


def band_rel_error(y, ref, L):
    """One ear: sqrt(max_f PE[f] / mean_f PR[f]) and the arg-max bin, PE / PR = |rfft|^2 of the Hann segments of y - ref / of ref, summed
    over the segments.  The denominator is the reference's MEAN band power, not PR[f]: a random HRIR has deep nulls, where rounding noise
    (white) would dominate a bin-by-bin ratio."""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    assert y.ndim == 1 and y.shape == ref.shape and L % 2 == 0
    pe = (np.abs(np.fft.rfft(_segments(y - ref, L), axis=1)) ** 2).sum(axis=0)
    pr = (np.abs(np.fft.rfft(_segments(ref, L), axis=1)) ** 2).sum(axis=0)
    f = int(np.argmax(pe))
    return float(np.sqrt(pe[f] / pr.mean())), f


def segment_length(frames, L):
    """L for calls of at least 2 L frames, else the largest power of two of which the call holds two: a single zero-filled segment would put a short
    call on the window's rising flank, its first frames at almost no weight."""
    while 2 * L > frames and L > 256:
        L //= 2
    return L


def worst_band(y, ref, L):
    """(error, bin, ear) of the worse ear of y, ref: [frames][2]; segments of segment_length(frames, L)."""
    L = segment_length(y.shape[0], L)
    return max((*band_rel_error(y[:, ear], ref[:, ear], L), ear) for ear in range(2))


def tone_phase(channel, tone):
    """Phase of one tone of one channel, within +-pi/4: different per channel and per tone, and a constant (k = 0) or an alternation
    (k = N/2), which keep only the cosine part, stay above 0.7 of their amplitude."""
    return (np.pi / 4) * (2.0 * ((0.37 * channel + 0.61 * tone + 0.13) % 1.0) - 1.0)


def tones(frames, channels, N, bins, half=False):
    """[frames][channels] float32: every channel the sum of cosines at k/N cycles per sample, k in bins ((k + 1/2)/N with half), total
    amplitude 0.4.  k = 0 is a constant, k = N/2 a +-alternation.  The phase advance is reduced in integers: exact at any frame index."""
    bins = list(bins)
    n = np.arange(frames, dtype=np.int64)
    x = np.zeros((frames, channels), np.float64)
    for c in range(channels):
        for i, k in enumerate(bins):
            turn = ((2 * k + 1) * n) % (2 * N) / (2.0 * N) if half else (k * n) % N / float(N)
            x[:, c] += np.cos(2.0 * np.pi * turn + tone_phase(c, i))
    return (x * (TONE_AMPLITUDE / len(bins))).astype(np.float32)


def end_heavy_hrir(oracle, tracks, taps, seed):
    """synth_hrir with an envelope that RISES by e^6 towards the last tap."""
    return oracle.synth_hrir(tracks, taps, seed, tau=-taps / 6.0)


def direct_hrir(oracle, tracks, taps, seed):
    """synth_hrir with tap 0 of every track set to 1.0 before renormalising to unit energy."""
    h = oracle.synth_hrir(tracks, taps, seed).astype(np.float64)
    h[:, 0] = 1.0
    h /= np.sqrt((h ** 2).sum(axis=1, keepdims=True))
    return h.astype(np.float32)


def maps(channels):
    """Channel -> (left, right) track of a 14-track HRIR, every channel on tracks of its own where 14 tracks allow it."""
    lt = (np.arange(channels) % 14).astype(np.int32)
    rt = ((np.arange(channels) * 3 + 7) % 14).astype(np.int32)
    return lt, rt
