"""Numpy restatement of the true-peak rule of airwave_amd/csrc/device/truepeak.hpp (aw_stream_true_peak): the 49-tap Hann-windowed sinc
in float64, its three computed phases, and the windows of a signal evaluated in float64 — with the formula's own coefficients or with the
float32 coefficients the library reports (aw_true_peak_filter) — next to the error bound of the float32 evaluation: twelve correctly
rounded operations give |t - t_ref| <= 12 * 2^-24 * sum_k |c[p][k]| |v[n-k]| per window."""
import numpy as np

TAPS, PHASES, HISTORY = 12, 3, 11
EPS = 12.0 * 2.0 ** -24


def prototype():
    """h[0 .. 48] in float64."""
    j = np.arange(49, dtype=np.float64)
    return np.sinc((j - 24.0) / 4.0) * (0.5 - 0.5 * np.cos(2.0 * np.pi * j / 48.0))


def coefficients():
    """c[p - 1][k] = h[p + 4k], p = 1 .. 3, float64 [3][12]."""
    h = prototype()
    return np.stack([h[p + 4 * np.arange(TAPS)] for p in (1, 2, 3)])


def sanitize(y):
    """(v, count): y as float64 with NaN / inf replaced by 0, and how many there were."""
    y = np.asarray(y, np.float32)
    bad = ~np.isfinite(y)
    return np.where(bad, np.float32(0), y).astype(np.float64), int(bad.sum())


def measure(y, c, hist=None):
    """y: [frames][2] float32, continuing a stream whose last 11 cleaned frames are hist [11][2] (default: silence); c: [3][12].
    Returns a dict: peak [2] (float64: max over frames of |v|, |t_1|, |t_2|, |t_3|), bound [2] (the largest per-window error bound of
    the float32 evaluation), nonfinite, hist (the next call's)."""
    v, bad = sanitize(y)
    frames = v.shape[0]
    c = np.asarray(c, np.float64)
    h = np.zeros((HISTORY, 2)) if hist is None else np.asarray(hist, np.float64)
    ext = np.concatenate([h, v])
    peak, bound = np.zeros(2), np.zeros(2)
    for at in range(0, frames, 1 << 16):                      # (bounded memory)
        n = np.arange(at, min(frames, at + (1 << 16)))
        w = ext[n[:, None] + HISTORY - np.arange(TAPS)[None, :]]              # w[n][k][ear] = v[n - k]
        t = np.einsum("pk,nke->npe", c, w)
        e = EPS * np.einsum("pk,nke->npe", np.abs(c), np.abs(w))
        peak = np.maximum(peak, np.maximum(np.abs(t).max(axis=(0, 1)), np.abs(w[:, 0]).max(axis=0)))
        bound = np.maximum(bound, e.max(axis=(0, 1)))
    return {"peak": peak, "bound": bound, "nonfinite": bad, "hist": ext[-HISTORY:].copy()}


def db(x):
    return 20.0 * np.log10(x)


def faded_sine(rate, freq, phase_deg, amplitude, seconds=0.1, fade=0.01):
    """[frames][2] float32: a stereo sine with a raised-cosine fade in and out (an abrupt start overshoots legitimately)."""
    n = np.arange(int(round(seconds * rate)), dtype=np.float64)
    f = int(round(fade * rate))
    env = np.ones(n.size)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(f) + 0.5) / f)
    env[:f], env[-f:] = ramp, ramp[::-1]
    s = (amplitude * env * np.sin(2.0 * np.pi * freq / rate * n + np.deg2rad(phase_deg))).astype(np.float32)
    return np.stack([s, s], axis=1)
