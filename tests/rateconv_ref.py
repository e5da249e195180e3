"""Numpy restatement of the sample-rate converter's rule of airwave_amd/csrc/device/rateconv.hpp (aw_rateconv_*): the plan of a pair of
rates, the Kaiser-windowed sinc in float64 with np.i0, the outputs of a signal evaluated in float64 — with the formula's own coefficients
or with the float32 table the library reports (aw_rateconv_filter) — next to the error bound of the float32 evaluation: T correctly
rounded operations give |y - y_ref| <= T * 2^-24 * sum_k |c[p][k]| |x[i + D - k]| per sample."""
from math import gcd

import numpy as np

Z, BETA, MAX_TERM = 48, 10.0, 640


def plan(in_rate, out_rate):
    """(L, M, T, D) of a pair of integer rates; ValueError where the library refuses."""
    if in_rate != int(in_rate) or out_rate != int(out_rate) or in_rate <= 0 or out_rate <= 0:
        raise ValueError("rates must be positive integers")
    a, b = int(in_rate), int(out_rate)
    if a == b:
        raise ValueError("equal rates")
    g = gcd(a, b)
    L, M = b // g, a // g
    if max(L, M) > MAX_TERM:
        raise ValueError("a reduced term above 640")
    D = -(-Z * M // L) if M > L else Z           # ceil(Z / rho)
    return L, M, 2 * D, D


def coefficients(L, M):
    """c[p][k] = h(k - D + p / L) in float64, [L][T]."""
    rho = min(1.0, L / M)
    W = Z / rho
    D = -(-Z * M // L) if M > L else Z
    A =BETA / 0.1102 + 8.7
    delta = (A - 7.95) / (14.36 * 2 * Z)
    fc = 0.5 - delta / 2.0
    t = (np.arange(2 * D, dtype=np.float64) - D)[None, :] + (np.arange(L, dtype=np.float64) / L)[:, None]
    inside = np.abs(t) <= W
    u = np.where(inside, t / W, 0.0)
    h = 2.0 * fc * rho * np.sinc(2.0 * fc * rho * t) * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(BETA)
    return np.where(inside, h, 0.0)


def output_count(n_in, L, M, D, flushed=False):
    """Outputs that exist after n_in input frames: max(0, ceil((N - D) L / M)); flushed: ceil(N L / M)."""
    n = n_in + D if flushed else n_in
    return max(0, -((n - D) * L // -M))


def _windows(x, L, M, D, c, n0, n1):
    """(c rows [n][T], x windows [n][T][C]) of the outputs n0 .. n1 - 1; x [N][C] with zeros outside."""
    T = c.shape[1]
    n = np.arange(n0, n1, dtype=np.int64)
    i, p = n * M // L, n * M % L
    at = i[:, None] + D - np.arange(T, dtype=np.int64)[None, :]                     # input frame of tap k
    ok = (at >= 0) & (at < x.shape[0])
    w = np.where(ok[:, :, None], x[np.clip(at, 0, max(x.shape[0] - 1, 0))], 0.0)
    return c[p], w


def convert64(x, L, M, D, c, flushed=False, with_bound=False):
    """The float64 evaluation of one stream: x [N][C] -> y [n_out][C], over the whole stream from a reset (flushed: D zero frames behind
    it).  c: [L][T], float64 or the library's float32 table.  with_bound: also the per-sample bound of the float32 evaluation."""
    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    T = c.shape[1]
    n_out = output_count(x.shape[0], L, M, D, flushed)
    y = np.zeros((n_out, x.shape[1]))
    b = np.zeros_like(y)
    for at in range(0, n_out, 1 << 12):                      # (bounded memory)
        end = min(n_out, at + (1 << 12))
        rows, w = _windows(x, L, M, D, c, at, end)
        y[at:end] = np.einsum("nk,nkc->nc", rows, w)
        if with_bound:
            b[at:end] = T * 2.0 ** -24 * np.einsum("nk,nkc->nc", np.abs(rows), np.abs(w))
    return (y, b) if with_bound else y
