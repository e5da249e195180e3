"""TEST-ONLY: the float64 reference of the loudness tests (test_loudness_host.py, test_emu_loudness.py, test_gpu_loudness.py,
test_example_loudness.py): ITU-R BS.1770-4 restated in numpy — the K-weighting coefficients from the analog prototypes, the sequential
transposed-direct-form-II recurrence, `reshape` hop sums and the gating.  Nothing here calls the code under test."""
import numpy as np

# ITU-R BS.1770-4, table 1 and 2 (48 kHz): b0 b1 b2 a0 a1 a2 of the shelf and of the high-pass
BS1770_TABLE = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                         [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])
SHELF_F0, SHELF_G, SHELF_Q, SHELF_EXP = 1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416
HP_F0, HP_Q = 38.13547087602444, 0.5003270373238773


def k_coefficients(fs):
    """[2][6]: b0 b1 b2 a0 a1 a2 (a0 = 1) of the shelf and the high-pass at fs, bilinear transform with K = tan(pi f0 / fs)."""
    K = np.tan(np.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_G / 20.0)
    Vb = Vh ** SHELF_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = [(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0, 1.0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0]
    K = np.tan(np.pi * HP_F0 / fs)
    a0 = 1.0 + K / HP_Q + K * K
    hp = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HP_Q + K * K) / a0]
    return np.array([shelf, hp], np.float64)


def sanitize(y):
    """(float64 copy with NaN / inf replaced by 0, the count of those)."""
    y = np.asarray(y, np.float64)
    bad = ~np.isfinite(y)
    return np.where(bad, 0.0, y), int(np.count_nonzero(bad))


def k_weight_loop(y, fs, state=None):
    """The sequential recurrence, frame by frame: y [..., frames] float64 (any leading axes run side by side).  state: [2][2][...] carried
    in and out (None: zeros).  Returns (k, state)."""
    c = k_coefficients(fs)
    v = np.array(y, np.float64)
    lead = v.shape[:-1]
    st = np.zeros((2, 2) + lead) if state is None else np.array(state, np.float64)
    for k in range(2):
        b0, b1, b2, _, a1, a2 = c[k]
        z1, z2 = st[k, 0].copy(), st[k, 1].copy()
        out = np.empty_like(v)
        for f in range(v.shape[-1]):
            x = v[..., f]
            lo = b0 * x + z1
            z1 = b1 * x - a1 * lo + z2
            z2 = b2 * x - a2 * lo
            out[..., f] = lo
        st[k, 0], st[k, 1] = z1, z2
        v = out
    return v, st


def k_weight(y, fs):
    """The same recurrence over long signals through scipy.signal.lfilter (float64 transposed direct form II, the loop above:
    test_loudness_host.py checks that the two agree), from a zero state: y [..., frames] -> k."""
    from scipy.signal import lfilter
    c = k_coefficients(fs)
    v = np.asarray(y, np.float64)
    for k in range(2):
        v = lfilter(c[k, :3], c[k, 3:], v, axis=-1)
    return v


def hop_energies(k_left, k_right, hop):
    """E[h] over the complete hops of one stream's K-weighted ears."""
    n = (k_left.shape[-1] // hop) * hop
    sq = k_left[:n] ** 2 + k_right[:n] ** 2
    return sq.reshape(-1, hop).sum(axis=1)


def block_loudness(e, hop):
    """(z_j, l_j) of the 400 ms blocks over the complete hops e."""
    e = np.asarray(e, np.float64)
    if e.size < 4:
        return np.zeros(0), np.zeros(0)
    z = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * hop)
    with np.errstate(divide="ignore"):
        return z, -0.691 + 10.0 * np.log10(z)


def gate(e, hop):
    """dict(integrated, relative_threshold, blocks, above_absolute, gated) of the hop energies e."""
    z, l = block_loudness(e, hop)
    r = {"integrated": -np.inf, "relative_threshold": -np.inf, "blocks": int(z.size), "above_absolute": 0, "gated": 0}
    keep = l > -70.0
    r["above_absolute"] = int(keep.sum())
    if not keep.any():
        return r
    r["relative_threshold"] = -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
    keep2 = keep & (l > r["relative_threshold"])
    r["gated"] = int(keep2.sum())
    if keep2.any():
        r["integrated"] = -0.691 + 10.0 * np.log10(z[keep2].mean())
    return r


def measure(y, fs):
    """y: [frames][2] -> gate() of its loudness, plus 'hops' and 'nonfinite'."""
    hop = int(round(fs / 10))
    v, bad = sanitize(y)
    k = k_weight(v.T, fs)
    e = hop_energies(k[0], k[1], hop)
    r = gate(e, hop)
    r["hops"], r["nonfinite"] = e, bad
    return r
