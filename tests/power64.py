"""Float64 restatements of the passes that follow the FFT in psa_dynamic_spectra, psa_lattice_spectra and psa_self_spectra,
on transformed segments taken as given (the inputs of psa_debug_dynamic_power, psa_debug_lattice_shell and
psa_debug_self_power), with the quantities the bars of tests/power_cases.py are relative to.  NumPy only; every float32
input is widened first and nothing is rounded on the way.

    density       = scale sum_s |F_0|^2
    longitudinal  = scale sum_s |h.F|^2                  h = k / |k| in float64 from the float32 k (k = 0: h = 0)
    transverse    = scale 1/2 sum_s sum_c |F_c - h_c (h.F)|^2
    A = sum_s sum_c |F_c|^2     P = sum_s sum_c |F_c - h_c (h.F)|^2     LAM = sum_s (sum_c |h_c| |F_c|)^2

The shell form adds, per vector, the term read at the mirrored frequency (L - o) mod L -- the partner -n of a half-space
member -- sums over the vectors of a bin and scales by 1 / (2 n_b norm); the self form sums |Z|^2 over atoms, segments and a
column's vectors, with the mirror term in the shell form."""
import numpy as np


def khat64(k_vectors):
    """k / |k| in float64 from float32 k (K, 3); a zero vector gives zeros"""
    k = np.asarray(k_vectors, np.float32).astype(np.float64).reshape(-1, 3)
    norm = np.sqrt(np.sum(k * k, axis=1, keepdims=True))
    return np.divide(k, norm, out=np.zeros_like(k), where=norm > 0)


def _sq(z):
    """|z|^2 without a square root: exact for Gaussian integers"""
    return z.real ** 2 + z.imag ** 2


def _parts(seg, h):
    """per (vector, segment, frequency): |F_0|^2, |h.F|^2, sum_c |F_perp,c|^2, sum_c |F_c|^2, (sum_c |h_c| |F_c|)^2; the last
    four are None without currents"""
    S = np.asarray(seg).astype(np.complex128)
    den = _sq(S[:, 0])
    if S.shape[1] == 1:
        return den, None, None, None, None
    F = S[:, 1:4]                                                          # (K, 3, ns, L)
    hh = h[:, :, None, None]
    p = np.sum(hh * F, axis=1)                                             # (K, ns, L)
    perp = F - hh * p[:, None]
    return (den, _sq(p), np.sum(_sq(perp), axis=1), np.sum(_sq(F), axis=1),
            np.sum(np.abs(hh) * np.abs(F), axis=1) ** 2)


def dynamic64(seg, k_vectors, scale):
    """seg (K, NC, ns, L) complex64 -> dict: out (1 or 3, L, K) float64 and A, P, LAM (L, K) (None without currents)"""
    den, lon, perp, a, lam = _parts(seg, khat64(k_vectors))
    sc = float(np.float32(scale))
    red = lambda x: None if x is None else np.sum(x, axis=1).T             # (L, K)
    rows = [sc * red(den)]
    if lon is not None:
        rows += [sc * red(lon), sc * 0.5 * red(perp)]
    return dict(out=np.stack(rows), A=red(a), P=red(perp), LAM=red(lam), scale=sc)


def _mirror(x):
    """x[..., (L - o) mod L]"""
    L = x.shape[-1]
    return x[..., (L - np.arange(L)) % L]


def shell64(seg, k_vectors, bin_of, n_bins, norm):
    """the shell form: dict with out (1 or 3, L, n_bins) float64, A, P, LAM (L, n_bins) sums over both sides, the bin's vectors
    and the segments, and scale (n_bins,) (an empty bin: 0)"""
    bins = np.asarray(bin_of)
    parts = _parts(seg, khat64(k_vectors))
    count = np.bincount(bins, minlength=n_bins).astype(np.float64)
    scale = np.divide(1.0, 2.0 * count * float(norm), out=np.zeros(n_bins), where=count > 0)

    def red(x):
        if x is None:
            return None
        both = np.sum(x + _mirror(x), axis=1)                              # (K, L)
        out = np.zeros((x.shape[-1], n_bins))
        np.add.at(out.T, bins, both)
        return out
    den, lon, perp, a, lam = (red(x) for x in parts)
    rows = [scale * den]
    if lon is not None:
        rows += [scale * lon, scale * 0.5 * perp]
    return dict(out=np.stack(rows), A=a, P=perp, LAM=lam, scale=scale)


def self64(work, groups, cols, scale, mirror):
    """work (na, nv, ns, L) complex64; groups (n_groups + 1, 2) = (first vector, column) -> (L, cols) float64"""
    Z = _sq(np.asarray(work).astype(np.complex128))
    if mirror:
        Z = Z + _mirror(Z)
    per_v = np.sum(Z, axis=(0, 2))                                         # (nv, L)
    g = np.asarray(groups).reshape(-1, 2)
    out = np.zeros((Z.shape[-1], cols))
    for i in range(g.shape[0] - 1):
        out[:, g[i, 1]] = np.sum(per_v[g[i, 0]:g[i + 1, 0]], axis=0)
    return out * np.asarray(scale, np.float64)[None, :]
