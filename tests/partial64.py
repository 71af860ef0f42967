"""A float64 restatement of the partial (species-resolved) spectra on the box's reciprocal lattice (psa_amd/partial.py,
psa_partial_spectra), for the host tests and the GPU parity tests.  It never calls the library.  NumPy only; every float32
input is widened first and nothing is rounded on the way.

    projection        per species, tests/lattice64.project64 on that species' atom list
    pair p = (a, b)   a <= b, row-major over the upper triangle
    density_ab        = scale sum_s Re F^a_0 conj F^b_0
    longitudinal_ab   = scale sum_s Re (h.F^a) conj (h.F^b)                  h = k / |k| in float64 (k = 0: h = 0)
    transverse_ab     = scale 1/2 sum_s sum_c Re F_perp,c^a conj F_perp,c^b     F_perp,c = F_c - h_c (h.F)

and what the bars of tests/partial_cases.py are relative to, each a sum over the segments (and, in the shell form, over
both sides and the bin's vectors) of products of the two species' moduli:

    D   = |F^a_0| |F^b_0|                                  LAM = (sum_c |h_c| |F^a_c|) (sum_c |h_c| |F^b_c|)
    A   = ||F^a|| ||F^b||     PP = ||F^a_perp|| ||F^b_perp||     M = ||F^a|| ||F^b_perp|| + ||F^a_perp|| ||F^b||

(||.||: the norm over the three components).  The shell form adds, per vector, the term read at the mirrored frequency
(L - o) mod L in BOTH factors -- the partner -n of a half-space member --, sums over a bin's vectors and scales by
1 / (2 n_b norm)."""
import numpy as np

import lattice64
from power64 import khat64

FIELDS = ("D", "LAM", "A", "PP", "M")


def pairs(n_species):
    """(P, 2) int: (0,0), (0,1), .., (0,S-1), (1,1), .."""
    return np.array([(a, b) for a in range(n_species) for b in range(a, n_species)], int)


def project64(positions, velocities, indices, inverse, species, weights=None, currents=True):
    """(K, S, NC, T) complex128: lattice64.project64 of every species' atom list (an empty list: zeros)"""
    return np.stack([lattice64.project64(positions, velocities, indices, inverse, np.asarray(g, np.int64), weights, currents)
                     for g in species], axis=1)


def _re(x, y):
    """Re x conj y without a complex product: exact for Gaussian integers"""
    return x.real * y.real + x.imag * y.imag


def _parts(seg, h):
    """seg (K, S, NC, ns, L), h (K, 3) float64 -> dict of (P, K, ns, L) float64: den, and with currents lon, tra (without its
    1/2) and the five fields the bars are relative to (without currents only D)"""
    Z = np.asarray(seg).astype(np.complex128)
    pr = pairs(Z.shape[1])
    a, b = pr[:, 0], pr[:, 1]
    F0 = np.moveaxis(Z[:, :, 0], 1, 0)                                     # (S, K, ns, L)
    out = dict(den=_re(F0[a], F0[b]), D=np.abs(F0[a]) * np.abs(F0[b]))
    if Z.shape[2] == 1:
        return out
    F = np.moveaxis(Z[:, :, 1:4], 1, 0)                                    # (S, K, 3, ns, L)
    hh = h[None, :, :, None, None]
    p = np.sum(hh * F, axis=2)                                             # (S, K, ns, L)
    perp = F - hh * p[:, :, None]
    norm = lambda x: np.sqrt(np.sum(x.real ** 2 + x.imag ** 2, axis=2))
    nF, nP, lam = norm(F), norm(perp), np.sum(np.abs(hh) * np.abs(F), axis=2)
    out.update(lon=_re(p[a], p[b]), tra=np.sum(_re(perp[a], perp[b]), axis=2), LAM=lam[a] * lam[b], A=nF[a] * nF[b],
               PP=nP[a] * nP[b], M=nF[a] * nP[b] + nP[a] * nF[b])
    return out


def _rows(parts, red, scale):
    rows = [scale * red(parts["den"])]
    if "lon" in parts:
        rows += [scale * red(parts["lon"]), scale * 0.5 * red(parts["tra"])]
    ref = dict(out=np.stack(rows), scale=scale)
    for f in FIELDS:
        ref[f] = red(parts[f]) if f in parts else None
    return ref


def vector64(seg, k_vectors, norm):
    """the per-vector form of transformed segments (K, S, NC, ns, L) complex64: dict with out (1 or 3, P, L, K) float64, the
    scale float32(1 / norm) as a float, and D, LAM, A, PP, M (P, L, K)"""
    sc = float(np.float32(1.0 / float(norm)))
    return _rows(_parts(seg, khat64(k_vectors)), lambda x: np.swapaxes(np.sum(x, axis=2), 1, 2), sc)


def _mirror(x):
    L = x.shape[-1]
    return x[..., (L - np.arange(L)) % L]


def shell64(seg, k_vectors, bin_of, n_bins, norm):
    """the shell form: out (1 or 3, P, L, n_bins) float64, the fields (P, L, n_bins) sums over both sides, the bin's vectors and
    the segments, scale (n_bins,) = 1 / (2 n_b norm) (an empty bin: 0)"""
    bins = np.asarray(bin_of)
    count = np.bincount(bins, minlength=n_bins).astype(np.float64)
    scale = np.divide(1.0, 2.0 * count * float(norm), out=np.zeros(n_bins), where=count > 0)

    def red(x):
        both = np.sum(x + _mirror(x), axis=2)                              # (P, K, L): the mirror of a product of mirrored factors
        out = np.zeros((x.shape[0], x.shape[-1], n_bins))
        for k, b in enumerate(bins):
            out[:, :, b] += both[:, k]
        return out
    return _rows(_parts(seg, khat64(k_vectors)), red, scale)


def transform64(q, window=None, L=None, H=None):
    """q (K, S, NC, T) complex128 -> (segments (K, S, NC, n_seg, L) = FFT(win q[s H : s H + L]) unscaled, norm = n_seg U L^2);
    no window: one boxcar segment of all frames"""
    T = q.shape[-1]
    if window is None:
        L, H, win = T, T, np.ones(T, np.float64)
    else:
        win = np.asarray(window, np.float32).astype(np.float64)
    n_seg = 1 + (T - L) // H
    seg = np.stack([np.fft.fft(win * q[..., s * H:s * H + L], axis=-1) for s in range(n_seg)], axis=3)
    return seg, n_seg * (float(np.dot(win, win)) / L) * float(L) ** 2


def spectra64(q, indices, inverse, window=None, L=None, H=None):
    """(density, longitudinal, transverse) per vector, each (P, L, K) float64 (the last two None for q of one series per
    species), of the projections q (K, S, NC, T): the definition, with k = n.G in float64"""
    seg, norm = transform64(q, window, L, H)
    parts = _parts(seg, khat64_exact(lattice64.lattice_k(indices, inverse)))
    red = lambda x: np.swapaxes(np.sum(x, axis=2), 1, 2) / norm
    if "lon" not in parts:
        return red(parts["den"]), None, None
    return red(parts["den"]), red(parts["lon"]), 0.5 * red(parts["tra"])


def khat64_exact(k):
    """k / |k| of float64 k, nothing rounded to float32 first"""
    k = np.asarray(k, np.float64).reshape(-1, 3)
    n = np.linalg.norm(k, axis=1, keepdims=True)
    return np.divide(k, n, out=np.zeros_like(k), where=n > 0)


def shell_mean64(fields, bin_of, n_bins):
    """mean over the vectors of each bin of per-vector fields (each (P, L, K) or None): (P, L, n_bins), zeros for an empty bin"""
    return tuple(None if X is None else np.stack(lattice64.shell_mean64(list(X), bin_of, n_bins)) for X in fields)
