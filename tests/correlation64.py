"""A float64 restatement of the time correlations on the box's reciprocal lattice (psa_amd/correlations.py,
psa_lattice_correlations, psa_self_correlations), for the host tests and the GPU parity tests.  It never calls the library.

The projections are formed as tests/lattice64.project64 and tests/self64.series64 form them.  F is computed by the
TIME-DOMAIN sums of the definition,

    F[t] = 1/(n_seg (L - t)) Re sum_s sum_{l=0}^{L-1-t} x[sH + l + t] conj x[sH + l],

never by an FFT: no padding, no transform length, no back-transform -- the reference shares nothing with the route under
test.  The shell mean is taken over an explicit list of vectors (the full sphere where the caller lists it)."""
import numpy as np

import dynamic64
import lattice64
import self64


def correlate64(x, L=None, H=None, n_lags=None):
    """(..., n_lags) float64 of series x (..., T) complex: the linear, unbiased correlation of the segments of L frames,
    H apart (None: one segment of all T frames), at lags 0 .. n_lags - 1 (None: L // 2)"""
    x = np.asarray(x, np.complex128)
    T = x.shape[-1]
    if L is None:
        L, H = T, T
    n_lags = L // 2 if n_lags is None else n_lags
    assert 1 <= n_lags <= L <= T and H >= 1
    n_seg = 1 + (T - L) // H
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    out = np.zeros(x.shape[:-1] + (n_lags,), np.float64)
    for t in range(n_lags):
        total = np.zeros(x.shape[:-1], np.float64)
        for s in range(n_seg):
            a, b = s * H, s * H + L
            # Re (u conj v) = u_r v_r + u_i v_i
            total += np.einsum("...l,...l->...", re[..., a + t:b], re[..., a:b - t])
            total += np.einsum("...l,...l->...", im[..., a + t:b], im[..., a:b - t])
        out[..., t] = total / (n_seg * (L - t))
    return out


def fields64(q, indices, inverse, L=None, H=None, n_lags=None):
    """(density, longitudinal, transverse), each (n_lags, K) float64 (the last two None for q of one series), of the
    projections q (K, NC, T) of tests/lattice64.project64: density from q_0, longitudinal from khat.q, transverse half the
    sum over the three perpendicular components q_c - khat_c (khat.q)"""
    q = np.asarray(q, np.complex128)
    den = correlate64(q[:, 0], L, H, n_lags).T
    if q.shape[1] == 1:
        return den, None, None
    h = dynamic64.khat64(lattice64.lattice_k(indices, inverse))            # (K, 3)
    par = np.einsum("kc,kct->kt", h, q[:, 1:])
    perp = q[:, 1:] - h[:, :, None] * par[:, None, :]
    tra = 0.5 * sum(correlate64(perp[:, c], L, H, n_lags) for c in range(3)).T
    return den, correlate64(par, L, H, n_lags).T, tra


def lattice_correlations64(positions, velocities, indices, inverse, idx=None, weights=None, currents=True, L=None, H=None,
                           n_lags=None):
    """fields64 of lattice64.project64: the whole definition, per vector"""
    q = lattice64.project64(positions, velocities, indices, inverse, idx, weights, currents)
    return fields64(q, indices, inverse, L, H, n_lags)


def self_correlations64(positions, indices, inverse, idx=None, weights=None, L=None, H=None, n_lags=None):
    """(n_lags, K) float64: sum over the atoms of the set of the correlation of z[a,n,.] = w_a exp(2 pi i n.s_a) -- atom
    by atom, nothing is summed over atoms before the correlation"""
    r = np.asarray(positions)
    N = r.shape[1]
    g = np.arange(N) if idx is None else np.asarray(idx, np.int64)
    total = None
    for a in g:
        c = correlate64(self64.series64(r, indices, inverse, [a], weights)[0], L, H, n_lags).T
        total = c if total is None else total + c
    return total


def shell_mean64(fields, bin_of, n_bins):
    """the mean of per-vector fields (each (n_lags, K) or None) over the vectors of each bin: (n_lags, n_bins) each, zeros
    for an empty bin"""
    return lattice64.shell_mean64(fields, bin_of, n_bins)
