"""A float64 restatement of the spectra on the box's reciprocal lattice and of their powder average (psa_amd/lattice.py,
psa_lattice_spectra), for the host tests and the GPU parity tests.  It never calls the library.

The inputs are what the device holds -- float32 positions, velocities and weights, integer indices, and the 9 float64
numbers of the box inverse the caller formed -- taken as exact; every operation is float64: s = r . Hinv, the phase
2 pi n.s, the exponential, the sums over atoms, the Welch stage (tests/dynamic64.spectra64 with k = n.G), and the mean over
a shell, which is taken over an explicit list of the FULL sphere: nothing is folded here."""
import numpy as np

import dynamic64


def lattice_k(indices, inverse):
    """(K, 3) float64 k = n.G, G = 2 pi Hinv^T"""
    return 2.0 * np.pi * (np.asarray(indices, np.float64).reshape(-1, 3) @ np.asarray(inverse, np.float64).T)


def project64(positions, velocities, indices, inverse, idx=None, weights=None, currents=True, with_abs=False):
    """(K, NC, T) complex128: q_0 = sum_a w_a exp(2 pi i n.s[t,a]), q_c = sum_a w_a v[t,a,c] exp(2 pi i n.s[t,a]) with
    s = r . Hinv, over the atom set idx (None: every atom), NC = 4 with currents, else 1.  with_abs: also (NC, T) float64
    sum_a |w_a| |d_a,c(t)|, d = 1 for c = 0 and v_c otherwise."""
    r = np.asarray(positions)
    T, N = r.shape[:2]
    g = np.arange(N) if idx is None else np.asarray(idx, np.int64)
    n = np.asarray(indices, np.float64).reshape(-1, 3)
    inv = np.asarray(inverse, np.float64)
    w = np.ones(N, np.float64) if weights is None else np.asarray(weights).astype(np.float64)
    w = w[g]
    nc = 4 if currents else 1
    q = np.zeros((n.shape[0], nc, T), np.complex128)
    absum = np.zeros((nc, T), np.float64)
    for t in range(T):
        s = r[t, g].astype(np.float64) @ inv                               # (n_g, 3) fractional coordinates
        s -= np.rint(s)                                                    # whole turns do not matter to integer n
        e = np.exp(2j * np.pi * (s @ n.T))                                 # (n_g, K)
        d = np.ones((g.size, 1), np.float64)
        if currents:
            d = np.concatenate([d, np.asarray(velocities)[t, g].astype(np.float64)], axis=1)
        wd = w[:, None] * d
        q[:, :, t] = e.T @ wd
        absum[:, t] = np.sum(np.abs(wd), axis=0)
    return (q, absum) if with_abs else q


def spectra64(q, indices, inverse, window=None, L=None, H=None):
    """(density, longitudinal, transverse) per vector, each (L, K) float64: dynamic64.spectra64 with k = n.G in float64"""
    return dynamic64.spectra64(q, lattice_k(indices, inverse), window, L, H)


def shell_mean64(fields, bin_of, n_bins):
    """mean over the vectors of each bin of per-vector fields (each (L, K) or None): (L, n_bins) each, zeros for an empty
    bin"""
    b = np.asarray(bin_of, np.int64)
    out = []
    for X in fields:
        if X is None:
            out.append(None)
            continue
        Y = np.zeros((X.shape[0], n_bins), np.float64)
        for i in range(n_bins):
            if np.any(b == i):
                Y[:, i] = X[:, b == i].mean(axis=1)
        out.append(Y)
    return tuple(out)


def powder64(positions, velocities, indices_full, inverse, bin_of_full, n_bins, idx=None, weights=None, currents=True,
             window=None, L=None, H=None):
    """the powder average over an explicit list of the full sphere (both n and -n listed, each with its bin): the
    per-vector spectra of every listed vector, averaged per bin.  No folding, no mirror."""
    q = project64(positions, velocities, indices_full, inverse, idx, weights, currents)
    return shell_mean64(spectra64(q, indices_full, inverse, window, L, H), bin_of_full, n_bins)


def fold64(fields_half, bin_of_half, n_bins, mirror=True):
    """what the implementation does, in float64: per half-space vector (X_n[o] + X_n[(L - o) mod L]) / 2, averaged per
    bin; mirror=False: the wrong fold X_n[o] alone, which the tests show to differ"""
    folded = []
    for X in fields_half:
        if X is None:
            folded.append(None)
            continue
        L = X.shape[0]
        folded.append(0.5 * (X + X[(L - np.arange(L)) % L]) if mirror else X)
    return shell_mean64(folded, bin_of_half, n_bins)
