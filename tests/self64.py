"""A float64 restatement of the self (incoherent) dynamic structure factor on the box's reciprocal lattice and of its powder
average (psa_amd/self_spectra.py, psa_self_spectra), for the host tests and the GPU parity tests.  It never calls the
library.

The inputs are what the device holds -- float32 positions and weights, integer indices, the 9 float64 numbers of the box
inverse -- taken as exact (an array that is float64 already is used as it is); every operation is float64: s = r . Hinv as
tests/lattice64.project64 forms it, the phase 2 pi n.s, the exponential, the window, the FFT, the modulus, the sums over
segments and atoms -- atom by atom, nothing is summed over atoms before the modulus -- and the mean over a shell, which is
taken over an explicit list of the FULL sphere: nothing is folded here."""
import numpy as np

import lattice64


def _atoms(positions, idx, weights):
    N = np.asarray(positions).shape[1]
    g = np.arange(N) if idx is None else np.asarray(idx, np.int64)
    w = np.ones(N, np.float64) if weights is None else np.asarray(weights).astype(np.float64)
    return g, w[g]


def series64(positions, indices, inverse, idx=None, weights=None):
    """(n_g, K, T) complex128: z[a,n,t] = w_a exp(2 pi i n.s[t,a]), s = r . Hinv, over the atom set idx (None: every atom)
    in its order"""
    r = np.asarray(positions)
    g, w = _atoms(r, idx, weights)
    n = np.asarray(indices, np.float64).reshape(-1, 3)
    inv = np.asarray(inverse, np.float64)
    z = np.zeros((g.size, n.shape[0], r.shape[0]), np.complex128)
    for i, a in enumerate(g):
        s = r[:, a].astype(np.float64) @ inv                               # (T, 3) fractional coordinates of one atom
        s -= np.rint(s)                                                    # whole turns do not matter to integer n
        z[i] = w[i] * np.exp(2j * np.pi * (n @ s.T))
    return z


def density64(positions, indices, inverse, idx=None, weights=None, window=None, L=None, H=None):
    """(L, K) float64: 1/(n_seg U L^2) sum_a sum_s |FFT_l(win[l] z[a,n,sH+l])|^2.  No window: L = H = T, win = 1."""
    r = np.asarray(positions)
    T = r.shape[0]
    g, _ = _atoms(r, idx, weights)
    if window is None:
        L, H, win = T, T, np.ones(T, np.float64)
    else:
        win = np.asarray(window, np.float32).astype(np.float64)
    n_seg = 1 + (T - L) // H
    U = float(np.dot(win, win)) / L
    K = np.asarray(indices).reshape(-1, 3).shape[0]
    den = np.zeros((L, K), np.float64)
    for a in g:                                                            # per atom: the modulus comes before the sum
        z = series64(r, indices, inverse, [a], weights)[0]                 # (K, T)
        for s in range(n_seg):
            den += (np.abs(np.fft.fft(win[None, :] * z[:, s * H:s * H + L], axis=1)) ** 2).T
    return den / (n_seg * U * L * L)


def shell_mean64(density, bin_of, n_bins):
    """the mean of a per-vector density (L, K) over the vectors of each bin: (L, n_bins), zeros for an empty bin"""
    return lattice64.shell_mean64([density], bin_of, n_bins)[0]
