"""A float64 restatement of the dynamic structure factor and the current correlations (psa_amd/dynamic.py,
psa_dynamic_spectra), for the host tests and the GPU parity tests.

The inputs are what the device holds -- float32 positions, velocities, weights and k-vectors -- taken as exact numbers;
every operation is float64: the phase k.r (the three products are exact in float64), the exponential, the sums over
atoms, and the Welch stage (window, segments, FFT, 1/L, the contraction with k/|k|, the modulus, the norm).  An array
that is float64 already is used as it is (the Jacobi-Anger test holds the identity, not the rounding of its inputs)."""
import numpy as np


def project64(positions, velocities, k_vectors, idx=None, weights=None, currents=True, with_abs=False):
    """(K, NC, T) complex128: q_0 = sum_a w_a exp(i k.r[t,a]), q_c = sum_a w_a v[t,a,c] exp(i k.r[t,a]) over the atom
    set idx (None: every atom), NC = 4 with currents, else 1.  with_abs: also (NC, T) float64 sum_a |w_a| |d_a,c(t)|,
    d = 1 for c = 0 and v_c otherwise -- what the per-element bound of the kernel multiplies."""
    r = np.asarray(positions)
    T, N = r.shape[:2]
    g = np.arange(N) if idx is None else np.asarray(idx, np.int64)
    k = np.asarray(k_vectors).astype(np.float64).reshape(-1, 3)
    w = np.ones(N, np.float64) if weights is None else np.asarray(weights).astype(np.float64)
    w = w[g]
    nc = 4 if currents else 1
    q = np.zeros((k.shape[0], nc, T), np.complex128)
    absum = np.zeros((nc, T), np.float64)
    for t in range(T):
        rt = r[t, g].astype(np.float64)                                   # (n, 3)
        e = np.exp(1j * (rt @ k.T))                                       # (n, K)
        d = np.ones((g.size, 1), np.float64)
        if currents:
            d = np.concatenate([d, np.asarray(velocities)[t, g].astype(np.float64)], axis=1)   # (n, 4)
        wd = w[:, None] * d
        q[:, :, t] = e.T @ wd
        absum[:, t] = np.sum(np.abs(wd), axis=0)
    return (q, absum) if with_abs else q


def khat64(k_vectors):
    """(K, 3) float64 k / |k|; k = 0: 0"""
    k = np.asarray(k_vectors).astype(np.float64).reshape(-1, 3)
    n = np.linalg.norm(k, axis=1)
    return np.divide(k, n[:, None], out=np.zeros_like(k), where=n[:, None] > 0)


def spectra64(q, k_vectors, window=None, L=None, H=None):
    """(density, longitudinal, transverse), each (L, K) float64 (the last two None for q of one series), of q (K, NC, T):
    F_s = (1/L) FFT_tau(win[tau] q[.., s H + tau]); density = 1/(n_seg U) sum_s |F_s,0|^2; longitudinal the same of
    sum_c khat_c F_s,c; transverse (sum_c |F_s,c|^2 averaged alike - longitudinal) / 2.  No window: L = H = T, win = 1."""
    K, nc, T = q.shape
    if window is None:
        L, H, win = T, T, np.ones(T, np.float64)
    else:
        win = np.asarray(window, np.float32).astype(np.float64)
    n_seg = 1 + (T - L) // H
    U = float(np.dot(win, win)) / L
    h = khat64(k_vectors)
    den = np.zeros((L, K), np.float64)
    lon, tot = np.zeros((L, K), np.float64), np.zeros((L, K), np.float64)
    for s in range(n_seg):
        F = np.fft.fft(win[None, None, :] * q[:, :, s * H:s * H + L], axis=2) / L      # (K, NC, L)
        den += (np.abs(F[:, 0]) ** 2).T
        if nc == 4:
            tot += np.sum(np.abs(F[:, 1:]) ** 2, axis=1).T
            lon += (np.abs(np.einsum("kc,kco->ko", h, F[:, 1:])) ** 2).T
    norm = n_seg * U
    if nc == 1:
        return den / norm, None, None
    return den / norm, lon / norm, 0.5 * (tot - lon) / norm


def dynamic_spectra64(positions, velocities, k_vectors, idx=None, weights=None, currents=True, window=None, L=None, H=None):
    """spectra64 of project64: the whole definition"""
    return spectra64(project64(positions, velocities, k_vectors, idx, weights, currents), k_vectors, window, L, H)
