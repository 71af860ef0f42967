"""A float64 restatement of the segment-averaged (Welch) SED (psa_amd/segments.py, psa_set_segments), for the GPU
parity tests and the check against scipy.signal.welch.

q is the projection of one atom group as tests/ref64.py computes it -- the reference's float32 phase argument, then
float64 -- before any FFT; everything after it (window, segments, FFT, 1/L, |.|^2, the norm) is float64."""
import numpy as np

from ref64 import phases


def project64(data, mean_pos_all, k_vectors, idx=None, weights=None):
    """(T, K, 3) complex128 q[t, k, c] = sum_a w_a d[t, a, c] exp(i k.r_a) over the group idx (None: every atom)."""
    data = np.asarray(data)
    g = np.arange(data.shape[1]) if idx is None else np.asarray(idx, np.int64)
    P = phases(k_vectors, np.asarray(mean_pos_all, np.float32)[g])                  # (K, n)
    if weights is not None:
        P = P * np.asarray(weights, np.float32)[g].astype(np.float64)[None, :]
    Pr, Pi = np.ascontiguousarray(P.real.T), np.ascontiguousarray(P.imag.T)
    q = np.empty((data.shape[0], P.shape[0], 3), np.complex128)
    for c in range(3):
        d = data[:, g, c].astype(np.float64)
        q[:, :, c] = d @ Pr + 1j * (d @ Pi)
    return q


def segment_count(T, L, H):
    return 1 + (T - L) // H


def segment_intensity64(q, window, L, H):
    """(L, K) float64: 1/(n_seg U) sum_s sum_c |(1/L) FFT_tau(w[tau] q[s H + tau, k, c])|^2 of q (T, K, 3)."""
    T = q.shape[0]
    n_seg = segment_count(T, L, H)
    w = np.asarray(window, np.float32).astype(np.float64)
    U = float(np.dot(w, w)) / L
    out = np.zeros((L, q.shape[1]), np.float64)
    for s in range(n_seg):
        F = np.fft.fft(w[:, None, None] * q[s * H:s * H + L], axis=0) / L
        out += np.sum(np.abs(F) ** 2, axis=-1)
    return out / (n_seg * U)


def welch_intensity64(data, mean_pos_all, k_vectors, groups, window, L, H, weights=None):
    """segment_intensity64 summed over the atom groups (a list of index arrays; [None] = every atom as one group)"""
    out = 0.0
    for g in groups:
        out = out + segment_intensity64(project64(data, mean_pos_all, k_vectors, g, weights), window, L, H)
    return out


def scipy_factor(window, L):
    """I = factor * scipy.signal.welch(..., scaling="spectrum") summed over components: (sum w)^2 / (L sum w^2)"""
    w = np.asarray(window, np.float32).astype(np.float64)
    return float(np.sum(w)) ** 2 / (L * float(np.dot(w, w)))
