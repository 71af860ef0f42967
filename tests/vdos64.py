"""A float64 restatement of the vibrational density of states (psa_vdos, psa_amd/vdos.py), for the GPU parity tests and
the check against scipy.signal.welch.  The data are taken as they are (float32 values, then float64 for everything:
mean subtraction, weight, window, FFT, 1/L, |.|^2, the sums, the norm)."""
import numpy as np


def segment_count(T, L, H):
    return 1 + (T - L) // H


def vdos64(data, groups, window=None, L=None, H=None, weights=None, mean=None):
    """(L // 2 + 1, G, 3) float64:  D[o,g,c] = 1/(n_seg U) sum_s sum_{a in g} w_a^2 |(1/L) FFT_tau(win[tau] d[s H + tau, a, c])[o]|^2

    data (T, N, 3); groups: a list of index arrays (None in it: every atom); window None: boxcar; L, H None: T;
    mean (N, 3): subtracted first (displacement mode)."""
    data = np.asarray(data)
    T, N = data.shape[0], data.shape[1]
    L = T if L is None else L
    H = L if H is None else H
    win = np.ones(L) if window is None else np.asarray(window, np.float32).astype(np.float64)
    n_seg, U, F = segment_count(T, L, H), float(np.dot(win, win)) / L, L // 2 + 1
    w = np.ones(N) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    out = np.zeros((F, len(groups), 3), np.float64)
    for gi, g in enumerate(groups):
        idx = np.arange(N) if g is None else np.asarray(g, np.int64)
        if idx.size == 0:
            continue
        d = data[:, idx, :].astype(np.float64)
        if mean is not None:
            d = d - np.asarray(mean, np.float64)[None, idx, :]
        d = d * w[idx][None, :, None]
        for s in range(n_seg):
            X = np.fft.fft(win[:, None, None] * d[s * H:s * H + L], axis=0)[:F] / L
            out[:, gi, :] += np.sum(np.abs(X) ** 2, axis=1)
    return out / (n_seg * U)


def scipy_factor(window, L):
    """D = factor * scipy.signal.welch(..., scaling="spectrum", return_onesided=False, detrend=False): (sum w)^2 / (L sum w^2)"""
    w = np.asarray(window, np.float32).astype(np.float64)
    return float(np.sum(w)) ** 2 / (L * float(np.dot(w, w)))


def parseval_sum(D, L):
    """D[0] + 2 sum_{0<o<L/2} D[o] (+ D[L/2] once for even L), over axis 0: the two-sided total of a one-sided spectrum"""
    D = np.asarray(D, np.float64)
    if L % 2 == 0:
        return D[0] + 2.0 * np.sum(D[1:L // 2], axis=0) + D[L // 2]
    return D[0] + 2.0 * np.sum(D[1:], axis=0)
