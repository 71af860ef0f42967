"""float64 reference of the pair-distribution tests, by the definition of include/psa_hip.h and nothing else: a brute force
over all ordered pairs and origins, the minimum image found by SEARCHING the periodic images n in {-2..2}^3 of the
difference folded into the cell with floor -- no rint, no tiling, nothing shared with the route."""
import itertools

import numpy as np

IMAGES = np.array(list(itertools.product(range(-2, 3), repeat=3)), np.float64)          # (125, 3)


def box64(box):
    """(H, Hinv) float64 of a box matrix whose float32 entries are taken as exact"""
    H = np.asarray(box, np.float32).astype(np.float64)
    return H, np.linalg.inv(H)


def fractions64(positions, box):
    """c (T, N, 3) float64 = sigma - floor(sigma) - 0.5, sigma = r Hinv, in extended precision where the platform has it"""
    r = np.asarray(positions, np.float32).astype(np.longdouble)
    s = r @ box64(box)[1].astype(np.longdouble)
    return (s - np.floor(s) - 0.5).astype(np.float64)


def origins(n_frames, lag, step=1):
    return np.arange(0, n_frames - lag, step)


def n_origins(n_frames, lag, step=1):
    return (n_frames - 1 - lag) // step + 1


def minimum_image(delta, box):
    """(e (n, 3), d (n, 3), r (n,)): of the differences delta (n, 3) the image of least length among (f + n) H, f the
    fractional difference folded into [0, 1), n in {-2..2}^3; e = f + n its fractional form, d = e H"""
    H, inv = box64(box)
    f = delta @ inv
    f = f - np.floor(f)
    cart, img = f @ H, IMAGES @ H
    e = np.empty_like(f)
    for lo in range(0, f.shape[0], 1 << 16):                               # |fH + nH|^2 = |fH|^2 + 2 fH.nH + |nH|^2: the argmin over n
        c = cart[lo:lo + (1 << 16)]
        best = np.argmin(2.0 * (c @ img.T) + (img * img).sum(axis=1)[None, :], axis=1)
        e[lo:lo + (1 << 16)] = f[lo:lo + (1 << 16)] + IMAGES[best]
    d = e @ H
    return e, d, np.sqrt((d * d).sum(axis=1))


def pair_samples(positions, box, alpha, beta, lag, step=1):
    """(e, d, r) of every sample (a in alpha, b in beta, b != a, o in O_lag): b at frame o + lag, a at frame o"""
    r = np.asarray(positions, np.float32).astype(np.float64)
    a, b = np.asarray(alpha, np.int64), np.asarray(beta, np.int64)
    o = origins(r.shape[0], lag, step)
    delta = r[o + lag][:, None, b, :] - r[o][:, a, None, :]                 # (n_o, N_a, N_b, 3)
    keep = np.broadcast_to((a[:, None] != b[None, :])[None], delta.shape[:3])
    return minimum_image(delta[keep], box)


def bins(r, dr, n_r):
    """(n_r + 1,) int64: the histogram of floor(r / dr), the last entry everything at n_r and beyond"""
    return np.bincount(np.minimum(np.floor(r / dr).astype(np.int64), n_r), minlength=n_r + 1)


def counts64(positions, box, groups, lags, step, dr, n_r):
    """(n_vh, S, S, n_r + 1) int64 by the definition"""
    S = len(groups)
    out = np.zeros((len(lags), S, S, n_r + 1), np.int64)
    for j, lag in enumerate(lags):
        for a in range(S):
            for b in range(S):
                if len(groups[a]) and len(groups[b]):
                    out[j, a, b] = bins(pair_samples(positions, box, groups[a], groups[b], int(lag), step)[2], dr, n_r)
    return out
