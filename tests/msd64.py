"""float64 references of the displacement tests, by the definitions of include/psa_hip.h and nothing else: the unwrapped
displacements, the moments as plain time-domain means over origins and atoms, the histogram of |D| / dr.  No tiling,
nothing shared with the route."""
import numpy as np


def box64(box):
    """(H, Hinv) float64 of a box matrix whose float32 entries are taken as exact"""
    H = np.asarray(box, np.float32).astype(np.float64)
    return H, np.linalg.inv(H)


def unwrap64(positions, box, unwrap=True):
    """(u (T, N, 3) float64, n (T, N, 3) int64, S (T, N, 3) float64) from float32 positions: d = (r[t] - r[t-1]) Hinv,
    m = rint(d), n = -cumsum(m), u = (r[t] - r[0]) + n H -- the last line in extended precision where the platform has
    it, rounded once to float64 -- and S = |r(t) - r(0)| + sum_j |n_j| |H_jc|, the magnitude the bound of u multiplies."""
    r = np.asarray(positions, np.float32).astype(np.float64)
    H, inv = box64(box)
    n = np.zeros(r.shape, np.int64)
    if unwrap:
        d = (r[1:] - r[:-1]) @ inv
        n[1:] = -np.cumsum(np.rint(d).astype(np.int64), axis=0)
    e = (r - r[:1]).astype(np.longdouble)
    u = (e + n.astype(np.longdouble) @ H.astype(np.longdouble)).astype(np.float64)
    S = np.abs(r - r[:1]) + np.abs(n).astype(np.float64) @ np.abs(H)
    return u, n, S


def hop_margin(positions, box):
    """the largest |d_j - rint(d_j)| over all frames, atoms and axes: how near the input comes to a tie"""
    r = np.asarray(positions, np.float32).astype(np.float64)
    d = (r[1:] - r[:-1]) @ box64(box)[1]
    return float(np.max(np.abs(d - np.rint(d)))) if d.size else 0.0


def origins(n_frames, lag, step=1):
    """the origins 0, s, 2 s, ... with o + lag <= T - 1"""
    return np.arange(0, n_frames - lag, step)


def n_origins(n_frames, lag, step=1):
    return (n_frames - 1 - lag) // step + 1


def displacements(u, atoms, lag, step=1):
    """D (n_o, n_a, 3) = u[o + lag, a] - u[o, a]"""
    o = origins(u.shape[0], lag, step)
    a = np.asarray(atoms, np.int64)
    return u[o + lag][:, a] - u[o][:, a]


def moments64(u, groups, n_lags, step=1):
    """(n_lags, G, 4) float64: the means over origins and the group's atoms of D_x^2, D_y^2, D_z^2, |D|^4; an empty group: 0"""
    out = np.zeros((n_lags, len(groups), 4))
    for g, atoms in enumerate(groups):
        if len(atoms) == 0:
            continue
        for t in range(n_lags):
            q = displacements(u, atoms, t, step) ** 2
            out[t, g, :3] = q.mean(axis=(0, 1))
            out[t, g, 3] = (q.sum(axis=2) ** 2).mean()
    return out


def alpha2(moments):
    msd = moments[..., :3].sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(msd != 0, 3.0 * moments[..., 3] / (5.0 * msd * msd) - 1.0, np.nan)


def counts64(u, groups, lags, step, dr, n_r):
    """(n_vh, G, n_r + 1) int64: bin floor(|D| / dr) of every (atom of the group, origin), the last entry the overflow"""
    out = np.zeros((len(lags), len(groups), n_r + 1), np.int64)
    for j, lag in enumerate(lags):
        for g, atoms in enumerate(groups):
            if len(atoms) == 0:
                continue
            x = np.sqrt((displacements(u, atoms, int(lag), step) ** 2).sum(axis=2)) / dr
            out[j, g] = np.bincount(np.minimum(np.floor(x).astype(np.int64), n_r).ravel(), minlength=n_r + 1)
    return out
