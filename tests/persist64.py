"""float64 reference of the bond-persistence tests, by the definition of include/psa_hip.h and nothing else: a brute force
over all ordered pairs of listed atoms at every frame, the minimum image found by the image SEARCH of tests/pair64.py, the
neighbours by r < r_cut at the origin, aliveness by r < r_break at the later frame -- no rint, no masks, no tags, no tiling,
nothing shared with the route."""
import numpy as np

import angle64 as A
import pair64 as R

CAPACITY = A.CAPACITY


def n_origins(n_frames, lag, step=1):
    return R.n_origins(n_frames, int(lag), step)


def visited(lag, sample_step):
    """the frames offsets v = sample_step, 2 sample_step, ... <= lag at which a bond must be alive to count as unbroken"""
    return list(range(sample_step, int(lag) + 1, sample_step))


def distances(positions, box, groups):
    """per frame the (n, n) minimum-image distances of the listed atoms"""
    atoms, _ = A.species_of(groups)
    return [A.frame_pairs(frame, box, atoms)[2] for frame in positions]


def counts64(positions, box, groups, r_cut, r_break, lags, step=1, sample_step=1, continuous=True, dist=None):
    """dict of bonds, alive, unbroken (n_lags, S, S), lost (n_lags, S, 65), truncated (n_lags, S) int64 by the definition"""
    S, T = len(groups), np.shape(positions)[0]
    rc, rb = A.cutoffs(r_cut, S), A.cutoffs(r_cut if r_break is None else r_break, S)
    atoms, spec = A.species_of(groups)
    n, n_l = atoms.size, len(lags)
    out = dict(bonds=np.zeros((n_l, S, S), np.int64), alive=np.zeros((n_l, S, S), np.int64), unbroken=np.zeros((n_l, S, S), np.int64),
               lost=np.zeros((n_l, S, CAPACITY + 1), np.int64), truncated=np.zeros((n_l, S), np.int64))
    if n == 0:
        return out
    dist = distances(positions, box, groups) if dist is None else dist
    cut, brk = rc[spec[:, None], spec[None, :]], rb[spec[:, None], spec[None, :]]
    off = ~np.eye(n, dtype=bool)
    for j, lag in enumerate(int(t) for t in lags):
        for o in range(0, T - lag, step):
            near = (dist[o] < cut) & off
            for a in range(n):
                nb = np.flatnonzero(near[a])
                if nb.size > CAPACITY:
                    out["truncated"][j, spec[a]] += 1
                    continue
                up = dist[o + lag][a, nb] < brk[a, nb]
                whole = np.ones(nb.size, bool)
                for v in visited(lag, sample_step) if continuous else []:
                    whole &= dist[o + v][a, nb] < brk[a, nb]
                for be in range(S):
                    of = spec[nb] == be
                    out["bonds"][j, spec[a], be] += int(of.sum())
                    out["alive"][j, spec[a], be] += int((of & up).sum())
                    if continuous:
                        out["unbroken"][j, spec[a], be] += int((of & whole).sum())
                out["lost"][j, spec[a], int((~up).sum())] += 1
    return out
