"""float64 reference of the bond-angle tests, by the definition of include/psa_hip.h and nothing else: a brute force over all
ordered pairs of listed atoms at every origin, the minimum image found by the image SEARCH of tests/pair64.py, neighbours
by r < r_cut, angles by arccos -- no rint, no table of cosines, no tiling, nothing shared with the route."""
import numpy as np

import pair64 as R

CAPACITY = 64


def n_origins(n_frames, step=1):
    return (n_frames - 1) // step + 1


def cutoffs(r_cut, n_species):
    rc = np.asarray(r_cut, np.float64)
    return np.full((n_species, n_species), float(rc)) if rc.ndim == 0 else rc


def pair_row(b, c, n_species):
    b, c = min(b, c), max(b, c)
    return b * n_species - b * (b - 1) // 2 + (c - b)


def species_of(groups):
    """(the atoms of the groups concatenated, the species of each list position)"""
    atoms = np.concatenate([np.asarray(g, np.int64) for g in groups]) if groups else np.zeros(0, np.int64)
    return atoms, np.concatenate([np.full(len(g), s, np.int64) for s, g in enumerate(groups)]) if groups else np.zeros(0, np.int64)


def frame_pairs(frame, box, atoms):
    """(e, d, r), each (n, n, ...): the minimum image of r_b - r_a for every ordered pair (a, b) of list positions"""
    n = atoms.size
    r = np.asarray(frame, np.float32).astype(np.float64)[atoms]
    delta = (r[None, :, :] - r[:, None, :]).reshape(-1, 3)
    e, d, dist = R.minimum_image(delta, box)
    return e.reshape(n, n, 3), d.reshape(n, n, 3), dist.reshape(n, n)


def theta_bin(cos, n_theta):
    """the bin of arccos(cos) among n_theta uniform bins over [0, pi]; pi itself in the last"""
    t = np.arccos(np.clip(cos, -1.0, 1.0))
    return np.minimum(np.floor(t * (n_theta / np.pi)).astype(np.int64), n_theta - 1)


def counts64(positions, box, groups, r_cut, step, n_theta):
    """(angles (S, P, n_theta + 1), coord (S, S, 65), truncated (S,)) int64 by the definition"""
    S = len(groups)
    P = S * (S + 1) // 2
    rc = cutoffs(r_cut, S)
    atoms, spec = species_of(groups)
    angles, coord, trunc = np.zeros((S, P, n_theta + 1), np.int64), np.zeros((S, S, CAPACITY + 1), np.int64), np.zeros(S, np.int64)
    for o in range(0, np.shape(positions)[0], step):
        if atoms.size == 0:
            break
        _, d, r = frame_pairs(positions[o], box, atoms)
        cut = rc[spec[:, None], spec[None, :]]
        near = (r < cut) & ~np.eye(atoms.size, dtype=bool)
        for a in range(atoms.size):
            nb = np.flatnonzero(near[a])
            if nb.size > CAPACITY:
                trunc[spec[a]] += 1
                continue
            for be in range(S):
                coord[spec[a], be, int((spec[nb] == be).sum())] += 1
            j, k = np.triu_indices(nb.size, 1)
            if j.size == 0:
                continue
            db, dc, rb, rk = d[a, nb[j]], d[a, nb[k]], r[a, nb[j]], r[a, nb[k]]
            with np.errstate(invalid="ignore", divide="ignore"):
                cos = (db * dc).sum(axis=1) / (rb * rk)
            bad = (rb == 0.0) | (rk == 0.0)
            bins = np.where(bad, n_theta, theta_bin(np.where(bad, 0.0, cos), n_theta))
            lo, hi = np.minimum(spec[nb[j]], spec[nb[k]]), np.maximum(spec[nb[j]], spec[nb[k]])
            np.add.at(angles[spec[a]], (lo * S - lo * (lo - 1) // 2 + hi - lo, bins), 1)
    return angles, coord, trunc


def neighbour_sets(frame, box, groups, r_cut, centres=None):
    """per list position (of `centres`, default all) the sorted list positions of its neighbours, by the definition"""
    S = len(groups)
    rc = cutoffs(r_cut, S)
    atoms, spec = species_of(groups)
    rows = np.arange(atoms.size) if centres is None else np.asarray(centres, np.int64)
    r = np.asarray(frame, np.float32).astype(np.float64)[atoms]
    dist = R.minimum_image((r[None, :, :] - r[rows][:, None, :]).reshape(-1, 3), box)[2].reshape(rows.size, atoms.size)
    near = (dist < rc[spec[rows][:, None], spec[None, :]]) & (rows[:, None] != np.arange(atoms.size)[None, :])
    return [np.flatnonzero(row) for row in near]
