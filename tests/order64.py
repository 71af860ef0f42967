"""float64 reference of the bond-order tests, by the definition of include/psa_hip.h at psa_bond_order and nothing else: the
neighbours by the brute force of tests/angle64.py (image search, r < r_cut), q_l from the spherical harmonics themselves --
associated Legendre functions by their recurrences, the complex sum over the legs for every m, the sum of the moduli over m.
No addition theorem, no Legendre polynomial of a cosine between legs, nothing shared with the route."""
import math

import numpy as np

import angle64 as A

CAPACITY = A.CAPACITY


def assoc_legendre(l_max, x):
    """P[l][m] (each like x), 0 <= m <= l <= l_max, of x in [-1, 1]: P_m^m = (2 m - 1)!! (1 - x^2)^(m/2) (the sign of the
    Condon-Shortley phase left out: only moduli are used), P_{m+1}^m = (2 m + 1) x P_m^m, then upwards in l"""
    x = np.asarray(x, np.float64)
    s = np.sqrt(np.maximum(1.0 - x * x, 0.0))
    P = [[None] * (l + 1) for l in range(l_max + 1)]
    P[0][0] = np.ones_like(x)
    for m in range(1, l_max + 1):
        P[m][m] = P[m - 1][m - 1] * (2 * m - 1) * s
    for m in range(l_max):
        P[m + 1][m] = (2 * m + 1) * x * P[m][m]
        for l in range(m + 2, l_max + 1):
            P[l][m] = ((2 * l - 1) * x * P[l - 1][m] - (l + m - 1) * P[l - 2][m]) / (l - m)
    return P


def q_squared(legs, ls):
    """q_l^2 (len(ls),) of one shell: legs (n, 3), none of length 0; n >= 1"""
    d = np.asarray(legs, np.float64)
    r = np.sqrt((d * d).sum(axis=1))
    ct, phi = d[:, 2] / r, np.arctan2(d[:, 1], d[:, 0])
    P = assoc_legendre(max(ls), ct)
    out = np.zeros(len(ls))
    for j, l in enumerate(ls):
        total = 0.0
        for m in range(l + 1):
            norm = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            mean = (norm * P[l][m] * np.exp(1j * m * phi)).mean()          # 1/n sum_b Y_lm(d_b)
            total += (1.0 if m == 0 else 2.0) * abs(mean) ** 2              # |Y_l,-m| = |Y_lm|
        out[j] = 4.0 * math.pi / (2 * l + 1) * total
    return out


def theorem(legs, ls):
    """the same by the addition theorem, 1/n^2 (n + 2 sum_{b<c} P_l(cos)): what the route evaluates, here only to be
    compared with `q_squared`"""
    d = np.asarray(legs, np.float64)
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    n = d.shape[0]
    j, k = np.triu_indices(n, 1)
    cos = np.clip((d[j] * d[k]).sum(axis=1), -1.0, 1.0)
    return np.array([(n + 2.0 * np.polynomial.legendre.legval(cos, [0.0] * l + [1.0]).sum()) / n ** 2 for l in ls])


def frame_shells(frame, box, groups, r_cut):
    """(d (n, n, 3), r (n, n), near (n, n) bool) of one frame over the groups' atoms concatenated: b is a neighbour of a where
    near[a, b]"""
    S = len(groups)
    rc = A.cutoffs(r_cut, S)
    atoms, spec = A.species_of(groups)
    _, d, r = A.frame_pairs(frame, box, atoms)
    return d, r, (r < rc[spec[:, None], spec[None, :]]) & ~np.eye(atoms.size, dtype=bool)


def per_atom(positions, box, groups, r_cut, step, ls):
    """(xq (n_o, n_a, n_l) float64 = n^2 q_l^2, NaN where the centre is left out; n (n_o, n_a) the neighbour counts; why
    (n_o, n_a): 0 counted, 1 truncated, 2 isolated, 3 undefined) by the definition"""
    atoms, _ = A.species_of(groups)
    origins = range(0, np.shape(positions)[0], step)
    xq = np.full((len(origins), atoms.size, len(ls)), np.nan)
    count, why = np.zeros((len(origins), atoms.size), np.int64), np.zeros((len(origins), atoms.size), np.int64)
    for o, f in enumerate(origins):
        if atoms.size == 0:
            break
        d, r, near = frame_shells(positions[f], box, groups, r_cut)
        for a in range(atoms.size):
            nb = np.flatnonzero(near[a])
            count[o, a] = nb.size
            if nb.size > CAPACITY:
                why[o, a] = 1
            elif nb.size == 0:
                why[o, a] = 2
            elif nb.size > 1 and np.any(r[a, nb] == 0.0):                  # a pair of legs without a cosine
                why[o, a] = 3
            elif nb.size == 1:                                              # one leg, no pair: q_l = 1 whatever the leg
                xq[o, a] = 1.0
            else:
                xq[o, a] = nb.size ** 2 * q_squared(d[a, nb], ls)
    return xq, count, why
