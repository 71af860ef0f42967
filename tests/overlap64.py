"""float64 reference of the self-overlap tests, by the definition of include/psa_hip.h and nothing else: per lag, group
and origin the number of atoms whose displacement is shorter than the cut-off, and its two sums over the origins.  Built
on tests/msd64.py (the unwrapped displacements); no tiling, nothing shared with the route."""
import numpy as np

import msd64 as R


def overlap64(u, groups, lags, step, cutoff):
    """(Q (n_lags, G, n_o_max) int64 -- zero at k >= n_o(lag) --, S1 (n_lags, G) int64, S2 (n_lags, G) int64) with
    Q[j,g,k] = #{a in g: |u[o_k + lag_j, a] - u[o_k, a]| / cutoff < 1}, the bin 0 of msd64.counts64 with one bin"""
    lags = [int(t) for t in lags]
    n_o_max = R.n_origins(u.shape[0], min(lags), step)
    Q = np.zeros((len(lags), len(groups), n_o_max), np.int64)
    for j, lag in enumerate(lags):
        for g, atoms in enumerate(groups):
            if len(atoms) == 0:
                continue
            x = np.sqrt((R.displacements(u, atoms, lag, step) ** 2).sum(axis=2)) / cutoff
            Q[j, g, :x.shape[0]] = (np.floor(x) == 0).sum(axis=1)
    return Q, Q.sum(axis=2), (Q * Q).sum(axis=2)


def chi4_fraction(s1, s2, n_o, n_g):
    """(n_o S2 - S1^2) / (n_o^2 N_g) as a fractions.Fraction"""
    from fractions import Fraction
    return Fraction(int(n_o) * int(s2) - int(s1) ** 2, int(n_o) ** 2 * int(n_g))
