"""
Steinhardt bond-orientational order parameters q_l: how ordered the neighbour shell of every atom is, in every frame.

With the neighbours of `psa_amd/angles.py` (b is a neighbour of a when b != a, r_cut[alpha, beta] > 0 and
|mi(r_b - r_a)| < r_cut[alpha, beta]; all species together), n of them around the centre a with unit legs d_b:

    q_l(a)^2 = 4 pi / (2 l + 1) sum_m |1/n sum_b Y_lm(d_b)|^2 = 1/n^2 (n + 2 sum_{b<c} P_l(cos theta_bc))

the second form by the addition theorem of the spherical harmonics: no spherical harmonic and no reference frame, a
Legendre recurrence on the cosines between pairs of legs.  q_l is rotation invariant, in [0, 1], and a fingerprint of the
shell: (q_4, q_6) = (0.19094, 0.57452) fcc, (0.09722, 0.48476) hcp, (0.50918, 0.62854) the eight of bcc, (0.03637, 0.51069)
its fourteen, (0, 0.66332) the icosahedron, (0.76376, 0.35355) simple cubic.

    counts[alpha, j, i] = #{(a in alpha, origin o): q_{ls[j]}(a, o) in bin i of n_q uniform bins over [0, 1]}

The kernel rounds every P_l to a multiple of 2^-24 and sums integers, X_l = n 2^24 + 2 sum t_l = n^2 2^24 q_l^2, so the
result is the same bits for any blocking, budget and atom order; the bin is found from X_l with integers only.  A centre is
left out of the histograms, all or nothing, when it has more than 64 neighbours (`truncated`; the calculator raises), none
(`isolated`) or a coincident one (`undefined`):

    sum_i counts[alpha, j, i] + truncated[alpha] + isolated[alpha] + undefined[alpha] = n_o N_alpha    for every j

  * Not here: the third-order invariants w_l, the neighbour-averaged q_l of Lechner and Dellago and the solid-like bonds
    are in `psa_amd/local_order.py`, which forms the q_lm vectors.  Left out of both: odd l there, the q_lm of other
    neighbour definitions, Voronoi or solid-angle weights, cluster analysis of the solid-like bonds, cell lists, sharding.

This module is host code only: the result type.  `SEDCalculator.calculate_bond_order` runs the kernels
(psa_amd/csrc/angle.hip's neighbour pass, psa_amd/csrc/order.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from ._hip import ORDER_MAX_BINS, ORDER_MAX_L, ORDER_MAX_LS, ORDER_SHIFT  # noqa: F401
from .pairs import _divide


@dataclass
class BondOrder:
    """Result of `SEDCalculator.calculate_bond_order`: `counts` (S, n_l, n_q) uint64, species x order x bin of q; `ls` (n_l,)
    the orders; `q_edges` (n_q + 1,) and `q` (n_q,) the bins over [0, 1]; `truncated`, `isolated`, `undefined` (S,) uint64
    the (centre, origin) left out; `samples` (S,) = n_o N_alpha; `origins` = n_o; `groups` the atom-index arrays used.  With
    `per_atom`: `q_atoms` (n_o, n_a, n_l) float64 = sqrt(X / (n^2 2^24)), NaN where the centre is left out; `neighbours`
    (n_o, n_a) the true neighbour counts; `atoms` (n_a,) the atom of every column, the groups concatenated; `mean` (S, n_l)
    the mean q_l over the centres counted (NaN for a species with none).  Without: None."""
    counts: np.ndarray
    ls: np.ndarray
    q_edges: np.ndarray
    q: np.ndarray
    truncated: np.ndarray
    isolated: np.ndarray
    undefined: np.ndarray
    samples: np.ndarray
    origins: int
    groups: List[np.ndarray]
    q_atoms: Optional[np.ndarray] = None
    neighbours: Optional[np.ndarray] = None
    atoms: Optional[np.ndarray] = None
    mean: Optional[np.ndarray] = None

    def order(self, l: int) -> int:
        """the column of order l in `counts`, `q_atoms` and `mean`"""
        at = np.flatnonzero(np.asarray(self.ls) == int(l))
        if at.size != 1:
            raise ValueError(f"order {l} is not among ls = {list(map(int, self.ls))}")
        return int(at[0])

    @property
    def density(self) -> np.ndarray:
        """counts normalised to integrate to 1 over q, (S, n_l, n_q) float64; 0 where a species has no centre counted"""
        width = np.diff(np.asarray(self.q_edges, np.float64))[None, None, :]
        return _divide(self.counts, self.counts.sum(axis=-1, dtype=np.uint64)[:, :, None].astype(np.float64) * width)


def q_from_x(x, n) -> np.ndarray:
    """q (n_o, n_a, n_l) float64 = sqrt(x / (n^2 2^24)) of the integers `Engine.bond_order` returns; NaN where x = -1"""
    x = np.asarray(x, np.int64)
    n2 = np.asarray(n, np.int64)[..., None].astype(np.float64) ** 2 * float(1 << ORDER_SHIFT)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x >= 0, np.sqrt(np.maximum(x, 0) / n2), np.nan)


def result(hist, truncated, isolated, undefined, x, n, ls, n_q: int, origins: int, groups) -> BondOrder:
    """the result type from what `Engine.bond_order` returns"""
    edges = np.linspace(0.0, 1.0, int(n_q) + 1)
    sizes = np.array([len(g) for g in groups], np.int64)
    res = BondOrder(np.asarray(hist), np.asarray(ls, np.int64).ravel().copy(), edges, 0.5 * (edges[1:] + edges[:-1]), np.asarray(truncated),
                    np.asarray(isolated), np.asarray(undefined), int(origins) * sizes, int(origins), list(groups))
    if x is None:
        return res
    res.q_atoms, res.neighbours = q_from_x(x, n), np.asarray(n)
    res.atoms = np.concatenate([np.asarray(g, np.int64) for g in groups]) if len(groups) else np.zeros(0, np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])
    res.mean = np.full((len(groups), res.ls.size), np.nan)
    for a in range(len(groups)):
        part = res.q_atoms[:, start[a]:start[a + 1]].reshape(-1, res.ls.size)
        kept = part[~np.isnan(part[:, 0])] if part.size else part
        if kept.size:
            res.mean[a] = kept.mean(axis=0)
    return res
