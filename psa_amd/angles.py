"""
Bond-angle distributions and coordination statistics: the three-body side of the real-space structure, from the neighbour
shell of every atom in every frame.

With H the box matrix (rows = box vectors), species alpha, beta (disjoint atom groups, at most 8), a symmetric matrix of
cut-offs r_cut[alpha, beta] (0: no bond) and the origins o = 0, s, 2 s, ... <= T - 1 (s = `origin_step`):

    b in beta is a neighbour of a in alpha at o   when b != a, r_cut[alpha, beta] > 0 and |mi(r_b(o) - r_a(o))| < r_cut[alpha, beta]
    counts[alpha, p, i] = #{(a in alpha, o, unordered neighbours {b, c} of a with species pair p): the angle b-a-c in bin i}
    coordination_counts[alpha, beta, n] = #{(a in alpha, o): a has exactly n neighbours of species beta}

`mi` the minimum image of the positions as stored (nothing is unwrapped, see psa_amd/pairs.py); p runs over the species
pairs beta <= gamma in the upper-triangle row-major order of `PartialSpectra.pairs`; the bins are uniform in the angle
over [0, 180] degrees.  A neighbour that coincides with its centre has no angle: such pairs are counted in `undefined`.
The counts are exact integers:

    sum_i counts[alpha, p(beta, beta)] + undefined = sum_n coordination_counts[alpha, beta, n] n (n - 1) / 2
    sum_n coordination_counts[alpha, beta, n] + truncated[alpha] = n_o N_alpha

  * Capacity: a centre holds at most ANGLE_MAX_NEIGHBOURS = 64 neighbours, all species together.  A (centre, origin) with
    more is left out of both histograms, all or nothing, and counted in `truncated`; the calculator raises where that
    happens, since it means r_cut reaches far beyond the first shell.
  * The cut-offs are held to the served radius of the pair histograms, `max_pair_radius(box)`.
  * With one scalar cut-off the neighbours are bit for bit the pairs `calculate_rdf` counts below r_cut.
  * Not here: cell lists for r_cut much smaller than the box, bond-length-resolved angle maps, ring statistics (the
    Steinhardt order parameters of the same shells: psa_amd/order.py), time-lagged neighbour persistence, `max_atoms` sampling, sharding.

This module is host code only: the result type.  `SEDCalculator.calculate_bond_angles` runs the kernels
(psa_amd/csrc/angle.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np

from ._hip import ANGLE_MAX_BINS, ANGLE_MAX_NEIGHBOURS  # noqa: F401
from .pairs import _divide
from .partial import pair_row, pair_table


@dataclass
class BondAngleDistribution:
    """Result of `SEDCalculator.calculate_bond_angles`: `counts` (S, P, n_theta) uint64, centre species x neighbour
    species pair x angle bin, and `undefined` (S, P) uint64 (pairs with a neighbour on top of its centre); `theta_edges`
    (n_theta + 1,) and `theta` (n_theta,) in degrees; `pairs` (P, 2) the species pairs (b, c), b <= c, as `PartialSpectra.pairs`;
    `coordination_counts` (S, S, 65) uint64; `truncated` (S,) uint64 the (centre, origin) left out for more than 64
    neighbours; `samples` (S,) = n_o N_alpha; `origins` = n_o; `groups` the atom-index arrays used."""
    counts: np.ndarray
    undefined: np.ndarray
    theta_edges: np.ndarray
    theta: np.ndarray
    pairs: np.ndarray
    coordination_counts: np.ndarray
    truncated: np.ndarray
    samples: np.ndarray
    origins: int
    groups: List[np.ndarray]

    def triplet(self, centre: int, b: int, c: int) -> np.ndarray:
        """the counts of the angle b-centre-c, (n_theta,); either order of b, c"""
        return self.counts[centre, pair_row(b, c, self.counts.shape[0])]

    @property
    def density(self) -> np.ndarray:
        """counts normalised to integrate to 1 over degrees, (S, P, n_theta) float64; 0 where a triplet has no sample"""
        width = np.diff(np.asarray(self.theta_edges, np.float64))[None, None, :]
        return _divide(self.counts, self.counts.sum(axis=-1, dtype=np.uint64)[:, :, None].astype(np.float64) * width)

    @property
    def coordination_fraction(self) -> np.ndarray:
        """coordination_counts / the centres counted: (S, S, 65) float64, the fraction of alpha-atoms with n beta-neighbours"""
        return _divide(self.coordination_counts, self.coordination_counts.sum(axis=-1, dtype=np.uint64)[:, :, None])

    @property
    def mean_coordination(self) -> np.ndarray:
        """(S, S) float64: the mean number of beta-neighbours of an alpha-atom"""
        n = np.arange(self.coordination_counts.shape[-1], dtype=np.float64)
        return (self.coordination_fraction * n[None, None, :]).sum(axis=-1)


def distribution(angles, coord, truncated, n_theta: int, origins: int, groups) -> BondAngleDistribution:
    """the result type from what `Engine.angle_histogram` returns"""
    S = len(groups)
    edges = np.linspace(0.0, 180.0, int(n_theta) + 1)
    sizes = np.array([len(g) for g in groups], np.int64)
    return BondAngleDistribution(np.ascontiguousarray(angles[:, :, :n_theta]), np.ascontiguousarray(angles[:, :, n_theta]), edges,
                                 0.5 * (edges[1:] + edges[:-1]), pair_table(S), np.asarray(coord), np.asarray(truncated),
                                 int(origins) * sizes, int(origins), list(groups))
