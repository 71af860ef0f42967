"""
Pair distributions in real space: the radial distribution function g(r), its species-resolved partials g_ab(r) with their
running coordination numbers, and the distinct van Hove function G_d(r,t).

With H the box matrix (rows = box vectors, r = s H), species alpha, beta (disjoint atom groups, at most 8), lags tau_j
in frames and the origins O_tau = {0, s, 2 s, ...: o + tau <= T - 1} (s = `origin_step`, n_o = (T - 1 - tau) // s + 1):

    counts[j,a,b,i] = #{(atom A in a, atom B in b, B != A, o in O_tau_j): floor(|mi(r_B(o + tau_j) - r_A(o))| / dr) = i}     i < n_r

`mi` the minimum image; everything at or beyond r_max = n_r dr is counted in `overflow`.  tau = 0 is g(r), tau > 0 is
G_d(r,t); G = G_s + G_d with the self part of `psa_amd.displacements`.  The counts are exact integers: sum_i counts +
overflow = samples = n_o N_a (N_b - delta_ab), and at tau = 0 counts[a,b] = counts[b,a].

  * Nothing is unwrapped, and nothing needs to be: within r_max at most one periodic image of B lies around A, so the
    minimum image of the positions as stored -- wrapped, unwrapped or moved by whole box vectors -- is the distance at
    any lag.  This is the real-space counterpart of "correct on wrapped trajectories as stored".
  * Served radius: with w_j = 1 / |column j of Hinv| the perpendicular widths of the box, rounding the fractional
    difference to the nearest integer gives the true minimum image of every pair closer than min_j w_j / 2, whatever the
    tilt.  `max_pair_radius(box)` = (1/2 - 2^-12) min_j w_j is the largest r_max served; `r_max=None` means that value.
  * g = counts / (n_o N_a rho_b shell volume), rho_b = N_b / V, tends to 1 - delta_ab / N_b for an ideal gas;
    coordination = cumsum(counts) / (n_o N_a) is N_ab(r), the mean number of b-atoms within r of an a-atom.
  * Not here: cell lists for r_max much smaller than the box, S(Q) by transforming g(r), per-frame box changes,
    sharding (bond angles and coordination: psa_amd/angles.py).

This module is host code only: the served radius and the result types.  `SEDCalculator.calculate_rdf` and
`SEDCalculator.calculate_distinct_van_hove` run the kernels (psa_amd/csrc/pair.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

RADIUS_FRACTION = 0.5 - 2.0 ** -12


def max_pair_radius(box) -> float:
    """The largest r_max the pair histograms serve for the (3, 3) box matrix `box` (rows = box vectors, taken as float32
    like the calculator takes it): (1/2 - 2^-12) of the least perpendicular width 1 / |column j of Hinv|.  ValueError for
    a box that is not (3, 3), not finite or singular."""
    H = np.asarray(box, np.float32).astype(np.float64)
    if H.shape != (3, 3) or not np.all(np.isfinite(H)):
        raise ValueError(f"box must be a finite (3, 3) matrix, got shape {H.shape}")
    try:
        inv = np.linalg.inv(H)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"the box is singular: {e}") from None
    if not np.all(np.isfinite(inv)):
        raise ValueError("the box is singular")
    return float(RADIUS_FRACTION / np.sqrt((inv * inv).sum(axis=0)).max())


def _shell_volumes(r_edges) -> np.ndarray:
    e = np.asarray(r_edges, np.float64)
    return (4.0 * np.pi / 3.0) * (e[1:] ** 3 - e[:-1] ** 3)


def _divide(counts, denom) -> np.ndarray:
    """counts / denom in float64, 0 where denom is 0 (an empty species)"""
    out = np.zeros(np.shape(counts), np.float64)
    d = np.broadcast_to(np.asarray(denom, np.float64), out.shape)
    np.divide(np.asarray(counts, np.float64), d, out=out, where=d > 0)
    return out


@dataclass
class RadialDistribution:
    """Result of `SEDCalculator.calculate_rdf`: `counts` (S, S, n_r) uint64 over ordered species pairs and `overflow`
    (S, S) uint64 (the pairs at r_max and beyond); `samples` (S, S) = n_o N_a (N_b - delta_ab) = counts.sum(-1) +
    overflow; `r_edges` (n_r + 1,), `r` (n_r,) the bin centres; `volume` of the box; `groups` the atom-index arrays
    used, `group_sizes` (S,); `origins` = n_o."""
    counts: np.ndarray
    overflow: np.ndarray
    samples: np.ndarray
    r_edges: np.ndarray
    r: np.ndarray
    volume: float
    groups: List[np.ndarray]
    group_sizes: np.ndarray
    origins: int

    def _per_atom(self) -> np.ndarray:
        """n_o N_a, shaped to divide counts"""
        return (float(self.origins) * np.asarray(self.group_sizes, np.float64))[:, None, None]

    @property
    def g(self) -> np.ndarray:
        """g_ab(r) = counts / (n_o N_a rho_b shell volume), rho_b = N_b / V: (S, S, n_r) float64"""
        rho = np.asarray(self.group_sizes, np.float64)[None, :, None] / float(self.volume)
        return _divide(self.counts, self._per_atom() * rho * _shell_volumes(self.r_edges)[None, None, :])

    @property
    def coordination(self) -> np.ndarray:
        """N_ab(r) = cumsum(counts) / (n_o N_a) at the bins' upper edges r_edges[1:]: (S, S, n_r) float64"""
        return _divide(np.cumsum(self.counts, axis=-1, dtype=np.uint64), self._per_atom())

    def pair(self, a: int, b: int) -> np.ndarray:
        """g_ab(r) of one ordered species pair, (n_r,)"""
        return self.g[a, b]


@dataclass
class VanHoveDistinct:
    """Result of `SEDCalculator.calculate_distinct_van_hove`: `counts` (n_vh, S, S, n_r) uint64, `overflow` and `samples`
    (n_vh, S, S), `origins` (n_vh,) = n_o(tau_j), `lag_frames` (n_vh,), `times` = lag_frames dt_ps; the rest as
    `RadialDistribution`.  The (a, b) and (b, a) counts differ at tau > 0."""
    counts: np.ndarray
    overflow: np.ndarray
    samples: np.ndarray
    r_edges: np.ndarray
    r: np.ndarray
    volume: float
    groups: List[np.ndarray]
    group_sizes: np.ndarray
    origins: np.ndarray
    lag_frames: np.ndarray
    times: np.ndarray
    dt_ps: Optional[float] = None

    def _per_atom(self) -> np.ndarray:
        return np.asarray(self.origins, np.float64)[:, None, None, None] * np.asarray(self.group_sizes, np.float64)[None, :, None, None]

    @property
    def g_d(self) -> np.ndarray:
        """G_d(r,t) / rho_b = counts / (n_o N_a rho_b shell volume): tends to 1 at large r and long times"""
        rho = np.asarray(self.group_sizes, np.float64)[None, None, :, None] / float(self.volume)
        return _divide(self.counts, self._per_atom() * rho * _shell_volumes(self.r_edges)[None, None, None, :])

    @property
    def radial_density(self) -> np.ndarray:
        """counts / (n_o N_a dr) = 4 pi r^2 G_d(r,t): the number of b-atoms per unit r around an a-atom's place at t = 0"""
        return _divide(self.counts, self._per_atom() * np.diff(np.asarray(self.r_edges, np.float64))[None, None, None, :])

    @property
    def coordination(self) -> np.ndarray:
        """cumsum(counts) / (n_o N_a) at the bins' upper edges"""
        return _divide(np.cumsum(self.counts, axis=-1, dtype=np.uint64), self._per_atom())

    def pair(self, a: int, b: int) -> np.ndarray:
        """g_d of one ordered species pair, (n_vh, n_r)"""
        return self.g_d[:, a, b]
