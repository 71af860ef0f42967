"""
Solid-like clusters: the connected components of the solid atoms over the neighbour lists, per time origin (ten Wolde,
Ruiz-Montero and Frenkel, J. Chem. Phys. 104, 9932, 1996) -- what `psa_amd/local_order.py`'s solid-like bonds are computed
for.  The size of the largest cluster, n_max(t) = `largest`, is the order parameter of a nucleation study; the cluster-size
distribution N(n) = `mean_size_counts` gives the nucleation free energy -kT ln(N(n) / N).

The inputs are `r_cut`, `solid_l`, `solid_threshold`, `min_connections` and `link`.

  * The neighbours are those of `calculate_local_order`: all species together, at most 64.
  * xi(a) is its number of solid-like bonds, by its exact rule and its exact arithmetic (the order `solid_l`, the threshold
    `solid_threshold`); xi(a) is -1 for a centre that is truncated, isolated, undefined or incomplete.
  * a is solid when xi(a) >= `min_connections`.
  * Two solid atoms a != b are joined when b is in a's list or a is in b's.  With `link="solid_bonds"` the bond, in whichever
    list holds it, must also be solid-like; the default `link="neighbours"` is the criterion of ten Wolde, Ruiz-Montero and
    Frenkel.
  * A cluster is a connected component of solid atoms.  Its label is the smallest column of its members; a column is the
    position in the concatenated atom list, as `LocalOrder.atoms` uses.
  * Atoms that are not solid have label -1 and size 0.

Everything is per time origin and on positions as stored.  The lists are minimum-image, so a cluster runs through the
periodic boundary.  Every result is an integer: a label is a minimum and a size a sum, the same bits for any budget, any
launch order and two identical calls; a permutation of the atoms gives the same partition.

    size_counts[s]      over all origins the clusters of exactly s atoms, 1 <= s <= n_sizes; slot n_sizes + 1 the larger
                        ones, slot 0 stays 0;  large_atoms  the atoms in the larger ones
    sum_s s size_counts[s] (exact slots) + large_atoms = sum_o n_solid[o],      sum_s size_counts[s] = sum_o n_clusters[o]
    connections[alpha, i]   (a in alpha, origin) with exactly i solid-like bonds, as `LocalOrder.connections`
    sum_i connections[alpha, i] + truncated + isolated + undefined + incomplete = n_o N_alpha

  * Left out: cluster shape descriptors (the gyration tensor), tracking a cluster across frames, cell lists, sharding.

This module is host code only: the result type.  `SEDCalculator.calculate_solid_clusters` runs the kernels
(psa_amd/csrc/angle.hip's neighbour pass, psa_amd/csrc/qlm.hip's first pass, psa_amd/csrc/cluster.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from ._hip import ANGLE_MAX_NEIGHBOURS, CLUSTER_LINKS, CLUSTER_MAX_SIZES, CLUSTER_ROW_WORDS  # noqa: F401


@dataclass
class SolidClusters:
    """Result of `SEDCalculator.calculate_solid_clusters`.  Counts: `size_counts` (n_sizes + 2,) uint64, `large_atoms` int,
    `sizes` (n_sizes + 2,) the s axis (the last entry stands for "more than n_sizes").  Per origin, (n_o,) int32: `n_solid`,
    `n_clusters`, `largest` (0: no cluster) and `largest_label` (the smallest label among the clusters of that size, -1:
    none).  Species rows: `connections` (S, 65) and `truncated`, `isolated`, `undefined`, `incomplete` (S,) uint64;
    `samples` (S,) = n_o N_alpha; `origins` = n_o; `groups` the atom-index arrays used; the parameters `solid_l`,
    `solid_threshold`, `min_connections`, `link`, `n_sizes`.  With `per_atom`, (n_o, n_a): `labels` int32 (-1: not solid),
    `size_atoms` int32 (the size of the atom's cluster, 0: not solid), `connections_atoms` int32 (xi, -1: left out),
    `neighbours` int32 the true neighbour counts, `bond_masks` uint64 (bit b: the bond to the b-th neighbour of the list is
    solid-like); `atoms` (n_a,) the atom of every column.  Without: None."""
    size_counts: np.ndarray
    large_atoms: int
    sizes: np.ndarray
    n_solid: np.ndarray
    n_clusters: np.ndarray
    largest: np.ndarray
    largest_label: np.ndarray
    connections: np.ndarray
    truncated: np.ndarray
    isolated: np.ndarray
    undefined: np.ndarray
    incomplete: np.ndarray
    samples: np.ndarray
    origins: int
    groups: List[np.ndarray]
    solid_l: int = 6
    solid_threshold: float = 0.7
    min_connections: int = 7
    link: str = "neighbours"
    n_sizes: int = 256
    labels: Optional[np.ndarray] = None
    size_atoms: Optional[np.ndarray] = None
    connections_atoms: Optional[np.ndarray] = None
    neighbours: Optional[np.ndarray] = None
    bond_masks: Optional[np.ndarray] = None
    atoms: Optional[np.ndarray] = None

    @property
    def mean_size_counts(self) -> np.ndarray:
        """size_counts / origins: N(n), the mean number of clusters of n atoms in a frame; NaN without an origin"""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.size_counts.astype(np.float64) / np.float64(self.origins)

    @property
    def solid_fraction(self) -> np.ndarray:
        """(S,) float64: the share of the centres counted that are solid (xi >= min_connections); NaN for a species with no
        centre counted"""
        total = self.connections.sum(axis=1, dtype=np.uint64).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(total > 0, self.connections[:, self.min_connections:].sum(axis=1, dtype=np.uint64).astype(np.float64) / total,
                            np.nan)

    def largest_atoms(self, origin: int) -> np.ndarray:
        """the atom indices of the largest cluster at time origin `origin` (the one `largest_label` names), ascending in the
        column; empty where there is no cluster.  Needs `per_atom`."""
        if self.labels is None:
            raise ValueError("largest_atoms needs the per-atom output: calculate_solid_clusters(..., per_atom=True)")
        o = int(origin)
        if not 0 <= o < self.origins:
            raise IndexError(f"origin {origin!r} is outside [0, {self.origins})")
        label = int(self.largest_label[o])
        if label < 0:
            return np.zeros(0, np.int64)
        return self.atoms[np.flatnonzero(self.labels[o] == label)]


def link_code(link) -> int:
    """0 for "neighbours", 1 for "solid_bonds" """
    if not isinstance(link, str) or link not in CLUSTER_LINKS:
        raise ValueError(f"link must be one of {CLUSTER_LINKS}, got {link!r}")
    return CLUSTER_LINKS.index(link)


def split_rows(rows) -> dict:
    """the parts of the (S, 69) species rows `Engine.solid_clusters` returns, by name"""
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != CLUSTER_ROW_WORDS:
        raise ValueError(f"rows of {rows.shape} are not (S, {CLUSTER_ROW_WORDS})")
    at = ANGLE_MAX_NEIGHBOURS + 1
    return dict(connections=rows[:, :at].copy(), truncated=rows[:, at].copy(), isolated=rows[:, at + 1].copy(),
                undefined=rows[:, at + 2].copy(), incomplete=rows[:, at + 3].copy())


def empty(S: int, n_sizes: int, n_o: int = 0) -> dict:
    """what `Engine.solid_clusters` returns where nothing is listed"""
    return dict(species_rows=np.zeros((S, CLUSTER_ROW_WORDS), np.uint64), size_counts=np.zeros(int(n_sizes) + 2, np.uint64), large_atoms=0,
                n_solid=np.zeros(n_o, np.int32), n_clusters=np.zeros(n_o, np.int32), largest=np.zeros(n_o, np.int32),
                largest_label=np.full(n_o, -1, np.int32), labels=None, size_atoms=None, connections=None, n=None, bond_masks=None)


def result(out: dict, solid_l: int, solid_threshold: float, min_connections: int, link: str, n_sizes: int, origins: int, groups) -> SolidClusters:
    """the result type from what `Engine.solid_clusters` returns"""
    sizes = np.array([len(g) for g in groups], np.int64)
    res = SolidClusters(size_counts=np.asarray(out["size_counts"]), large_atoms=int(out["large_atoms"]), sizes=np.arange(int(n_sizes) + 2),
                        n_solid=np.asarray(out["n_solid"]), n_clusters=np.asarray(out["n_clusters"]), largest=np.asarray(out["largest"]),
                        largest_label=np.asarray(out["largest_label"]), samples=int(origins) * sizes, origins=int(origins), groups=list(groups),
                        solid_l=int(solid_l), solid_threshold=float(solid_threshold), min_connections=int(min_connections), link=str(link),
                        n_sizes=int(n_sizes), **split_rows(out["species_rows"]))
    if out.get("labels") is None:
        return res
    res.labels, res.size_atoms = np.asarray(out["labels"]), np.asarray(out["size_atoms"])
    res.connections_atoms, res.neighbours, res.bond_masks = np.asarray(out["connections"]), np.asarray(out["n"]), np.asarray(out["bond_masks"])
    res.atoms = np.concatenate([np.asarray(g, np.int64) for g in groups]) if len(groups) else np.zeros(0, np.int64)
    return res
