"""
Common-neighbour analysis (Honeycutt and Andersen, J. Phys. Chem. 91, 4950, 1987; Faken and Jonsson, Comput. Mater. Sci. 2,
279, 1994): which crystal structure an atom is in, and the signature of every bond -- the first structure-identification
step of MD post-processing.  The share of the (5,5,5), (5,4,4) and (4,3,3) bonds is the usual measure of icosahedral order in
a metallic glass; the census of fcc and hcp atoms over time follows a crystallisation or a stacking fault.

The input is `r_cut` alone.

  * The neighbours are those of `calculate_bond_angles`: all species together, at most 64; a centre with more is left out
    whole (`truncated`).
  * Two neighbours of a centre are bonded by the same test (their own species' entry of `r_cut`), so the adjacency is what the
    neighbour lists themselves hold.
  * The bond a-b has the signature (j, k, l): j the common neighbours of a and b, k the bonds among those, l the bonds of the
    largest connected piece of that bond graph (the "longest chain" of the widely used implementations: a star of three
    bonds has l = 3).
  * The type of a centre with n neighbours:

        1 fcc    n = 12, 12 x (4,2,1)                  3 bcc    n = 14, 8 x (6,6,6) + 6 x (4,4,4)
        2 hcp    n = 12, 6 x (4,2,1) + 6 x (4,2,2)     4 ico    n = 12, 12 x (5,5,5)
        0 other  anything else

    bcc needs a cut-off between the second and the third shell, (1 + sqrt 2) / 2 of the lattice constant say; fcc, hcp and ico
    one between the first and the second.

Everything is integers, per time origin and on positions as stored: the same bits for any budget, any blocking, two
identical calls and any order of the atoms inside a species.

    signature_counts[alpha, j, k, l]    the bonds of the centres of species alpha with that signature, over all origins
    sum signature_counts[alpha] + signature_outside[alpha] = sum_n n coordination_counts[alpha, :, n] of calculate_bond_angles
    sum_t type_counts[o, alpha, t] + the centres of alpha truncated at o = N_alpha

  * Left out: diamond identification, signature tables resolved by the species pair of the bond (`bond_signatures` with the
    neighbour lists give them on the host), cell lists, sharding.  Adaptive CNA (a cut-off per atom from its sorted
    neighbours): psa_amd/acna.py.

This module is host code only: the result type.  `SEDCalculator.calculate_common_neighbours` runs the kernels
(psa_amd/csrc/angle.hip's neighbour pass, psa_amd/csrc/cna.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from ._hip import ANGLE_MAX_NEIGHBOURS, CNA_TABLE, CNA_TYPES  # noqa: F401

NO_BOND = 0xFFFFFFFF


def pack(j: int, k: int, l: int) -> int:
    """the word of `bond_signatures` for the signature (j, k, l): j | k << 8 | l << 16, k and l clamped to 255"""
    return int(j) | min(int(k), 255) << 8 | min(int(l), 255) << 16


@dataclass
class CommonNeighbours:
    """Result of `SEDCalculator.calculate_common_neighbours`.  Counts, uint64: `signature_counts` (S, 8, 16, 16) per species of
    the centre, `signature_outside` (S,) the bonds whose signature the table does not hold, `type_counts` (n_o, S, 5) the
    centres by type at every origin, `truncated` (S,).  `structure_names` the names of the five types; `sizes` (S,) the
    atoms of every species; `origins` = n_o; `groups` the atom-index arrays used.  With `per_atom`: `types` (n_o, n_a) int32
    (-1: truncated), `neighbours` (n_o, n_a) int32 the true neighbour counts, `bond_signatures` (n_o, n_a, 64) uint32 (`pack`
    of the bond to the i-th neighbour in list order, 0xFFFFFFFF: no bond), `atoms` (n_a,) the atom of every column.  Without:
    None."""
    signature_counts: np.ndarray
    signature_outside: np.ndarray
    type_counts: np.ndarray
    truncated: np.ndarray
    sizes: np.ndarray
    origins: int
    groups: List[np.ndarray]
    structure_names: Tuple[str, ...] = CNA_TYPES
    types: Optional[np.ndarray] = None
    neighbours: Optional[np.ndarray] = None
    bond_signatures: Optional[np.ndarray] = None
    atoms: Optional[np.ndarray] = None

    def _type(self, kind) -> int:
        if isinstance(kind, str):
            if kind not in self.structure_names:
                raise ValueError(f"type must be one of {self.structure_names} or 0 .. {len(self.structure_names) - 1}, got {kind!r}")
            return self.structure_names.index(kind)
        if isinstance(kind, (bool, np.bool_)) or not isinstance(kind, (int, np.integer)) or not 0 <= int(kind) < len(self.structure_names):
            raise ValueError(f"type must be one of {self.structure_names} or 0 .. {len(self.structure_names) - 1}, got {kind!r}")
        return int(kind)

    def fraction(self, kind) -> np.ndarray:
        """(n_o, S) float64: the share of the atoms of every species that are of this type (a name or a code) at every origin
        -- the crystallisation time series; a truncated centre counts as none; NaN for an empty species"""
        t = self._type(kind)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.sizes[None, :] > 0, self.type_counts[:, :, t].astype(np.float64) / self.sizes[None, :].astype(np.float64), np.nan)

    def signature(self, j: int, k: int, l: int) -> np.ndarray:
        """(S,) uint64: the bonds with the signature (j, k, l) per species of the centre, over all origins"""
        if not all(isinstance(v, (int, np.integer)) and 0 <= int(v) < cap for v, cap in zip((j, k, l), CNA_TABLE)):
            raise ValueError(f"the table holds j < {CNA_TABLE[0]}, k < {CNA_TABLE[1]}, l < {CNA_TABLE[2]}, got {(j, k, l)!r}")
        return self.signature_counts[:, int(j), int(k), int(l)].copy()

    @property
    def bonds(self) -> np.ndarray:
        """(S,) uint64: all bonds of the centres counted, the table's and those outside it"""
        return self.signature_counts.reshape(self.signature_counts.shape[0], -1).sum(axis=1, dtype=np.uint64) + self.signature_outside

    def share(self, j: int, k: int, l: int) -> float:
        """the signature's share of all bonds, all species together (the 555 share of a glass); NaN without a bond"""
        total = int(self.bonds.sum(dtype=np.uint64))
        return float(int(self.signature(j, k, l).sum(dtype=np.uint64)) / total) if total else float("nan")

    def atoms_of(self, origin: int, kind) -> np.ndarray:
        """the atom indices of this type at time origin `origin`, ascending in the column.  Needs `per_atom`."""
        if self.types is None:
            raise ValueError("atoms_of needs the per-atom output: calculate_common_neighbours(..., per_atom=True)")
        o = int(origin)
        if not 0 <= o < self.origins:
            raise IndexError(f"origin {origin!r} is outside [0, {self.origins})")
        return self.atoms[np.flatnonzero(self.types[o] == self._type(kind))]


def empty(S: int, n_o: int = 0) -> dict:
    """what `Engine.common_neighbours` returns where nothing is listed"""
    return dict(signature_counts=np.zeros((S,) + CNA_TABLE, np.uint64), signature_outside=np.zeros(S, np.uint64),
                type_counts=np.zeros((n_o, S, len(CNA_TYPES)), np.uint64), truncated=np.zeros(S, np.uint64), types=None, n=None,
                bond_signatures=None)


def result(out: dict, origins: int, groups) -> CommonNeighbours:
    """the result type from what `Engine.common_neighbours` returns"""
    res = CommonNeighbours(signature_counts=np.asarray(out["signature_counts"]), signature_outside=np.asarray(out["signature_outside"]),
                           type_counts=np.asarray(out["type_counts"]), truncated=np.asarray(out["truncated"]),
                           sizes=np.array([len(g) for g in groups], np.int64), origins=int(origins), groups=list(groups))
    if out.get("types") is None:
        return res
    res.types, res.neighbours, res.bond_signatures = np.asarray(out["types"]), np.asarray(out["n"]), np.asarray(out["bond_signatures"])
    res.atoms = np.concatenate([np.asarray(g, np.int64) for g in groups]) if len(groups) else np.zeros(0, np.int64)
    return res
