"""
Adaptive common-neighbour analysis (Stukowski, Modelling Simul. Mater. Sci. Eng. 20, 045021, 2012): the structure type of
every atom without a cut-off to tune.  The plain analysis (psa_amd/cna.py) needs one `r_cut` that for bcc must fall into a
window a few percent wide; here every atom derives its own from its nearest neighbours, so a melt that crystallises while its
density changes, a strained or thermally expanded crystal, an fcc/bcc two-phase sample or an NPT run need none.

The input is `r_cut` alone, now a generous candidate radius: it must contain the 14 nearest atoms of every centre (up to the
third shell, usually) and not more than 64.

  * The candidates are the neighbours of `calculate_bond_angles` for `r_cut`: all species together, at most 64; a centre with
    more is left out whole (`truncated`), one with fewer than 12 is `other` without bonds (`short`).
  * The candidates are ranked by distance, a tie going to the earlier atom of the list.
  * Test A: the 12 nearest; their cut-off is (1 + sqrt 2) / 2 times their mean distance -- halfway between the first and
    the second shell of fcc --; two of them are bonded when their own minimum-image distance is below it.  The signatures
    (j, k, l) of the 12 bonds centre-member are those of `calculate_common_neighbours`:

        1 fcc    12 x (4,2,1)          2 hcp    6 x (4,2,1) + 6 x (4,2,2)          4 ico    12 x (5,5,5)

  * Test B, where test A found none of these and there are 14 candidates: the 14 nearest; the cut-off is (1 + sqrt 2) / 2
    times the mean of the 8 nearest distances times 2 / sqrt 3 and the 6 next -- the lattice constant of bcc from both shells:

        3 bcc    8 x (6,6,6) + 6 x (4,4,4)          0 other    anything else

  * The bonds counted, the per-atom rows and `cutoffs` of a centre are those of the test that ran last, indexed by rank.

Everything after the adjacency is integers: the same bits for any budget, any blocking and two identical calls.

    sum_t type_counts[o, alpha, t] + the centres of alpha truncated at o = N_alpha
    sum signature_counts[alpha] + signature_outside[alpha] = 12 #(centres whose last test is A) + 14 #(B)

  * Left out: diamond identification, signature tables resolved by the species pair of the bond, cell lists, sharding.

This module is host code only: the result type.  `SEDCalculator.calculate_adaptive_common_neighbours` runs the kernels
(psa_amd/csrc/angle.hip's neighbour pass, psa_amd/csrc/acna.hip, psa_amd/csrc/cna.hip's census).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._hip import ACNA_MEMBERS, CNA_TABLE, CNA_TYPES  # noqa: F401
from .cna import NO_BOND, CommonNeighbours, pack  # noqa: F401


@dataclass
class AdaptiveCommonNeighbours(CommonNeighbours):
    """Result of `SEDCalculator.calculate_adaptive_common_neighbours`: the fields and methods of `CommonNeighbours` --
    `signature_counts` (S, 8, 16, 16), `signature_outside` (S,), `type_counts` (n_o, S, 5), `truncated` (S,), uint64;
    `structure_names`, `sizes`, `origins`, `groups`; `fraction`, `signature`, `bonds`, `share`, `atoms_of` -- and `short` (S,)
    uint64, the centres with fewer than 12 candidates.  With `per_atom`: `types` (n_o, n_a) int32 (-1: truncated),
    `neighbours` (n_o, n_a) int32 the true candidate counts, `cutoffs` (n_o, n_a) float32 the cut-off of the test that ran
    last (NaN: none ran), `nearest` (n_o, n_a, 14) int32 the members by rank as columns of `atoms` (-1 beyond the last test's
    members), `bond_signatures` (n_o, n_a, 14) uint32 (`pack` of the bond to that member, 0xFFFFFFFF: no bond), `atoms`
    (n_a,).  Without: None."""
    short: Optional[np.ndarray] = None
    cutoffs: Optional[np.ndarray] = None
    nearest: Optional[np.ndarray] = None

    def atoms_of(self, origin: int, kind) -> np.ndarray:
        """the atom indices of this type at time origin `origin`, ascending in the column.  Needs `per_atom`."""
        if self.types is None:
            raise ValueError("atoms_of needs the per-atom output: calculate_adaptive_common_neighbours(..., per_atom=True)")
        return super().atoms_of(origin, kind)


def empty(S: int, n_o: int = 0) -> dict:
    """what `Engine.adaptive_common_neighbours` returns where nothing is listed"""
    return dict(signature_counts=np.zeros((S,) + CNA_TABLE, np.uint64), signature_outside=np.zeros(S, np.uint64),
                type_counts=np.zeros((n_o, S, len(CNA_TYPES)), np.uint64), truncated=np.zeros(S, np.uint64),
                short=np.zeros(S, np.uint64), types=None, n=None, cutoffs=None, nearest=None, bond_signatures=None)


def result(out: dict, origins: int, groups) -> AdaptiveCommonNeighbours:
    """the result type from what `Engine.adaptive_common_neighbours` returns"""
    res = AdaptiveCommonNeighbours(signature_counts=np.asarray(out["signature_counts"]),
                                   signature_outside=np.asarray(out["signature_outside"]), type_counts=np.asarray(out["type_counts"]),
                                   truncated=np.asarray(out["truncated"]), sizes=np.array([len(g) for g in groups], np.int64),
                                   origins=int(origins), groups=list(groups), short=np.asarray(out["short"]))
    if out.get("types") is None:
        return res
    res.types, res.neighbours, res.bond_signatures = np.asarray(out["types"]), np.asarray(out["n"]), np.asarray(out["bond_signatures"])
    res.cutoffs, res.nearest = np.asarray(out["cutoffs"]), np.asarray(out["nearest"])
    res.atoms = np.concatenate([np.asarray(g, np.int64) for g in groups]) if len(groups) else np.zeros(0, np.int64)
    return res
