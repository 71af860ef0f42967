"""
Bond persistence: how long a neighbour stays a neighbour -- the Si-O bond lifetime of a silica melt, the Na-Cl pair residence
time of a molten salt, the time a Li ion keeps its anion cage, the cage-breaking time of a supercooled metal (Rapaport, Mol.
Phys. 50, 1151, 1983, for the two bond correlations; Rabani, Gezelter and Berne, J. Chem. Phys. 107, 6867, 1997, for the
cage correlation).

The inputs are `r_cut`, `r_break`, the lags, `origin_step`, `sample_step` and `continuous`.

  * The neighbours of an atom a at a time origin o are those of `calculate_bond_angles`: b != a of species beta with a
    minimum-image distance below r_cut[alpha, beta], all species together, at most 64; a (centre, origin) with more is left
    out whole and counted in `truncated`.
  * A listed bond (a, b, o) is ALIVE at frame o + f while its distance at that frame is below r_break[alpha, beta] >= r_cut
    (hysteresis: a bond that forms below r_cut is not broken by a vibration across it; the default r_break = r_cut has none).
  * The origins of lag tau are o = 0, origin_step, ... with o + tau <= T - 1.

    bonds[j, alpha, beta]      the bonds listed at the origins of lag j between centres of alpha and neighbours of beta
    alive[j, alpha, beta]      those alive at o + tau_j                           intermittent = alive / bonds
    unbroken[j, alpha, beta]   those alive at every frame o + sample_step, o + 2 sample_step, ... up to o + tau_j
                                                                                  continuous = unbroken / bonds
    lost[j, alpha, m]          the (centre, origin) with exactly m listed neighbours not alive at o + tau_j
                                                                                  cage(c) = sum_{m < c} lost / sum_m lost
    sum_m lost + truncated = n_o(tau_j) N_alpha,   sum_m m lost = sum_beta (bonds - alive),   unbroken <= alive <= bonds

The intermittent correlation lets a bond break and form again, the continuous one does not: its decay time is the bond
lifetime, seen at the resolution `sample_step`.  Every result is an integer count, the same bits for any budget, any blocking
and any order of the atoms inside a species; the correlations are their float64 quotients.

  * Left out: new neighbours entering the shell (the list-changed variant of the cage correlation), first-passage cage
    times, per-bond residence-time histograms, cell lists, sharding.

This module is host code only: the result type.  `SEDCalculator.calculate_bond_persistence` runs the kernels
(psa_amd/csrc/angle.hip's neighbour pass, psa_amd/csrc/persist.hip).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from ._hip import ANGLE_MAX_NEIGHBOURS, PERSIST_MAX_LAGS  # noqa: F401
from .correlations import relaxation_time


@dataclass
class BondPersistence:
    """Result of `SEDCalculator.calculate_bond_persistence`.  Counts, uint64: `bonds`, `alive`, `unbroken` (n_lags, S, S)
    (`unbroken` None when the continuous correlation was not computed), `lost` (n_lags, S, 65), `truncated` (n_lags, S).
    `lags` (n_lags,) int64 in frames, `times` (n_lags,) in ps (in frames without a time step), `origins` (n_lags,) int64 =
    n_o(tau_j), `groups` the atom-index arrays used, `dt_ps`.  With `per_atom`, (n_lags, n_o(0), n_a) uint64: `alive_masks`
    and `unbroken_masks` -- bit i stands for the i-th neighbour of the centre's list at the origin, ascending in the column;
    0 for a truncated centre and for an origin beyond those of the lag --, and `atoms` (n_a,) the atom of every column.
    Without: None."""
    bonds: np.ndarray
    alive: np.ndarray
    unbroken: Optional[np.ndarray]
    lost: np.ndarray
    truncated: np.ndarray
    lags: np.ndarray
    times: np.ndarray
    origins: np.ndarray
    groups: List[np.ndarray]
    dt_ps: Optional[float] = None
    alive_masks: Optional[np.ndarray] = None
    unbroken_masks: Optional[np.ndarray] = None
    atoms: Optional[np.ndarray] = None

    def _share(self, part) -> np.ndarray:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.bonds > 0, part.astype(np.float64) / self.bonds.astype(np.float64), np.nan)

    @property
    def intermittent(self) -> np.ndarray:
        """alive / bonds, (n_lags, S, S) float64: the share of the bonds listed at an origin that are alive a lag later,
        whatever happened in between; NaN where there is no bond"""
        return self._share(self.alive)

    @property
    def continuous(self) -> Optional[np.ndarray]:
        """unbroken / bonds, (n_lags, S, S) float64: the share of the bonds that were alive at every sampled frame up to
        the lag; NaN where there is no bond; None when it was not computed"""
        return None if self.unbroken is None else self._share(self.unbroken)

    def cage(self, c: int = 1) -> np.ndarray:
        """(n_lags, S) float64: the share of the centres counted that lost fewer than `c` of their listed neighbours (c = 1:
        the whole cage is still there); NaN where no centre was counted"""
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or not 1 <= int(c) <= ANGLE_MAX_NEIGHBOURS + 1:
            raise ValueError(f"c must be an integer in [1, {ANGLE_MAX_NEIGHBOURS + 1}], got {c!r}")
        total = self.lost.sum(axis=2, dtype=np.uint64).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(total > 0, self.lost[:, :, :int(c)].sum(axis=2, dtype=np.uint64).astype(np.float64) / total, np.nan)

    def pair(self, a: int, b: int) -> dict:
        """the species pair (centre a, neighbour b): dict of `bonds`, `alive`, `unbroken` (n_lags,) uint64 and `intermittent`,
        `continuous` (n_lags,) float64 (`unbroken`, `continuous` None when not computed)"""
        S = self.bonds.shape[1]
        if not (0 <= int(a) < S and 0 <= int(b) < S):
            raise IndexError(f"species pair ({a!r}, {b!r}) is outside [0, {S})")
        a, b = int(a), int(b)
        cont = self.continuous
        return dict(bonds=self.bonds[:, a, b].copy(), alive=self.alive[:, a, b].copy(),
                    unbroken=None if self.unbroken is None else self.unbroken[:, a, b].copy(), intermittent=self.intermittent[:, a, b],
                    continuous=None if cont is None else cont[:, a, b])

    def lifetime(self, kind: str = "continuous", level: float = 1.0 / math.e) -> np.ndarray:
        """(S, S) float64: the time at which the correlation `kind` ("continuous" or "intermittent"), divided by its value at
        the first lag, first falls to `level` (`psa_amd.relaxation_time`: linear between two lags; NaN where it never does or
        where there is no bond).  List lag 0 first for a correlation that starts at 1."""
        if kind not in ("continuous", "intermittent"):
            raise ValueError(f"kind must be 'continuous' or 'intermittent', got {kind!r}")
        f = self.continuous if kind == "continuous" else self.intermittent
        if f is None:
            raise ValueError("the continuous correlation was not computed: calculate_bond_persistence(..., continuous=True)")
        S = self.bonds.shape[1]
        return relaxation_time(np.nan_to_num(f.reshape(f.shape[0], S * S), nan=0.0), self.times, level).reshape(S, S)


def check_lags(lag_frames, n_frames: int, sample_step: int) -> np.ndarray:
    """`lag_frames` (a scalar or a list) as int64 (n_lags,); ValueError unless they are 1 to 1024 strictly ascending integers
    in [0, T - 1], multiples of `sample_step`"""
    tau = np.asarray(lag_frames)
    if tau.ndim == 0:
        tau = tau.reshape(1)
    if tau.ndim != 1 or tau.dtype.kind == "b" or (tau.size and not (tau.dtype.kind in "iu" or (tau.dtype.kind == "f" and np.all(tau == np.rint(tau))))):
        raise ValueError("lag_frames must be a list of integers")
    tau = tau.astype(np.int64)
    if not 1 <= tau.size <= PERSIST_MAX_LAGS:
        raise ValueError(f"between 1 and {PERSIST_MAX_LAGS} lags are served, got {tau.size}")
    if np.any(np.diff(tau) <= 0):
        raise ValueError("lag_frames must be strictly ascending")
    if np.any(tau < 0) or (n_frames and np.any(tau > n_frames - 1)):
        raise ValueError(f"lag_frames must lie in [0, T - 1 = {n_frames - 1}]")
    if np.any(tau % sample_step):
        raise ValueError(f"every lag must be a multiple of sample_step = {sample_step}")
    return tau


def check_break(r_break, r_cut) -> np.ndarray:
    """`r_break` as an array of r_cut's shape (None: r_cut itself); ValueError unless it is finite, symmetric, at least r_cut
    entry by entry and 0 exactly where r_cut is"""
    rc = np.asarray(r_cut, np.float64)
    if r_break is None:
        return rc
    rb = np.asarray(r_break, np.float64)
    if rb.ndim not in (0, 2) or not np.all(np.isfinite(rb)):
        raise ValueError("r_break must be a scalar or an (S, S) matrix of finite values")
    if rb.ndim == 2 and not np.array_equal(rb, rb.T):
        raise ValueError("r_break must be symmetric")
    if rb.ndim == 2 and rc.ndim == 2 and rb.shape != rc.shape:
        raise ValueError(f"r_break {rb.shape} does not fit r_cut {rc.shape}")
    if rb.ndim == 0 and rc.ndim == 2:
        rb = np.where(rc > 0.0, float(rb), 0.0)               # a scalar r_break keeps r_cut's "no bond" entries
    if np.any(rb < rc):
        raise ValueError("r_break must be at least r_cut, entry by entry")
    if np.any((rb == 0.0) != (rc == 0.0)):
        raise ValueError("r_break must be 0 exactly where r_cut is 0 (no bond between these species)")
    return rb


def empty(S: int, n_lags: int) -> dict:
    """what `Engine.bond_persistence` returns where nothing is listed"""
    pair = lambda: np.zeros((n_lags, S, S), np.uint64)                                                # noqa: E731
    return dict(bonds=pair(), alive=pair(), unbroken=pair(), lost=np.zeros((n_lags, S, ANGLE_MAX_NEIGHBOURS + 1), np.uint64),
                truncated=np.zeros((n_lags, S), np.uint64), alive_masks=None, unbroken_masks=None)


def result(out: dict, lags, origins, groups, dt_ps, continuous: bool) -> BondPersistence:
    """the result type from what `Engine.bond_persistence` returns"""
    tau = np.asarray(lags, np.int64)
    res = BondPersistence(bonds=np.asarray(out["bonds"]), alive=np.asarray(out["alive"]),
                          unbroken=np.asarray(out["unbroken"]) if continuous else None, lost=np.asarray(out["lost"]),
                          truncated=np.asarray(out["truncated"]), lags=tau, times=tau.astype(np.float64) * (dt_ps if dt_ps is not None else 1.0),
                          origins=np.asarray(origins, np.int64), groups=list(groups), dt_ps=dt_ps)
    if out.get("alive_masks") is None:
        return res
    res.alive_masks = np.asarray(out["alive_masks"])
    res.unbroken_masks = np.asarray(out["unbroken_masks"]) if continuous else None
    res.atoms = np.concatenate([np.asarray(g, np.int64) for g in groups]) if len(groups) else np.zeros(0, np.int64)
    return res
