"""
Dynamic heterogeneity in real space: the self-overlap function and the four-point susceptibility chi_4(t).

With the unwrapped displacements u of `psa_amd.displacements`, a cut-off length a and the time origins o_k = k s
(s = `origin_step`, k < n_o(t) = (T - 1 - t) // s + 1), the self-overlap of group g at the origin o_k and the lag t is

    Q[t,g,k] = number of atoms a of g with |u[o_k + t, a] - u[o_k, a]| < a

-- the atoms that have not left the neighbourhood they were in.  Its mean over the origins is the overlap function
q(t) = <Q> / N_g, which falls from 1 to 0 with the structural relaxation; its variance over the origins is the
four-point susceptibility

    chi4[t,g] = (<Q^2> - <Q>^2) / N_g = (n_o S2 - S1^2) / (n_o^2 N_g),      S1 = sum_k Q,  S2 = sum_k Q^2.

chi_4(t) peaks at the lifetime t* of the dynamic heterogeneity, and the peak height counts the atoms that move together.

  * Everything the GPU returns is an integer: Q (uint32), S1 and S2 (uint64).  S1 is, bit for bit, bin 0 of
    `SEDCalculator.calculate_van_hove` with one bin of width a; the numerator of chi4 is formed in Python integers, so it
    is exact, and only the last division rounds.
  * The variance is taken over the origins used, which overlap in time: neighbouring origins are correlated, so the
    estimate is that of the population variance over the trajectory (divisor n_o, not n_o - 1), and its own statistical
    error falls with the number of independent windows T / t, not with n_o.  With one origin it is 0.
  * a is customarily 0.3 of the nearest-neighbour distance.
  * Not here: the distinct part of the overlap (a pair pass per origin and lag), chi_4 of F_s(k,t), block averaging of
    the variance, per-atom mobility flags, sharding.

This module is host code only: the result type.  `SEDCalculator.calculate_overlap` runs the kernels
(psa_amd/csrc/overlap.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .correlations import relaxation_time


@dataclass
class DynamicOverlap:
    """Result of `SEDCalculator.calculate_overlap`: `sum` and `sum_squares` (n_lags, G) uint64, S1 = sum_k Q and
    S2 = sum_k Q^2 over the origins; `origins` (n_lags,) = n_o(t); `counts` (G,) = N_g; `cutoff`; `lag_frames` (n_lags,),
    `times` = lag_frames dt_ps; `groups` the atom-index arrays used; `q_origins` (n_lags, G, n_o_max) uint32, Q itself
    (zero beyond a lag's origins), when the call asked for it with `per_origin=True`, else None."""
    sum: np.ndarray
    sum_squares: np.ndarray
    origins: np.ndarray
    counts: np.ndarray
    cutoff: float
    lag_frames: np.ndarray
    times: np.ndarray
    groups: List[np.ndarray]
    q_origins: Optional[np.ndarray] = None
    dt_ps: Optional[float] = None

    @property
    def q(self) -> np.ndarray:
        """The overlap function q(t) = S1 / (n_o N_g), (n_lags, G) float64; NaN for an empty group"""
        den = np.asarray(self.origins, np.float64)[:, None] * np.asarray(self.counts, np.float64)[None, :]
        out = np.full(den.shape, np.nan)
        np.divide(np.asarray(self.sum, np.float64), den, out=out, where=den > 0)
        return out

    @property
    def chi4(self) -> np.ndarray:
        """The four-point susceptibility (n_o S2 - S1^2) / (n_o^2 N_g), (n_lags, G) float64: the variance of Q over the
        origins used, per atom.  The origins overlap in time, so this is the population variance over the trajectory
        (divisor n_o), not an estimate from independent samples.  The numerator is formed in Python integers (exact);
        NaN for an empty group, 0 with one origin."""
        out = np.full(np.shape(self.sum), np.nan)
        for j in range(out.shape[0]):
            n_o = int(self.origins[j])
            for g in range(out.shape[1]):
                n_g = int(self.counts[g])
                if n_g > 0 and n_o > 0:
                    s1, s2 = int(self.sum[j, g]), int(self.sum_squares[j, g])
                    out[j, g] = (n_o * s2 - s1 * s1) / (n_o * n_o * n_g)
        return out

    def relaxation_time(self, level: float = 1.0 / np.e) -> np.ndarray:
        """The time at which q(t) / q(t_0) first falls to `level`, per group, (G,), by `psa_amd.relaxation_time` on the
        lags in the order given (they should ascend from a lag where q is positive)"""
        return relaxation_time(np.nan_to_num(self.q, nan=0.0), self.times, level)

    def peak(self) -> Tuple[np.ndarray, np.ndarray]:
        """(t*, chi4*) per group, each (G,): the time of the largest chi4 among the lags of the call and its height;
        NaN for an empty group"""
        chi = self.chi4
        t_star, height = np.full(chi.shape[1], np.nan), np.full(chi.shape[1], np.nan)
        for g in range(chi.shape[1]):
            if chi.shape[0] and not np.all(np.isnan(chi[:, g])):
                j = int(np.nanargmax(chi[:, g]))
                t_star[g], height[g] = float(np.asarray(self.times)[j]), chi[j, g]
        return t_star, height
