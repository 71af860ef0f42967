"""
The real-space half of the self dynamics: mean-square displacement, non-Gaussian parameter and self van Hove function.

The self spectra and F_s(k,t) of `psa_amd.self_spectra` and `psa_amd.correlations` live in reciprocal space, where a
wrapped trajectory needs no unwrapping.  Their small-Q limit, F_s(Q,t) -> exp(-Q^2 msd(t) / 6), is a statement about
the mean-square displacement, which does: with H the box matrix (rows = box vectors, r = s H)

    d[t,a,:] = (r[t,a] - r[t-1,a]) Hinv   (t >= 1)       m[t,a,j] = rint(d_j)
    n[t,a]   = -sum_{t' <= t} m[t',a]     (n[0] = 0)     u[t,a]   = (r[t,a] - r[0,a]) + n[t,a] H

in float64 from the float32 positions.  Contract: no atom moves half a box length or more along a box axis between two
stored frames -- the only convention possible without image flags; an unwrapped trajectory passes through unchanged
(m = 0), and `unwrap=False` skips the search.  With D = u[o+t,a] - u[o,a] over the origins O_t = {0, s, 2 s, ...:
o + t <= T - 1} (s = `origin_step`, n_o(t) = (T - 1 - t) // s + 1) and the atoms of group g:

    components[t,g,c] = <D_c^2>        msd[t,g] = sum_c components[t,g,c]        fourth[t,g] = <|D|^4>
    alpha2[t,g]       = 3 fourth / (5 msd^2) - 1                                  (NaN where msd = 0)
    counts[j,g,i]     = number of (a, o) with i = floor(|D| / dr) at the lag lag_frames[j],   i < n_r, else overflow

  * The estimator is a direct sum over origins, not an FFT: the FFT form is S_1 - 2 S_2, a float32 difference of numbers
    of size |r|^2 for a result of size |D|^2.  The kernel forms D first and squares afterwards.
  * alpha2 is 0 for a Gaussian displacement distribution (Brownian motion, a harmonic solid); jump diffusion and cage
    breaking show as a peak at the time of the jump.
  * `radial_density` = counts / (samples dr) is 4 pi r^2 G_s(r,t), which integrates to 1 - overflow / samples;
    `g_s` = counts / (samples x shell volume) is G_s(r,t) itself.
  * Not here: centre-of-mass drift removal, the velocity autocorrelation in time, per-atom output, sharding.  The
    distinct part G_d and g(r) are in `psa_amd.pairs` (`SEDCalculator.calculate_distinct_van_hove`, `calculate_rdf`);
    the self-overlap per time origin and chi_4(t), its variance over the origins, in `psa_amd.overlap`
    (`SEDCalculator.calculate_overlap`).

This module is host code only: the result types.  `SEDCalculator.calculate_msd` and `SEDCalculator.calculate_van_hove`
run the kernels (psa_amd/csrc/msd.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .pairs import _divide, _shell_volumes


def origin_counts(n_frames: int, n_lags: int, origin_step: int = 1) -> np.ndarray:
    """n_o(t) = (T - 1 - t) // origin_step + 1 for t = 0 .. n_lags - 1, int64"""
    t = np.arange(int(n_lags), dtype=np.int64)
    return (int(n_frames) - 1 - t) // int(origin_step) + 1


def check_origin_step(origin_step) -> int:
    """`origin_step` as an int; ValueError unless it is an integer of at least 1"""
    if isinstance(origin_step, bool) or not isinstance(origin_step, (int, np.integer)) or int(origin_step) < 1:
        raise ValueError(f"origin_step must be an integer of at least 1, got {origin_step!r}")
    return int(origin_step)


def check_count(name: str, value, cap: int) -> int:
    """`value` as an int; ValueError unless it is an integer in [1, cap]"""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= cap:
        raise ValueError(f"{name} must be an integer in [1, {cap}], got {value!r}")
    return int(value)


def check_lag_frames(lag_frames, cap: int, n_frames: int) -> np.ndarray:
    """`lag_frames` (a scalar or a list) as int64 (n_vh,); ValueError unless they are 1 to `cap` integers in [0, T - 1]"""
    tau = np.asarray(lag_frames)
    if tau.ndim == 0:
        tau = tau.reshape(1)
    if tau.ndim != 1 or (tau.size and not (np.issubdtype(tau.dtype, np.integer) or np.all(tau == np.rint(tau)))):
        raise ValueError("lag_frames must be a list of integers")
    tau = tau.astype(np.int64)
    if not 1 <= tau.size <= cap:
        raise ValueError(f"between 1 and {cap} lags are served, got {tau.size}")
    if n_frames and (np.any(tau < 0) or np.any(tau > n_frames - 1)):
        raise ValueError(f"lag_frames must lie in [0, T - 1 = {n_frames - 1}]")
    return tau


def radial_bins(r_max, n_r: int) -> Tuple[float, np.ndarray, np.ndarray]:
    """(dr = r_max / n_r, the n_r + 1 edges, the n_r centres) of a radial histogram; ValueError unless r_max is positive
    and finite"""
    if not (np.isfinite(r_max) and float(r_max) > 0.0):
        raise ValueError(f"r_max must be positive and finite, got {r_max!r}")
    dr = float(r_max) / n_r
    edges = dr * np.arange(n_r + 1, dtype=np.float64)
    return dr, edges, 0.5 * (edges[1:] + edges[:-1])


def alpha2(msd: np.ndarray, fourth: np.ndarray) -> np.ndarray:
    """3 fourth / (5 msd^2) - 1 in float64, NaN where msd = 0"""
    m = np.asarray(msd, np.float64)
    out = np.full(m.shape, np.nan)
    np.divide(3.0 * np.asarray(fourth, np.float64), 5.0 * m * m, out=out, where=m != 0)
    return np.where(m != 0, out - 1.0, np.nan)


@dataclass
class MeanSquareDisplacement:
    """Result of `SEDCalculator.calculate_msd`: `msd` (n_lags, G), `components` (n_lags, G, 3), `fourth` (n_lags, G) and
    `alpha2` (n_lags, G), float64; `times` (n_lags,) = arange(n_lags) dt_ps; `origins` (n_lags,) = n_o(t); `groups` the
    atom-index arrays used, `counts` (G,) their sizes."""
    msd: np.ndarray
    components: np.ndarray
    fourth: np.ndarray
    alpha2: np.ndarray
    times: np.ndarray
    origins: np.ndarray
    groups: List[np.ndarray]
    counts: np.ndarray
    dt_ps: Optional[float] = None

    def diffusion(self, fit: Tuple[float, float], per_axis: bool = False) -> np.ndarray:
        """The diffusion coefficient from the least-squares slope of msd(t) over t0_ps <= t <= t1_ps: slope / 6 per group,
        (G,), in (length unit)^2 / ps; `per_axis=True`: slope / 2 of each component, (G, 3).  ValueError when the
        interval holds fewer than two lags."""
        t0, t1 = float(fit[0]), float(fit[1])
        t = np.asarray(self.times, np.float64)
        keep = (t >= t0) & (t <= t1)
        if int(np.count_nonzero(keep)) < 2:
            raise ValueError(f"the fit interval [{t0}, {t1}] ps holds fewer than two lags")
        y = np.asarray(self.components if per_axis else self.msd, np.float64)[keep]
        tc = t[keep] - np.mean(t[keep])
        slope = np.tensordot(tc, y - np.mean(y, axis=0), axes=(0, 0)) / np.sum(tc * tc)
        return slope / (2.0 if per_axis else 6.0)


@dataclass
class VanHoveSelf:
    """Result of `SEDCalculator.calculate_van_hove`: `counts` (n_vh, G, n_r) uint64 and `overflow` (n_vh, G) uint64 (the
    displacements of r_max and beyond); `r_edges` (n_r + 1,), `r` (n_r,) the bin centres; `samples` (n_vh, G) = N_g n_o;
    `lag_frames` (n_vh,), `times` = lag_frames dt_ps; `groups` the atom-index arrays used."""
    counts: np.ndarray
    overflow: np.ndarray
    r_edges: np.ndarray
    r: np.ndarray
    samples: np.ndarray
    lag_frames: np.ndarray
    times: np.ndarray
    groups: List[np.ndarray]
    dt_ps: Optional[float] = None

    def _per_atom(self) -> np.ndarray:
        """N_g n_o, shaped to divide counts"""
        return np.asarray(self.samples, np.float64)[:, :, None]

    @property
    def radial_density(self) -> np.ndarray:
        """counts / (samples dr) = 4 pi r^2 G_s(r,t): sum_i radial_density dr = 1 - overflow / samples"""
        return _divide(self.counts, self._per_atom() * np.diff(self.r_edges)[None, None, :])

    @property
    def g_s(self) -> np.ndarray:
        """counts / (samples (4 pi / 3)(r_hi^3 - r_lo^3)) = G_s(r,t)"""
        return _divide(self.counts, self._per_atom() * _shell_volumes(self.r_edges)[None, None, :])
