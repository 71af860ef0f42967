"""
Time correlations on the reciprocal lattice of the simulation box: the intermediate scattering function F(k,t), its self
part F_s(k,t) and the current correlations C_L(k,t), C_T(k,t), per vector and powder-averaged.

The spectra of `psa_amd.lattice` and `psa_amd.self_spectra` are functions of frequency.  Relaxation is read off the same
quantities as functions of time: the 1/e time of F or F_s is the alpha-relaxation time, its decay rate D Q^2 the
diffusion coefficient, its plateau the glass; the t -> 0 values and the oscillations of C_L and C_T are the sound modes.
Transforming a spectrum back on the host gives the CIRCULAR correlation of each segment -- lag t contaminated by lag
L - t, wrong exactly at the long times.  What is computed here is the linear, unbiased estimator.  With the segments
L, H, n_seg = 1 + (T - L) // H of `psa_amd.Segments` (boxcar only: a taper biases a correlation function; None is one
segment of all T frames) and 1 <= n_lags <= L, for a series x (a row of q of `psa_amd.lattice` for the coherent fields,
z[a,n,.] of `psa_amd.self_spectra` for the self part):

    P      = the smallest power of two >= L + n_lags - 1                (the padded FFT length; part of the definition)
    A_s[o] = sum_{l<L} x[sH + l] exp(-2 pi i o l / P),   o = 0 .. P - 1
    C[t]   = (1/P) sum_o (sum_s |A_s[o]|^2) cos(2 pi o t / P)
           = Re sum_s sum_{l=0}^{L-1-t} x[sH + l + t] conj x[sH + l]    (exactly, because P >= L + n_lags - 1)
    F[t]   = C[t] / (n_seg (L - t)),                     t = 0 .. n_lags - 1

  density       from q_0; for the self part the sum over the atoms of C_a[t] (the weights enter squared)
  longitudinal  from khat.q
  transverse    (1/2) sum_c over the perpendicular components q_c - khat_c (khat.q)

Only the real part is produced: per vector the part even in t; in the powder form the mean over the full sphere is real
(C_{-n}[t] = conj C_n[t]), so the half-space members alone give it.  F[0] is the mean of |x|^2 over the frames used,
F_s(n, 0) = sum_a w_a^2, and with boxcar segments of the same L and H, F[0] = sum_o of the matching spectrum (Parseval).

This module is host code only: the result classes and `relaxation_time`.  `SEDCalculator.calculate_lattice_correlations`,
`calculate_powder_correlations`, `calculate_self_correlations` and `calculate_powder_self_correlations` run them (kernels:
psa_amd/csrc/correlation.hip and the spectral calls' own).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .segments import Segments


def padded_length(length: int, n_lags: int) -> int:
    """P: the smallest power of two >= L + n_lags - 1"""
    P = 1
    while P < int(length) + int(n_lags) - 1:
        P *= 2
    return P


def check_lags(lags, length: int) -> int:
    """`lags` as n_lags (None: L // 2, at least 1); ValueError unless 1 <= n_lags <= L"""
    if lags is None:
        return max(1, int(length) // 2)
    if isinstance(lags, bool) or not isinstance(lags, (int, np.integer)):
        raise ValueError(f"lags must be an integer, got {lags!r}")
    if not 1 <= int(lags) <= int(length):
        raise ValueError(f"lags = {int(lags)} is outside [1, L = {int(length)}]")
    return int(lags)


def check_boxcar(segments: Optional[Segments]) -> None:
    """ValueError unless `segments` is None or every value of its float32 window is exactly 1"""
    if segments is not None and not np.all(segments.window_array() == np.float32(1.0)):
        raise ValueError("time correlations need boxcar segments (Segments(L, H, 'boxcar')): a tapered window biases a "
                         "correlation function")


class _Correlations:
    def normalized(self, field: str = "density") -> np.ndarray:
        """X / X[0] of `field` ("density", "longitudinal" or "transverse") in float64; a column whose X[0] is 0: NaN"""
        if field not in ("density", "longitudinal", "transverse"):
            raise ValueError(f"unknown field {field!r}")
        x = getattr(self, field)
        if x is None:
            raise ValueError(f"this result holds no {field} field")
        x = np.asarray(x, np.float64)
        out = np.full(x.shape, np.nan)
        np.divide(x, x[:1], out=out, where=x[:1] != 0)
        return out


@dataclass
class TimeCorrelations(_Correlations):
    """Result of `SEDCalculator.calculate_lattice_correlations` and `calculate_self_correlations`: `density` = F(k,t) or
    F_s(k,t), `longitudinal` = C_L(k,t), `transverse` = C_T(k,t), (n_lags, K) float32 each (the two current fields None
    for the self part and with `currents=False`); `times` (n_lags,) = arange(n_lags) dt_ps; `origins` (n_lags,) =
    n_seg (L - t), the time origins behind each lag; `k_points`, `k_vectors`, `atoms`, `weight_norm`, `dt_ps` as for
    `DynamicSpectra`."""
    density: np.ndarray
    longitudinal: Optional[np.ndarray]
    transverse: Optional[np.ndarray]
    times: np.ndarray
    origins: np.ndarray
    k_points: np.ndarray
    k_vectors: np.ndarray
    atoms: np.ndarray
    weight_norm: float
    dt_ps: Optional[float] = None


@dataclass
class PowderTimeCorrelations(_Correlations):
    """Result of `SEDCalculator.calculate_powder_correlations` and `calculate_powder_self_correlations`: the fields of
    `TimeCorrelations` as (n_lags, n_bins) float32 averages over the shells (an empty bin: zeros), `times`, `origins`;
    `q`, `q_edges`, `counts`, `available`, `indices`, `bin_index`, `atoms`, `weight_norm`, `dt_ps` as for
    `PowderSpectra`."""
    density: np.ndarray
    longitudinal: Optional[np.ndarray]
    transverse: Optional[np.ndarray]
    times: np.ndarray
    origins: np.ndarray
    q: np.ndarray
    q_edges: np.ndarray
    counts: np.ndarray
    available: np.ndarray
    indices: np.ndarray
    bin_index: np.ndarray
    atoms: np.ndarray
    weight_norm: float
    dt_ps: Optional[float] = None


def relaxation_time(F, times, level: float = 1.0 / math.e) -> np.ndarray:
    """The time at which F / F[0] first falls to `level`: per column of F (n_lags,) or (n_lags, C) the first t_i with
    F[i] / F[0] <= level, linearly interpolated between t_{i-1} and t_i; NaN where the function never crosses, where
    F[0] is not positive, and 0 where it starts at or below the level.  Returns float64 of shape () or (C,)."""
    f = np.asarray(F, np.float64)
    t = np.asarray(times, np.float64).ravel()
    if f.ndim not in (1, 2) or f.shape[0] != t.size or t.size < 1:
        raise ValueError(f"F {f.shape} and times {t.shape} do not fit (n_lags,) or (n_lags, C) and (n_lags,)")
    cols = f.reshape(t.size, -1)
    out = np.full(cols.shape[1], np.nan)
    for j in range(cols.shape[1]):
        if not cols[0, j] > 0:
            continue
        g = cols[:, j] / cols[0, j]
        below = np.nonzero(g <= level)[0]
        if below.size == 0:
            continue
        i = int(below[0])
        out[j] = t[0] if i == 0 else t[i - 1] + (g[i - 1] - level) / (g[i - 1] - g[i]) * (t[i] - t[i - 1])
    return out.reshape(f.shape[1:])
