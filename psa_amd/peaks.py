"""
Frequencies and lifetimes: Lorentzian fits of spectrum peaks on the GPU (psa_fit_peaks; kernels: csrc/peaks.hip).

A spectrum is phi (F, ...) float32 whose row i is bin i of an F-point transform, f_i = i df with df = 1 / (F dt_ps) THz --
the (T, K, M) mode spectra of `calculate_mode_sed` or its Welch-averaged (L, K, M) spectra (`segments=`; F = L, what
`calculate_mode_peaks(..., segments=...)` fits), the (T, K) or Welch-averaged (L, K) SED of `calculate`.  Only the
positive half is used, bins 1 .. ceil(F/2) - 1 (no DC, no Nyquist).  Every column is fitted on its own:

    band     [lo, hi) bins: `band` = (fmin, fmax) THz for all columns (default: the positive half), with `centers` (one
             frequency per column) and `search` the interval [center - search, center + search] cut to it;
             lo = ceil(fmin / df), hi = floor(fmax / df) + 1.
    window   p = the lowest bin of the band at which phi is largest; the run of bins around p with phi >= phi[p] / 2 has
             l + r + 1 bins, h0 = max(1, (l + r + 1) / 2); the fit uses the bins within n = ceil(window_hwhm h0) of p
             (`half_window` THz instead, if given), 4 <= n <= 2047, cut to the band.
    model    height hwhm^2 / ((f - f0)^2 + hwhm^2) + baseline, unweighted least squares by Levenberg-Marquardt.
    status   0 converged; 1 iteration cap reached (best so far); 2 no fit: a band of fewer than 5 bins, no positive
             value, or a non-finite value in the band (NaN results); 3 converged, but f0 outside the window or hwhm
             wider than it.

For a column of the mode-projected SED, `frequency` is the frequency of mode (k, nu) and `lifetime` = 1 / (4 pi hwhm) its
lifetime: tau = 1 / (2 Gamma) with Gamma = 2 pi hwhm the decay rate of the mode's amplitude.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np


@dataclass
class PeakFit:
    """One Lorentzian per spectrum column; every field has the column shape of the input ((K, M) for mode spectra, (K,)
    for an SED), `window` that shape + (2,): `frequency` and `hwhm` in THz, `height`, `baseline` and `rss` (residual sum
    of squares) in the units of the spectrum and its square, `peak_bin` the bin of the band's maximum, `status` (see the
    module text), `iterations`, `window` = [a, b) bins fitted."""
    frequency: np.ndarray
    hwhm: np.ndarray
    height: np.ndarray
    baseline: np.ndarray
    rss: np.ndarray
    peak_bin: np.ndarray
    status: np.ndarray
    iterations: np.ndarray
    window: np.ndarray

    @property
    def lifetime(self) -> np.ndarray:
        """1 / (4 pi hwhm) in ps"""
        return 1.0 / (4.0 * np.pi * self.hwhm)

    @property
    def fwhm(self) -> np.ndarray:
        return 2.0 * self.hwhm

    @property
    def ok(self) -> np.ndarray:
        return self.status == 0

    @classmethod
    def from_arrays(cls, fit: np.ndarray, info: np.ndarray, shape: Tuple[int, ...]) -> "PeakFit":
        """from the (C, 6) float32 and (C, 4) int32 arrays of psa_fit_peaks"""
        f = [np.ascontiguousarray(fit[:, i]).reshape(shape) for i in range(6)]
        window = np.stack([info[:, 2], info[:, 2] + info[:, 3]], axis=-1).reshape(tuple(shape) + (2,))
        peak_bin = np.where(np.isfinite(f[5]), f[5], 0).astype(np.int32)
        return cls(f[0], f[1], f[2], f[3], f[4], peak_bin, np.ascontiguousarray(info[:, 0]).reshape(shape),
                   np.ascontiguousarray(info[:, 1]).reshape(shape), window)


def positive_half(F: int) -> Tuple[int, int]:
    """[1, ceil(F/2)): the bins a band may cover"""
    return 1, (int(F) + 1) // 2


def peak_bands(F: int, df: float, C: int, band=None, centers=None, search=None) -> np.ndarray:
    """(C, 2) int32 bands [lo, hi) of the C columns of an F-bin spectrum with frequency step df (the band arithmetic of
    the module text; host only).  ValueError: `centers` without `search`, a band outside (0, Nyquist) or empty."""
    F, C, df = int(F), int(C), float(df)
    if F < 12:
        raise ValueError(f"a spectrum of {F} frequency bins is too short to fit (need at least 12)")
    if not (np.isfinite(df) and df > 0):
        raise ValueError(f"df must be a positive frequency step, got {df}")
    p_lo, p_hi = positive_half(F)
    nyquist = 0.5 * F * df
    g_lo, g_hi = p_lo, p_hi
    if band is not None:
        fmin, fmax = (float(v) for v in band)
        if not (0.0 <= fmin < fmax <= nyquist):
            raise ValueError(f"band ({fmin}, {fmax}) THz must satisfy 0 <= fmin < fmax <= Nyquist = {nyquist}")
        g_lo, g_hi = max(p_lo, int(np.ceil(fmin / df))), min(p_hi, int(np.floor(fmax / df)) + 1)
        if g_lo >= g_hi:
            raise ValueError(f"band ({fmin}, {fmax}) THz holds no frequency bin (df = {df})")
    out = np.empty((C, 2), np.int32)
    out[:] = (g_lo, g_hi)
    if (centers is None) != (search is None):
        raise ValueError("centers and search go together: one frequency per column and the half width of its interval")
    if centers is not None:
        c = np.asarray(centers, np.float64)
        if c.size != C:
            raise ValueError(f"centers has {c.size} values for {C} spectrum columns")
        c, s = c.reshape(C), float(search)
        if not (s > 0 and np.all(np.isfinite(c))):
            raise ValueError("search must be positive and centers finite")
        lo = np.maximum(g_lo, np.ceil((c - s) / df)).astype(np.int64)
        hi = np.minimum(g_hi, np.floor((c + s) / df) + 1).astype(np.int64)
        if np.any(lo >= hi):
            j = int(np.flatnonzero(lo >= hi)[0])
            raise ValueError(f"column {j}: [{c[j] - s}, {c[j] + s}] THz holds no frequency bin of the band")
        out[:, 0], out[:, 1] = lo, hi
    return out


def half_window_bins(half_window: Optional[float], df: float) -> int:
    """`half_window` THz as the bins the library takes: clamp(round(half_window / df), 4, 2047); None: 0 = automatic"""
    if half_window is None:
        return 0
    if not (np.isfinite(half_window) and half_window > 0):
        raise ValueError(f"half_window must be a positive frequency, got {half_window}")
    return int(min(max(int(round(float(half_window) / float(df))), 4), 2047))


def check_fit_options(window_hwhm: float, max_iter: int):
    if not (np.isfinite(window_hwhm) and window_hwhm > 0):
        raise ValueError(f"window_hwhm must be positive, got {window_hwhm}")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter}")


def spectrum_columns(spectrum) -> Tuple[np.ndarray, Tuple[int, ...]]:
    """(the spectrum as C-contiguous float32 (F, C), its column shape)"""
    a = np.asarray(spectrum)
    if a.ndim < 1 or a.ndim > 3 or np.iscomplexobj(a):
        raise ValueError(f"spectrum must be a real (F,), (F, K) or (F, K, M) array, got shape {a.shape} of {a.dtype}")
    shape = tuple(a.shape[1:])
    a = np.ascontiguousarray(a, np.float32).reshape(a.shape[0], -1)
    if a.shape[0] < 12 or a.shape[1] < 1:
        raise ValueError(f"spectrum of shape {np.shape(spectrum)}: need at least 12 frequency bins and one column")
    return a, shape


def fit_peaks(spectrum, dt_ps: Optional[float] = None, freqs=None, engine=None, **kw) -> PeakFit:
    """`Engine.fit_peaks` with the frequency step from `dt_ps` (df = 1 / (F dt_ps)) or from `freqs` (the spectrum's
    np.fft.fftfreq axis: df = freqs[1] - freqs[0]); `engine`: a `psa_amd._hip.Engine` to run on (default: a new one on
    the default device, closed afterwards).  Keywords: band, centers, search, window_hwhm, half_window, max_iter."""
    from . import _hip
    F = np.shape(spectrum)[0]
    if (dt_ps is None) == (freqs is None):
        raise ValueError("give either dt_ps or freqs")
    if freqs is not None:
        freqs = np.asarray(freqs, np.float64)
        if freqs.shape != (F,):
            raise ValueError(f"freqs has shape {freqs.shape} for a spectrum of {F} bins")
        df = float(freqs[1] - freqs[0])
    else:
        df = 1.0 / (F * float(dt_ps))
    own = engine is None
    eng = _hip.Engine() if own else engine
    try:
        return eng.fit_peaks(spectrum, df, **kw)
    finally:
        if own:
            eng.close()
