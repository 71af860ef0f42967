"""
Segment-averaged (Welch) SED spectra.

The trajectory is cut into windowed segments of L frames, H frames apart; each segment's spectrum is taken and the
power averaged over the segments:

    n_seg      = 1 + (T - L) // H                 (frames after the last segment are not used)
    U          = (1/L) sum_tau w[tau]^2
    F_s[k,c,o] = (1/L) sum_tau w[tau] q[k,c,s H + tau] exp(-2 pi i o tau / L)
    I[o,k]     = 1/(n_seg U) sum_s sum_c |F_s[k,c,o]|^2      (summed over the atom groups of an incoherent sum)

q is the projection of one atom group (the same for every projection route).  No detrending; the frequencies are
np.fft.fftfreq(L, dt_ps), two-sided, in FFT order.  With a boxcar window and L = H = T the result is the ordinary
intensity; with a boxcar window and H = L, sum_o I is the mean power over the frames used (Parseval).  The result is
(L, K) float32 instead of (T, K, 3) complex64: noise falls as 1/sqrt(n_seg) and the download by T / L.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

_WINDOWS = ("hann", "boxcar")


@dataclass(frozen=True)
class Segments:
    """Welch segments for `SEDCalculator.calculate(..., segments=...)`.

    `length` L >= 2 frames; `hop` H >= 1 frames between segment starts (default L // 2; H > L leaves gaps);
    `window`: "hann" (periodic, 0.5 - 0.5 cos(2 pi tau / L), as scipy.signal.get_window("hann", L)), "boxcar", or a
    1-D array of L finite real values that are not all zero (kept as a tuple of floats)."""
    length: int
    hop: Optional[int] = None
    window: Union[str, Tuple[float, ...]] = "hann"

    def __post_init__(self):
        L = self.length
        if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or L < 2:
            raise ValueError(f"segment length must be an integer >= 2, got {L!r}")
        object.__setattr__(self, "length", int(L))
        hop = self.length // 2 if self.hop is None else self.hop
        if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or hop < 1:
            raise ValueError(f"segment hop must be an integer >= 1, got {hop!r}")
        object.__setattr__(self, "hop", int(hop))
        w = self.window
        if isinstance(w, str):
            if w not in _WINDOWS:
                raise ValueError(f"unknown window {w!r}: use one of {_WINDOWS} or an array of length {self.length}")
        else:
            a = np.asarray(w)
            if a.ndim != 1 or a.shape[0] != self.length:
                raise ValueError(f"window must be a 1-D array of length {self.length}, got shape {a.shape}")
            if not np.issubdtype(a.dtype, np.number) or np.issubdtype(a.dtype, np.complexfloating):
                raise ValueError(f"window must be real numbers, got dtype {a.dtype}")
            object.__setattr__(self, "window", tuple(float(v) for v in a.astype(np.float64)))
        wa = self.window_array()
        if not np.all(np.isfinite(wa)):
            raise ValueError("window values must be finite (as float32)")
        if not self.norm() > 0.0:
            raise ValueError("window must not be zero everywhere")

    def window_array(self) -> np.ndarray:
        """The window as (L,) float32 -- what the device multiplies each segment by."""
        L = self.length
        if self.window == "hann":
            # scipy.signal.get_window("hann", L)'s own float64 arithmetic (a periodic general cosine window)
            fac = np.linspace(-np.pi, np.pi, L + 1)[:L]
            return (0.5 + 0.5 * np.cos(fac)).astype(np.float32)
        if self.window == "boxcar":
            return np.ones(L, np.float32)
        with np.errstate(over="ignore"):
            return np.asarray(self.window, np.float64).astype(np.float32)

    def norm(self) -> float:
        """U = (1/L) sum w^2 of the float32 window, in float64."""
        w = self.window_array().astype(np.float64)
        return float(np.dot(w, w) / self.length)

    def count(self, n_frames: int) -> int:
        """n_seg = 1 + (T - L) // H segments in a trajectory of T frames; ValueError if L > T."""
        T = int(n_frames)
        if self.length > T:
            raise ValueError(f"segment length {self.length} exceeds the trajectory's {T} frames")
        return 1 + (T - self.length) // self.hop
