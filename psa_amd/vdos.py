"""
Vibrational density of states: the power spectrum of the atoms' own series, summed over the atoms of each group.

    X_s[a,c,o] = (1/L) sum_tau win[tau] d[s H + tau, a, c] exp(-2 pi i o tau / L)
    D[o,g,c]   = 1/(n_seg U) sum_s sum_{a in g} w_a^2 |X_s[a,c,o]|^2          o = 0 .. L // 2

with the segments (L, H, win; U = (1/L) sum win^2, n_seg = 1 + (T - L) // H) of `psa_amd.Segments` -- none: one boxcar
segment of all T frames -- and per-atom weights w_a (none: 1).  One-sided, not doubled: row o is the two-sided value
at bin o of `np.fft.rfftfreq(L, dt_ps)`.  No detrending.  The SED sums amplitudes over atoms before the FFT; this sums
powers after it, so it is the k-integrated companion of a dispersion: band edges, gaps, partial (per-species) DOS.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np


@dataclass
class VDOS:
    """Result of `SEDCalculator.calculate_vdos`: `dos` (F, G, 3) float32 per frequency, atom group and Cartesian
    component, F = L // 2 + 1; `freqs` (F,) = np.fft.rfftfreq(L, dt_ps); `groups`: the G atom-index arrays."""
    dos: np.ndarray
    freqs: np.ndarray
    groups: List[np.ndarray]

    @property
    def total(self) -> np.ndarray:
        """(F, G): summed over the Cartesian components"""
        return np.sum(self.dos, axis=-1)
