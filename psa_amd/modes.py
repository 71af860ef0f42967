"""
Mode-projected SED (normal-mode decomposition): the spectra of the B basis sites of the primitive cell, contracted with
the polarisation vectors of M modes per k-point before the modulus is taken.

    q_b[k,c,t]  = sum_{a in b} w_a d[t,a,c] exp(+i k.r_a)          the projection of `calculate`, group b = site b
    S_b[k,c,w]  = (1/T) sum_t q_b[k,c,t] exp(-2 pi i w t / T)
    Q[k,nu,w]   = sum_b sum_c conj(eig[k,nu,b,c]) S_b[k,c,w]
    Phi[w,k,nu] = |Q[k,nu,w]|^2                                     (T, K, M) float32, w in FFT order

d is the velocity (the displacement with `use_displacements=True`), r_a the mean position of atom a, w_a its weight
(none: 1; `psa_amd.mass_weights` gives the mass-weighted mode coordinate).  One peak per branch: its position and width
are the frequency and inverse lifetime of mode (k, nu), where the plain SED puts all 3B branches of a k-point into one
column.

Conventions.  `eig` is used as given -- not normalised, not required to be orthogonal, M is free (the three acoustic
branches alone are as valid as all 3B).  The phase is the projection's: exp(+i k.r_a) with each atom's OWN mean
position, not the origin of its cell, and the vectors enter conjugated.  Eigenvectors of a lattice-dynamics code
(phonopy, GULP) that uses exp(-i k.r), cell origins, or another ordering of the sites have to be converted by the
caller.  Pairs (k, -k) are not folded: every k-vector has its own vectors.  With unitary vectors (M = 3B) the columns
sum to the incoherent SED of the B groups; with the Cartesian unit vectors they are its |S_b[k,c,w]|^2.

Welch average (`calculate_mode_sed(..., segments=psa_amd.Segments(L, H, window))`; conventions of psa_amd/segments.py:
n_seg = 1 + (T - L) // H, U = (1/L) sum win^2, no detrending, two-sided, FFT order, frames after the last segment
unused).  The segments are cut from the projected series, between the projection and the contraction:

    F_b,s[k,c,w] = (1/L) sum_tau win[tau] q_b[k,c,s H + tau] exp(-2 pi i w tau / L)
    Q_s[k,nu,w]  = sum_b sum_c conj(eig[k,nu,b,c]) F_b,s[k,c,w]
    Phi[w,k,nu]  = 1/(n_seg U) sum_s |Q_s[k,nu,w]|^2                (L, K, M) float32, freqs = fftfreq(L, dt_ps)

One boxcar segment of T frames is the definition above.  With the Cartesian unit vectors of one site (M = 3) the sum
over nu is the segment-averaged `calculate` of that site.  The noise of a thermal spectrum falls as 1/sqrt(n_seg) --
which is what lets `calculate_mode_peaks(..., segments=...)` converge on it -- at the price of resolution: 1 / (L dt).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np


@dataclass
class ModeSED:
    """Result of `SEDCalculator.calculate_mode_sed`: `sed` (T, K, M) float32 per frequency, k-point and mode vector;
    `freqs` (T,) = np.fft.fftfreq(T, dt_ps) -- (L, K, M) and fftfreq(L, dt_ps) with `segments` of length L; `k_points` (K,), `k_vectors` (K, 3); `groups`: the B atom-index arrays."""
    sed: np.ndarray
    freqs: np.ndarray
    k_points: np.ndarray
    k_vectors: np.ndarray
    groups: List[np.ndarray]

    @property
    def total(self) -> np.ndarray:
        """(T, K): summed over the mode vectors"""
        return np.sum(self.sed, axis=-1)


def site_groups(labels) -> List[np.ndarray]:
    """Atom-index arrays, one per distinct label in ascending order of the labels -- the groups of
    `calculate_mode_sed` from a per-atom site index (`np.arange(N) % 8` for the synthetic silicon of `psa_amd.synth`,
    whose atoms are ordered cell-major, basis-minor)."""
    labels = np.asarray(labels)
    if labels.ndim != 1:
        raise ValueError(f"labels must be one value per atom, got shape {labels.shape}")
    return [np.flatnonzero(labels == v) for v in np.unique(labels)]
