"""
Dynamic structure factor and current correlations: spectra whose phase comes from where the atoms ARE in every frame.

Every other spectrum of this package puts the phase on the time-averaged position of an atom, exp(i k.r_mean): the
one-phonon term of a crystal, and noise for a run whose atoms do not stay at a site.  Here

    q_0[k,t]          = sum_a w_a exp(i k.r[t,a])                    the density rho(k,t)
    q_c[k,t]          = sum_a w_a v[t,a,c] exp(i k.r[t,a])           c = 1,2,3: the current j(k,t)
    F_s[k,c,o]        = (1/L) sum_tau win[tau] q_c[k, s H + tau] exp(-2 pi i o tau / L)
    density[o,k]      = 1/(n_seg U) sum_s |F_s[k,0,o]|^2
    longitudinal[o,k] = 1/(n_seg U) sum_s |sum_c khat_c F_s[k,c,o]|^2          khat = k / |k|  (k = 0: khat = 0)
    transverse[o,k]   = ( 1/(n_seg U) sum_s sum_c |F_s[k,c,o]|^2 - longitudinal[o,k] ) / 2
                      = 1/(2 n_seg U) sum_s sum_c |F_s[k,c,o] - khat_c (khat.F_s[k,.,o])|^2

(the GPU forms the transverse part the second way, from the component of F perpendicular to khat: it is a sum of squares
and never negative, however small beside the longitudinal part)

over one atom set (all atoms by default), with per-atom weights w_a (none: 1; scattering lengths, `mass_weights`) and the
segments of `psa_amd.Segments` (L, H, win; U = (1/L) sum win^2, n_seg = 1 + (T - L) // H; none: one boxcar segment of
all T frames; no detrending, two-sided, FFT order, frames after the last segment unused).  r is the positions array as
stored -- no mean is subtracted, `use_displacements` plays no part -- and v the velocities; the phase is exp(+i k.r) of
the float32 inputs taken as exact numbers.  All three are (L, K) float32.

What they show that the mean-position SED cannot: the multi-phonon lines (a wave of amplitude A along e at (k0, w0)
puts |F|^2 = N^2 J_n(k.e A)^2 at (n k0 + G, n w0)), the Debye-Waller decay of the intensity with |k|, the quasi-elastic
line of diffusing atoms -- what an inelastic neutron or X-ray measurement sees.

Conventions.
  * The physical S(k, omega) is `density * L * dt / sum_a w_a^2`: the `structure_factor` property.  It is not baked in.
  * A k = 0 row has no direction: longitudinal is 0 there and transverse (1/2) sum_c |j_c|^2.
  * The static part of rho at a reciprocal-lattice vector -- the Bragg peak, N^2 for unit weights -- sits in bin 0, and
    in its neighbours under a tapered window.  Subtract nothing: it is part of the definition.
  * Pairs (k, -k) are not folded.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np


def time_step(dt_ps, freqs, L):
    """the time step behind a spectrum of L bins: `dt_ps`, or 1 / (L freqs[1]) where that is None (ValueError for L = 1)"""
    if dt_ps is not None:
        return dt_ps
    if L < 2:
        raise ValueError("structure_factor needs dt_ps: the frequencies of a one-bin spectrum hold no time step")
    return 1.0 / (L * abs(float(freqs[1])))


@dataclass
class DynamicSpectra:
    """Result of `SEDCalculator.calculate_dynamic_spectra`: `density`, `longitudinal`, `transverse` (L, K) float32 per
    frequency and k-point (the two current fields None when `currents=False`); `freqs` (L,) = np.fft.fftfreq(L, dt_ps);
    `k_points` (K,), `k_vectors` (K, 3); `atoms`: the atom-index array; `weight_norm` = sum_a w_a^2 over it; `dt_ps`: the
    time step (the calculator sets it; None: `structure_factor` takes it from `freqs`)."""
    density: np.ndarray
    longitudinal: Optional[np.ndarray]
    transverse: Optional[np.ndarray]
    freqs: np.ndarray
    k_points: np.ndarray
    k_vectors: np.ndarray
    atoms: np.ndarray
    weight_norm: float
    dt_ps: Optional[float] = None

    @property
    def structure_factor(self) -> np.ndarray:
        """(L, K) float64: S(k, omega) = density L dt / sum_a w_a^2; dt is `dt_ps`, or 1 / (L freqs[1]) where that is
        None (ValueError for L = 1, whose `freqs` hold no time step)"""
        L = self.density.shape[0]
        return self.density.astype(np.float64) * (L * time_step(self.dt_ps, self.freqs, L) / self.weight_norm)
