"""
Partial (species-resolved) dynamic spectra on the reciprocal lattice of the simulation box.

A molten salt, an oxide glass or a Li/Na conductor has more than one species, and what is measured or modelled is never
one spectrum but the matrix of partials S_ab(k, w) and of the partial current correlations C_L^ab, C_T^ab, combined
afterwards with neutron or X-ray scattering lengths, with charges (charge-charge and number-number, Bhatia-Thornton) or
with concentrations.  The conventions are those of `psa_amd.lattice` and `psa_amd.dynamic`: nothing about H, Hinv, s,
the segments, the window, U, the FFT order or khat changes.

  * Species a = 0 .. S - 1 are disjoint atom lists A_a, each in the order given; the weights w are the atom weights.
        q^a_0[n,t] = sum_{i in A_a} w_i exp(2 pi i n.s[t,i])
        q^a_c[n,t] = sum_{i in A_a} w_i v[t,i,c] exp(2 pi i n.s[t,i])            c = 1, 2, 3
    F^a is their windowed transform per segment, exactly as for the lattice spectra.
  * One entry per pair a <= b; the pairs run in row-major order over the upper triangle, (0,0), (0,1), .., (0,S-1),
    (1,1), ..: P = S (S + 1) / 2.  With scale = 1 / (L^2 n_seg U)
        density_ab[o,n]      = scale sum_seg Re(F^a_0 conj F^b_0)
        longitudinal_ab[o,n] = scale sum_seg Re((khat.F^a) conj(khat.F^b))
        transverse_ab[o,n]   = scale 1/2 sum_seg sum_c Re(F_perp,c^a conj F_perp,c^b)     F_perp,c = F_c - khat_c (khat.F)
  * The real part is returned: the symmetrised (ab + ba) / 2, the only part that enters sum_ab b_a b_b S_ab.
  * Off-diagonal entries are not doubled, so  sum_a X_aa + 2 sum_{a<b} X_ab  is the field X of the union of the species.
  * The powder average is that of `psa_amd.lattice`: half-space members, X^ab_-n[o] = X^ab_n[(L - o) mod L] (it holds
    for the real part, since q^a(-n) = conj q^a(n) for real weights), an empty bin a row of zeros.  An empty species
    gives zeros in all of its pairs.

This module is host code only: the pair order, the two result types and what they derive.
`SEDCalculator.calculate_partial_spectra` and `SEDCalculator.calculate_powder_partial_spectra` run the spectra.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from .dynamic import time_step

MAX_SPECIES = 8                        # psa_amd._hip.PARTIAL_MAX_SPECIES: 36 pairs


def pair_table(n_species: int) -> np.ndarray:
    """(P, 2) int: the pairs a <= b of S species in row-major order over the upper triangle"""
    S = int(n_species)
    if S < 1:
        raise ValueError(f"need at least one species, got {n_species}")
    return np.array([(a, b) for a in range(S) for b in range(a, S)], int)


def pair_row(a: int, b: int, n_species: int) -> int:
    """the row of the pair (a, b), in either order, among the P = S (S + 1) / 2 pairs of S species"""
    S = int(n_species)
    a, b = (int(a), int(b)) if a <= b else (int(b), int(a))
    if not 0 <= a <= b < S:
        raise IndexError(f"pair ({a}, {b}) of {S} species")
    return a * S - a * (a - 1) // 2 + (b - a)


class _Partials:
    """what the two result types derive from their (P, L, columns) fields"""

    @property
    def n_species(self) -> int:
        return len(self.groups)

    def pair(self, a: int, b: int) -> int:
        """the row of the pair (a, b) of species, in either order"""
        return pair_row(a, b, self.n_species)

    @property
    def structure_factor(self) -> np.ndarray:
        """(P, L, columns) float64, Ashcroft-Langreth: S_ab = density_ab L dt / sqrt(W_a W_b), W = `weight_norms`; dt is
        `dt_ps`, or 1 / (L freqs[1]) where that is None (ValueError for L = 1).  A pair with an empty species: zeros."""
        L = self.density.shape[1]
        dt = time_step(self.dt_ps, self.freqs, L)
        W = np.asarray(self.weight_norms, np.float64)
        norm = np.sqrt(W[self.pairs[:, 0]] * W[self.pairs[:, 1]])
        factor = np.divide(L * dt, norm, out=np.zeros_like(norm), where=norm > 0)
        return self.density.astype(np.float64) * factor[:, None, None]

    def combine(self, coefficients, field: str = "density") -> np.ndarray:
        """(L, columns) float64: sum_ab c_a c_b X_ab over all ordered pairs -- the diagonal once, every off-diagonal
        entry twice -- for X = `field` ("density", "longitudinal" or "transverse").  c = scattering lengths gives the
        neutron or X-ray total, c = charges the charge-charge spectrum, c = ones the number-number spectrum: the field
        of the union of the species."""
        if field not in ("density", "longitudinal", "transverse"):
            raise ValueError(f"field must be 'density', 'longitudinal' or 'transverse', got {field!r}")
        X = getattr(self, field)
        if X is None:
            raise ValueError(f"the result holds no {field} field (currents=False)")
        c = np.asarray(coefficients, np.float64).ravel()
        if c.size != self.n_species:
            raise ValueError(f"{c.size} coefficients for {self.n_species} species")
        a, b = self.pairs[:, 0], self.pairs[:, 1]
        factor = c[a] * c[b] * np.where(a == b, 1.0, 2.0)
        return np.tensordot(factor, X.astype(np.float64), axes=(0, 0))


@dataclass
class PartialSpectra(_Partials):
    """Result of `SEDCalculator.calculate_partial_spectra`: `density`, `longitudinal`, `transverse` (P, L, K) float32 per
    pair of species, frequency and vector (the two current fields None when `currents=False`); `pairs` (P, 2) the species
    of every row, a <= b; `groups`: the S atom-index arrays; `weight_norms` (S,) = sum_{i in a} w_i^2; `freqs` (L,) =
    np.fft.fftfreq(L, dt_ps); `k_points` (K,), `k_vectors` (K, 3) = n.G in float64; `dt_ps` as for `DynamicSpectra`."""
    density: np.ndarray
    longitudinal: Optional[np.ndarray]
    transverse: Optional[np.ndarray]
    pairs: np.ndarray
    groups: List[np.ndarray]
    weight_norms: np.ndarray
    freqs: np.ndarray
    k_points: np.ndarray
    k_vectors: np.ndarray
    dt_ps: Optional[float] = None


@dataclass
class PowderPartialSpectra(_Partials):
    """Result of `SEDCalculator.calculate_powder_partial_spectra`: `density`, `longitudinal`, `transverse`
    (P, L, n_bins) float32, the averages over the shells per pair of species (the two current fields None when
    `currents=False`; an empty bin: zeros); `pairs`, `groups`, `weight_norms` as for `PartialSpectra`; `q`, `q_edges`,
    `counts`, `available`, `indices`, `bin_index`, `freqs`, `dt_ps` as for `PowderSpectra`."""
    density: np.ndarray
    longitudinal: Optional[np.ndarray]
    transverse: Optional[np.ndarray]
    pairs: np.ndarray
    groups: List[np.ndarray]
    weight_norms: np.ndarray
    q: np.ndarray
    q_edges: np.ndarray
    counts: np.ndarray
    available: np.ndarray
    indices: np.ndarray
    bin_index: np.ndarray
    freqs: np.ndarray
    dt_ps: Optional[float] = None
