"""
Spectral covariance of the site projections, and the mode vectors of the trajectory itself.

    q_i[k,t]    i = 3b + c :  the projection of group b, component c   (as psa_amd/modes.py, weights included)
    S_i[k,w]  = (1/T) sum_t q_i[k,t] exp(-2 pi i w t / T)
    G^(m)[k,i,j] = sum_w g_m[w] S_i[k,w] conj(S_j[k,w])                m = 0 .. n_w - 1,  g_m: (T,) float32, FFT order

a 3B x 3B Hermitian, positive semidefinite (g >= 0) matrix per k-point and weight row, (n_w, K, 3B, 3B) complex128,
reduced over frequency on the GPU without the B group spectra ever leaving HBM (`calculate_spectral_covariance`).

  * With g = 1, Parseval gives G = (1/T) sum_t q q^+, the equal-time covariance of the projected series.
  * For a velocity series, g = 1/(2 pi f)^2 with f != 0 gives the covariance of the displacements derived from the
    velocities.
  * For a displacement series (`use_displacements=True`), g = 1 is the displacement covariance and g = (2 pi f)^2 the
    velocity covariance.
  * `band` = (fmin, fmax) zeroes g outside fmin <= |f| < fmax.
  * The bin f = 0 always has g = 0 in the weights `spectral_weights` makes (a drift has no frequency to divide by); the
    GPU uses the weights it is given as they are.

Mode vectors (`calculate_mode_vectors`, `mode_vectors`).  With mass weights (`psa_amd.mass_weights`) and classical MD the
displacement covariance of the mass-weighted site coordinates at k is k_B T D(k)^-1 (the Green's-function method of
LAMMPS `fix phonon`, Kong 2011): its eigenvectors e_nu are the polarisation vectors of the system at the temperature of
the run, anharmonic shifts included, in exactly the convention `calculate_mode_sed` contracts with -- exp(+i k.r_a) with
each atom's own mean position, the vectors entering conjugated -- because sum_w g Phi[w,k,nu] = e_nu^+ G e_nu is what
that contraction computes.  With G_u the displacement and G_v the velocity covariance,

    G_u e_nu = lambda_nu e_nu              frequency_nu = sqrt(e_nu^+ G_v e_nu / e_nu^+ G_u e_nu) / 2 pi

a Rayleigh quotient in which the temperature cancels.  So the pipeline closes without a lattice-dynamics code:

    mv = calc.calculate_mode_vectors(k_mags, k_vecs, groups, atom_weights=psa_amd.mass_weights(masses))
    fit = calc.calculate_mode_peaks(k_mags, k_vecs, mv.eigenvectors, groups, atom_weights=..., centers=mv.frequency, search=...)

Caveats.  Degenerate branches return some orthonormal basis of their subspace, not a particular one.  The method rests
on equipartition: classical MD and mass weights; without them the eigenvectors of G_u are those of another matrix.  On a
velocity calculator the unweighted g = 1 covariance alone is (by the same equipartition) nearly a multiple of the
identity and carries no mode information: the vectors come from the g = 1/(2 pi f)^2 row.  Welch segments, sharded
calculators and folding of (k, -k) pairs are not supported.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np


def spectral_weights(T: int, dt_ps: float, moment: int, band: Optional[Tuple[float, float]] = None) -> np.ndarray:
    """(T,) float32 weights g = (2 pi f)^moment over f = np.fft.fftfreq(T, dt_ps) in THz, built in float64; `moment` is
    0, -2 or +2.  g is 0 at f = 0 and, with `band` = (fmin, fmax) THz, outside fmin <= |f| < fmax.  ValueError for
    another moment, and for a band that holds no bin or does not lie within (0, Nyquist] (fmin = 0 is accepted: that bin
    is zero anyway)."""
    if moment not in (0, -2, 2):
        raise ValueError(f"moment must be 0, -2 or +2, got {moment!r}")
    if int(T) < 1 or not dt_ps > 0:
        raise ValueError(f"need T >= 1 frames and dt_ps > 0, got T = {T}, dt_ps = {dt_ps}")
    f = np.fft.fftfreq(int(T), d=float(dt_ps))
    keep = f != 0
    if band is not None:
        fmin, fmax = (float(x) for x in band)
        nyquist = 0.5 / float(dt_ps)
        if not (0 <= fmin < fmax <= nyquist * (1 + 1e-12)):
            raise ValueError(f"band = ({fmin}, {fmax}) THz must satisfy 0 <= fmin < fmax <= Nyquist = {nyquist} THz")
        keep &= (np.abs(f) >= fmin) & (np.abs(f) < fmax)
        if not keep.any():
            raise ValueError(f"band = ({fmin}, {fmax}) THz holds no frequency bin (the step is {1.0 / (T * dt_ps)} THz)")
    g = np.zeros(int(T), np.float64)
    g[keep] = (2 * np.pi * f[keep]) ** moment if moment else 1.0
    return g.astype(np.float32)


@dataclass
class ModeVectors:
    """Result of `SEDCalculator.calculate_mode_vectors` / `mode_vectors`: per k-point the 3B modes in ascending
    frequency.  `eigenvectors` (K, 3B, B, 3) complex64, ready to pass as `eigenvectors=` of `calculate_mode_sed` and
    `calculate_mode_peaks`; `frequency` (K, 3B) THz (NaN where `ok` is False); `eigenvalues` (K, 3B) of the displacement
    covariance; `displacement_covariance`, `velocity_covariance` (K, 3B, 3B) complex128; `ok` (K, 3B) bool; `k_points`
    (K,), `k_vectors` (K, 3); `groups`: the B atom-index arrays."""
    eigenvectors: np.ndarray
    frequency: np.ndarray
    eigenvalues: np.ndarray
    displacement_covariance: np.ndarray
    velocity_covariance: np.ndarray
    ok: np.ndarray
    k_points: Optional[np.ndarray] = None
    k_vectors: Optional[np.ndarray] = None
    groups: Optional[List[np.ndarray]] = None


def mode_vectors(G_u: np.ndarray, G_v: np.ndarray) -> ModeVectors:
    """Modes of the displacement covariance `G_u` and the velocity covariance `G_v`, both (K, n, n) Hermitian with
    n = 3B, in float64 on the host: per k-point eigh(G_u), frequency_nu = sqrt(e^+ G_v e / e^+ G_u e) / 2 pi, the modes
    sorted by ascending frequency (those without one last), each vector's largest-modulus component made real and
    positive.  A non-positive eigenvalue or quotient gives a NaN frequency and ok = False for that mode."""
    G_u, G_v = np.asarray(G_u, np.complex128), np.asarray(G_v, np.complex128)
    if G_u.ndim != 3 or G_u.shape[1] != G_u.shape[2] or G_u.shape != G_v.shape or G_u.shape[1] % 3:
        raise ValueError(f"covariances have shapes {G_u.shape} and {G_v.shape}, expected two of (K, 3B, 3B)")
    K, n = G_u.shape[:2]
    vectors = np.zeros((K, n, n), np.complex128)           # [k, nu, i]
    freq, lam = np.full((K, n), np.nan), np.zeros((K, n))
    ok = np.zeros((K, n), bool)
    for k in range(K):
        w, V = np.linalg.eigh(0.5 * (G_u[k] + G_u[k].conj().T))
        num = np.real(np.einsum("in,ij,jn->n", V.conj(), G_v[k], V))
        den = np.real(np.einsum("in,ij,jn->n", V.conj(), G_u[k], V))
        good = (w > 0) & (den > 0) & (num > 0)
        f = np.full(n, np.nan)
        f[good] = np.sqrt(num[good] / den[good]) / (2 * np.pi)
        order = np.argsort(np.where(good, f, np.inf), kind="stable")
        V = V[:, order].T                                      # rows: modes
        top = np.argmax(np.abs(V), axis=1)
        pivot = V[np.arange(n), top]
        V = V * (np.abs(pivot) / np.where(pivot == 0, 1, pivot))[:, None]
        vectors[k], freq[k], lam[k], ok[k] = V, f[order], w[order], good[order]
    return ModeVectors(vectors.reshape(K, n, n // 3, 3).astype(np.complex64), freq, lam, G_u, G_v, ok)
