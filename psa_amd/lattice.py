"""
Dynamic spectra on the reciprocal lattice of the simulation box, and their powder average.

A liquid, a glass or a superionic conductor has no direction: what is measured is S(Q, w), C_L(Q, w) and C_T(Q, w)
averaged over all k-vectors of a shell |k| ~ Q.  And under periodic boundaries only the commensurate vectors are
legitimate,

    k_n = n_1 G_1 + n_2 G_2 + n_3 G_3,    n integer,    G_i the reciprocal vectors of the WHOLE box

(no atom has a site, so nothing else is defined).  On them the phase is defined by the integers, not by a rounded k:

  * H is the box matrix, its rows the box vectors (`Trajectory.box_matrix`); its float32 entries are taken as exact.
  * Hinv = np.linalg.inv(H) in float64.  The library and the float64 reference use the same 9 numbers.
  * G = 2 pi Hinv^T; its rows are G_1, G_2, G_3.
  * s[t,a,:] = r[t,a,:] . Hinv, on the float32 positions taken as exact: the fractional coordinates.
        q_0[n,t] = sum_a w_a exp(2 pi i n.s[t,a])
        q_c[n,t] = sum_a w_a v[t,a,c] exp(2 pi i n.s[t,a])                 c = 1, 2, 3
  * F_s, `density`, `longitudinal` and `transverse` per vector are exactly those of `psa_amd.dynamic` (segments, U,
    scaling, FFT order), with khat = n.G / |n.G| formed in float64.
  * Powder average.  A bin b holds a set V_b of vectors of the FULL sphere; n = 0 is never in a bin;
        X_b[o] = (1/|V_b|) sum_{n in V_b} X_n[o]                            X = density, longitudinal, transverse.
    One vector of each pair (n, -n) is projected -- the half-space member, whose first non-zero index is positive --
    and X_{-n}[o] = X_n[(L - o) mod L] supplies the other, since q(-n) = conj q(n) for real weights.  A bin with no
    vector is a row of zeros with count 0.

The phase factorises on this lattice, exp(2 pi i n.s) = e^{2 pi i n_1 s_1} e^{2 pi i n_2 s_2} e^{2 pi i n_3 s_3}, which is
what makes a shell of thousands of vectors affordable (psa_amd/csrc/lattice.hip), and the shell sum is formed on the GPU,
so (L, n_bins) crosses to the host and not (L, K).

This module is host code only: the enumeration of the vectors, the bins, and the result type.
`SEDCalculator.calculate_lattice_spectra` and `SEDCalculator.calculate_powder_spectra` run the spectra.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from .dynamic import time_step


def box_inverse(box_matrix) -> np.ndarray:
    """Hinv (3, 3) float64 of the box matrix (rows = box vectors), its float32 entries taken as exact; ValueError for a
    matrix that is not (3, 3), not finite or singular"""
    H = np.asarray(box_matrix, np.float32).astype(np.float64)
    if H.shape != (3, 3) or not np.all(np.isfinite(H)):
        raise ValueError(f"box_matrix must be a finite (3, 3) matrix, got shape {H.shape}")
    if np.linalg.det(H) == 0.0:
        raise ValueError("box_matrix is singular")
    return np.linalg.inv(H)


def lattice_k(indices, inverse) -> np.ndarray:
    """(K, 3) float64 k = n.G = 2 pi n . Hinv^T of integer indices (K, 3)"""
    return 2.0 * np.pi * (np.asarray(indices, np.float64).reshape(-1, 3) @ np.asarray(inverse, np.float64).T)


def is_half_space(indices) -> np.ndarray:
    """(K,) bool: the first non-zero index is positive (n = 0: False)"""
    n = np.asarray(indices).reshape(-1, 3)
    lead = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
    return lead > 0


def index_reach(box_matrix, q_max: float) -> np.ndarray:
    """(3,) int: the largest |n_j| a vector with |k| <= q_max can have; n_j = k.a_j / 2 pi, so |n_j| <= |k| |a_j| / 2 pi"""
    H = np.asarray(box_matrix, np.float32).astype(np.float64)
    return np.floor(q_max * np.linalg.norm(H, axis=1) / (2.0 * np.pi) + 1e-9).astype(int)


def commensurate_vectors(box_matrix, q_max: float, q_min: float = 0.0, *, half_space: bool = True):
    """The vectors k = n.G of the box's reciprocal lattice with q_min <= |k| <= q_max, n = 0 excluded:
    (indices (K, 3) int32, k_vectors (K, 3) float64, q (K,) float64 = |k|), sorted by |k| -- compared after rounding to
    1e-12 of q_max, so that vectors equivalent by symmetry count as equal -- then by index.
    half_space: one vector of each pair (n, -n), the one whose first non-zero index is positive; else the full sphere."""
    inv = box_inverse(box_matrix)
    if not (np.isfinite(q_max) and q_max >= 0.0 and 0.0 <= q_min <= q_max):
        raise ValueError(f"need 0 <= q_min <= q_max, got q_min = {q_min}, q_max = {q_max}")
    reach = index_reach(box_matrix, q_max)
    axes = [np.arange(-r, r + 1) for r in reach]
    n = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    n = n[np.any(n != 0, axis=1)]
    if half_space:
        n = n[is_half_space(n)]
    k = lattice_k(n, inv)
    q = np.linalg.norm(k, axis=1)
    keep = (q >= q_min) & (q <= q_max)
    n, k, q = n[keep], k[keep], q[keep]
    # (vectors equivalent by symmetry have norms that differ in the last bits: the key is |k| rounded to 1e-12 of q_max)
    key = np.rint(q / (max(q_max, np.finfo(float).tiny) * 1e-12))
    order = np.lexsort((n[:, 2], n[:, 1], n[:, 0], key))
    return n[order].astype(np.int32), k[order], q[order]


def shell_bins(q, q_edges, *, max_per_bin: Optional[int] = None, seed: int = 0):
    """Shells of |k|: bin b holds the vectors with q_edges[b] <= q < q_edges[b + 1].  Returns
    (bin_index (K,) int32, -1 outside every bin; selected (K,) bool; available (n_bins,) int64; used (n_bins,) int64):
    every vector inside a bin is selected unless `max_per_bin` caps the vectors drawn per bin, without replacement, by
    np.random.default_rng(seed) -- the same seed, the same draw."""
    q = np.asarray(q, np.float64).ravel()
    edges = np.asarray(q_edges, np.float64).ravel()
    if edges.size < 2 or not np.all(np.isfinite(edges)) or np.any(np.diff(edges) <= 0) or edges[0] < 0:
        raise ValueError("q_edges must be at least two finite, non-negative, strictly ascending numbers")
    if max_per_bin is not None and int(max_per_bin) < 1:
        raise ValueError(f"max_per_bin must be at least 1, got {max_per_bin}")
    n_bins = edges.size - 1
    b = np.searchsorted(edges, q, side="right") - 1
    b = np.where((b >= 0) & (b < n_bins), b, -1).astype(np.int32)
    available = np.bincount(b[b >= 0], minlength=n_bins).astype(np.int64)
    selected = b >= 0
    if max_per_bin is not None:
        rng = np.random.default_rng(seed)
        for i in range(n_bins):
            members = np.flatnonzero(b == i)
            if members.size > int(max_per_bin):
                selected[members] = False
                selected[rng.choice(members, int(max_per_bin), replace=False)] = True
    used = np.bincount(b[selected], minlength=n_bins).astype(np.int64)
    return b, selected, available, used


@dataclass
class PowderSpectra:
    """Result of `SEDCalculator.calculate_powder_spectra`: `density`, `longitudinal`, `transverse` (L, n_bins) float32,
    the averages over the shells (the two current fields None when `currents=False`; an empty bin: zeros); `q` (n_bins,)
    the mean |k| of the vectors used (NaN for an empty bin), `q_edges` (n_bins + 1,); `counts` and `available`
    (n_bins,): full-sphere vectors used and present; `indices` (K, 3) int32 the half-space vectors projected and
    `bin_index` (K,) their bins; `freqs` (L,) = np.fft.fftfreq(L, dt_ps); `atoms`, `weight_norm`, `dt_ps` as for
    `DynamicSpectra`."""
    density: np.ndarray
    longitudinal: Optional[np.ndarray]
    transverse: Optional[np.ndarray]
    q: np.ndarray
    q_edges: np.ndarray
    counts: np.ndarray
    available: np.ndarray
    indices: np.ndarray
    bin_index: np.ndarray
    freqs: np.ndarray
    atoms: np.ndarray
    weight_norm: float
    dt_ps: Optional[float] = None

    @property
    def structure_factor(self) -> np.ndarray:
        """(L, n_bins) float64: S(Q, omega) = density L dt / sum_a w_a^2; dt is `dt_ps`, or 1 / (L freqs[1]) where that
        is None (ValueError for L = 1, whose `freqs` hold no time step)"""
        L = self.density.shape[0]
        return self.density.astype(np.float64) * (L * time_step(self.dt_ps, self.freqs, L) / self.weight_norm)
