"""
Per-atom weights of the SED projection (mass-weighted or charge-weighted spectra).

With weights w the projection of every group becomes q[k,c,t] = sum_a w_a d[t,a,c] exp(i k.r_a).
The phonon SED weights each basis atom by its mass,
    Phi(k, w) ~ sum_b m_b |sum_n int v(n,b,t) exp(i k.r_n - i w t) dt|^2,
which is what an incoherent sum over single-type groups gives with w_a = sqrt(m_b): `mass_weights`.
Signed weights (charges) give the dipole-current spectrum.
"""
from __future__ import annotations

from typing import Mapping

import numpy as np


def mass_weights(types, masses: Mapping[int, float]) -> np.ndarray:
    """sqrt(mass) per atom, float32, for `SEDCalculator.calculate(..., atom_weights=...)`.

    `types`: (N,) atom types (`Trajectory.types`); `masses`: type -> mass.  A type without a mass, or a
    negative or non-finite mass, is a ValueError."""
    t = np.asarray(types).reshape(-1)
    out = np.empty(t.shape, np.float64)
    for kind in np.unique(t):
        key = kind.item()
        if key not in masses:
            raise ValueError(f"no mass given for atom type {key}")
        m = float(masses[key])
        if not (np.isfinite(m) and m >= 0.0):
            raise ValueError(f"mass of atom type {key} must be finite and non-negative, got {m}")
        out[t == kind] = np.sqrt(m)
    return out.astype(np.float32)


def check_atom_weights(atom_weights, n_atoms: int) -> np.ndarray:
    """The weights as a contiguous (n_atoms,) float32 array; ValueError for another shape or a value that is
    not finite (also after the conversion to float32)."""
    w = np.asarray(atom_weights)
    if w.shape != (n_atoms,):
        raise ValueError(f"atom_weights must have shape ({n_atoms},), got {w.shape}")
    if not np.issubdtype(w.dtype, np.number) or np.issubdtype(w.dtype, np.complexfloating):
        raise ValueError(f"atom_weights must be real numbers, got dtype {w.dtype}")
    with np.errstate(over="ignore"):                       # (a value beyond float32 becomes inf: refused below)
        w = np.ascontiguousarray(w, np.float32)
    if not np.all(np.isfinite(w)):
        raise ValueError("atom_weights must be finite (as float32)")
    return w
