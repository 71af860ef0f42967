"""
The self (incoherent) dynamic structure factor on the reciprocal lattice of the simulation box, and its powder average.

The spectra of `psa_amd.dynamic` and `psa_amd.lattice` are coherent: the modulus of a sum over atoms,
|sum_a w_a exp(i k.r_a(t))|^2.  A quasi-elastic neutron measurement on hydrogen, lithium, sodium or vanadium is dominated
by the incoherent cross-section, the SELF part: a sum over atoms of moduli, whose half width Gamma(Q) gives the diffusion
coefficient and the jump length.  Hinv, s and the window are those of `psa_amd.lattice`; the segments L, H, win, U, n_seg
those of `psa_amd.dynamic`:

    z[a,n,t]     = w_a exp(2 pi i n.s[t,a])
    Z_s[a,n,o]   = sum_l win[l] z[a,n,sH+l] exp(-2 pi i o l / L)                  (the library's forward FFT)
    density[o,n] = 1/(n_seg U L^2) sum_{a in set} sum_s |Z_s[a,n,o]|^2

  * The weights enter squared, so signed weights are legal and `weight_norm` = sum_a w_a^2 over the atoms used (for a
    neutron measurement w_a = b_inc of the atom's species).  The result is a SUM over atoms, not a mean;
    `structure_factor` = density L dt / weight_norm normalises it.
  * Sum rule: sum_o density[o,n] = sum_a w_a^2 for every vector and every trajectory (Parseval and U = (1/L) sum win^2):
    exact for one boxcar segment, else up to the segments' coverage of the frames.
  * Wrapped trajectories.  exp(2 pi i n.s) with integer n does not notice a whole box vector added to r, so the self
    function of a diffusing atom is correct on wrapped coordinates as stored -- which is why it lives on this lattice:
    with any other k the phase would jump at every crossing of the periodic boundary.
  * Powder form: the mean of `density` over the FULL-sphere vectors of each shell.  The half space is projected and -n
    comes from the frequency mirror, X_{-n}[o] = X_n[(L - o) mod L], since z_{-n}(t) = conj z_n(t) for a real window.
    Bins, counts, the empty bin and the scale 1/(2 n_half n_seg U L^2) are those of `calculate_powder_spectra`.
  * Cost: N_g K n_seg L units of 8 bytes through the FFT -- N_g times the coherent density after its projection.  The
    self part is a mean over atoms and converges as 1/sqrt(N): `max_atoms` draws that many atoms of the set.

This module is host code only: the draw of the atoms.  `SEDCalculator.calculate_self_spectra` and
`SEDCalculator.calculate_powder_self_spectra` run the spectra (kernels: psa_amd/csrc/self.hip) and return the
`DynamicSpectra` and `PowderSpectra` of the coherent methods with the two current fields None.
"""
from __future__ import annotations

from typing import Optional

import numpy as np


def check_max_atoms(max_atoms: Optional[int]) -> Optional[int]:
    """`max_atoms` as an int, or None; ValueError unless it is None or an integer of at least 1"""
    if max_atoms is None:
        return None
    if isinstance(max_atoms, bool) or not isinstance(max_atoms, (int, np.integer)) or int(max_atoms) < 1:
        raise ValueError(f"max_atoms must be an integer of at least 1, got {max_atoms!r}")
    return int(max_atoms)


def draw_atoms(atoms, max_atoms: Optional[int], seed: int = 0) -> np.ndarray:
    """The atoms a self spectrum uses: all of `atoms` (None, or no fewer than the set holds), else `max_atoms` of them
    drawn without replacement by np.random.default_rng(seed), in the order of the set -- the same seed, the same draw.
    ValueError for a `max_atoms` that is not an integer of at least 1."""
    atoms = np.asarray(atoms)
    count = check_max_atoms(max_atoms)
    if count is None or count >= atoms.size:
        return atoms
    keep = np.sort(np.random.default_rng(seed).choice(atoms.size, count, replace=False))
    return atoms[keep]
