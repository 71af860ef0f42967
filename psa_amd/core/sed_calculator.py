"""
SEDCalculator -- host side of the MI355X SED path.

Drop-in for `psa.core.sed_calculator.SEDCalculator` (reference
src/psa/core/sed_calculator.py): same constructor, same `get_k_path` / `get_k_grid` /
`calculate` / `calculate_chiral_phase` signatures, attributes (`a1..a3`, `b1..b3`,
`recip_vecs_prim`, `dt_ps`, `traj`, `use_displacements`) and ValueErrors.  What differs is
where the arithmetic runs: the reference's `_calculate_sed_for_group` (:58-84, NumPy
einsum + pocketfft) is replaced by libpsa_hip.so (phase table -> split-precision f16-MFMA projection, fp32-equivalent ->
batched rocFFT -> epilogue) through `psa_amd._hip.Engine`.  There is no CPU path here.

Residency: the first `calculate` uploads the velocity array (positions with
`use_displacements=True`) to HBM -- projecting the frames of each chunk as it lands -- and later
calls reuse it.  "The same array" is decided by object identity plus a hash of ~2000 sampled
elements, so in-place edits are normally noticed; after editing a trajectory array in place call
`calculator.invalidate()` to be certain (the reference re-reads the array on every call).

`calculate_kpath_sed` / `calculate_kgrid_sed` / `calculate_chiral_sed` are the composites
the reference's README names (README.md:100-140) and its GUI implements privately
(src/psa/gui/psa_gui.py:923-1017, :2099-2247): k generator -> `calculate` -> optional
chiral phase -> `SED`.
"""
from __future__ import annotations

import contextlib
import logging
import weakref
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .. import _hip
from ..io.writer import out_to_qdump
from ..correlations import PowderTimeCorrelations, TimeCorrelations, check_boxcar, check_lags
from ..covariance import ModeVectors, mode_vectors, spectral_weights
from ..displacements import (MeanSquareDisplacement, VanHoveSelf, alpha2, check_count, check_lag_frames, check_origin_step,
                             origin_counts, radial_bins)
from ..dynamic import DynamicSpectra
from ..overlap import DynamicOverlap
from .. import acna, angles, clusters, cna, local_order, order, persistence
from ..angles import BondAngleDistribution
from ..order import BondOrder
from ..clusters import SolidClusters
from ..persistence import BondPersistence
from ..cna import CommonNeighbours
from ..acna import AdaptiveCommonNeighbours
from ..local_order import LocalOrder
from ..pairs import RadialDistribution, VanHoveDistinct, max_pair_radius
from .. import lattice
from ..lattice import PowderSpectra
from ..modes import ModeSED
from ..partial import MAX_SPECIES, PartialSpectra, PowderPartialSpectra, pair_table
from ..peaks import PeakFit
from ..segments import Segments
from ..self_spectra import check_max_atoms, draw_atoms
from ..utils.helpers import parse_direction
from ..vdos import VDOS
from ..weights import check_atom_weights
from .sed import SED
from .trajectory import Trajectory

logger = logging.getLogger(__name__)

_MODES = ("coherent", "incoherent")
# Cartesian components whose phase difference defines chirality about an axis
# (psa_gui.py:975-980)
_CHIRAL_PAIR = {"x": (1, 2), "y": (0, 2), "z": (0, 1)}


class SEDCalculator:
    def __init__(self, traj: Trajectory, nx: int, ny: int, nz: int,
                 use_displacements: bool = False, dt_ps: Optional[float] = None):
        if not (nx > 0 and ny > 0 and nz > 0):
            raise ValueError("System dimensions (nx, ny, nz) must be positive.")
        self.traj = traj
        self.use_displacements = use_displacements

        # timestep: explicit argument (deprecated in the reference, :26-32) wins
        if dt_ps is not None:
            logger.warning("Explicitly providing dt_ps to SEDCalculator is deprecated. "
                           "The provided dt_ps will override the Trajectory's dt_ps.")
            self.dt_ps = dt_ps
        elif getattr(traj, "dt_ps", None) is not None:
            self.dt_ps = traj.dt_ps
        else:
            raise ValueError("Timestep dt_ps not found in Trajectory object and not provided to SEDCalculator.")
        if self.dt_ps <= 0:
            raise ValueError("Timestep dt_ps must be positive.")

        # primitive cell = rows of the box matrix divided by the replication counts (:40-41)
        self.a1, self.a2, self.a3 = (traj.box_matrix[i, :] / n for i, n in enumerate((nx, ny, nz)))
        if min(np.linalg.norm(v) for v in (self.a1, self.a2, self.a3)) < 1e-9:
            raise ValueError("One or more primitive vectors (a1,a2,a3) near zero. Check nx,ny,nz or box matrix.")
        volume = np.abs(np.dot(self.a1, np.cross(self.a2, self.a3)))
        if np.isclose(volume, 0):
            cell = np.vstack([self.a1, self.a2, self.a3])
            if np.linalg.matrix_rank(cell) < 3 or np.isclose(np.linalg.det(cell), 0):
                raise ValueError(f"Primitive cell vectors coplanar/collinear; volume zero ({volume:.2e}).")
            logger.warning("Primitive cell volume very small (%.2e).", volume)
        scale = 2 * np.pi / volume
        self.b1 = scale * np.cross(self.a2, self.a3)
        self.b2 = scale * np.cross(self.a3, self.a1)
        self.b3 = scale * np.cross(self.a1, self.a2)
        self.recip_vecs_prim = np.vstack([self.b1, self.b2, self.b3]).astype(np.float32)

        self._engine: Optional[_hip.Engine] = None
        self._shard = None                    # psa_amd.dist.KShardGroup when k-sharding
        self._mean_cache = None               # (weakref to positions, mean array)

    # ------------------------------------------------------------------ device plumbing
    @property
    def engine(self) -> "_hip.Engine":
        """The GPU context (created on first use; raises if libpsa_hip / a GPU is missing)."""
        if self._engine is None:
            self._engine = _hip.Engine()
        return self._engine

    def attach(self, engine=None, shard_group=None) -> "SEDCalculator":
        """Use an existing Engine and/or shard the k-points over a `dist.KShardGroup`."""
        if engine is not None:
            self._engine = engine
        if shard_group is not None:
            self._shard = shard_group
            self._engine = shard_group.engine
        return self

    def close(self):
        if self._engine is not None and self._shard is None:
            self._engine.close()
        self._engine = None

    def invalidate(self):
        """Forget everything cached about the trajectory arrays -- the copies resident in HBM and
        the mean positions.  Call it after modifying `traj.positions` / `traj.velocities` in
        place; the next `calculate` uploads afresh."""
        self._mean_cache = None
        if self._engine is not None:
            self._engine.invalidate()

    def _mean_positions(self) -> np.ndarray:
        """np.mean(positions, axis=0, dtype=float32) exactly as the reference (:205), cached per
        positions array because it is a full pass over (T,N,3).  In displacement mode the
        positions have to be in HBM anyway, so the pass runs there (mean_over_frames_kernel adds
        the frames in the same order into a float32 accumulator: bit-identical); otherwise it
        is the reference's own NumPy call on the host."""
        pos = self.traj.positions
        stamp = _hip.Engine._fingerprint(pos) if isinstance(pos, np.ndarray) and pos.size else None
        if self._mean_cache is not None and self._mean_cache[0]() is pos and self._mean_cache[2] == stamp:
            return self._mean_cache[1]
        frame_sharded = self._shard is not None and self._shard.nranks > 1 and self._shard.mode != "k"
        if self.use_displacements and not frame_sharded:
            self.engine.ensure_resident(_hip.SLOT_POSITIONS, pos)
            mean = self.engine.mean_positions(_hip.SLOT_POSITIONS)
        elif (isinstance(pos, np.ndarray) and pos.dtype == np.float32 and pos.flags.c_contiguous and pos.ndim == 3
              and pos.nbytes >= (64 << 20)):
            # velocity mode: the positions stay on the host; a large array is averaged by the library's
            # host threads -- the same sequential float32 chain per column as np.mean, bit for bit
            mean = _hip.host_mean_frames(pos)
        else:               # (a frame-sharded rank holds only its own frames in HBM)
            mean = np.mean(pos, axis=0, dtype=np.float32)
        try:
            self._mean_cache = (weakref.ref(pos), mean, stamp)
        except TypeError:
            self._mean_cache = None
        return mean

    def _data_slot(self):
        if self.use_displacements:
            return _hip.SLOT_POSITIONS, self.traj.positions, _hip.F_DISPLACEMENTS
        return _hip.SLOT_VELOCITIES, self.traj.velocities, 0

    def _device_groups(self, groups: Sequence[np.ndarray]):
        """None (= all atoms in order, the coalesced fast path) when that is what the single
        group is; the index lists otherwise."""
        n = self.traj.n_atoms
        if len(groups) == 1 and groups[0].size == n and np.array_equal(groups[0], np.arange(n)):
            return None
        return [np.asarray(g) for g in groups]

    @contextlib.contextmanager
    def _engine_state(self, weights, segments):
        """The engine locked, with `weights` and `segments` (each only when not None: an engine without them never hears
        of them) set for the block alone: no later calculation (iSED included) sees them."""
        eng = self.engine
        with eng.lock:
            if weights is not None:
                eng.set_atom_weights(weights)
            try:
                if segments is not None:     # (inside the try: cleared whatever happens)
                    eng.set_segments(segments)
                yield
            finally:
                if weights is not None:
                    eng.set_atom_weights(None)
                if segments is not None:
                    eng.set_segments(None)

    def _run_device(self, k_vectors: np.ndarray, groups, intensity: bool, mean_pos_all,
                    fetch: bool = True, atom_weights: Optional[np.ndarray] = None,
                    segments: Optional[Segments] = None):
        """(result, sum_c |result|^2 or None): the second array accompanies a complex result -- it is
        what `SED.intensity` returns (core/sed.py:22-24), produced on the device in the pass that
        writes the result.  `atom_weights` (validated (N,) float32, or None) are set on the engine for
        this calculation only; a sharded run needs nothing more, as every rank makes this same call.
        `segments` (validated against T, intensity only; not on sharded runs) likewise: the result is then
        the (L, K) float32 segment-averaged intensity."""
        slot, data, flags = self._data_slot()
        if intensity:
            flags |= _hip.F_INTENSITY
        want = not intensity
        eng = self.engine
        with self._engine_state(atom_weights, segments):   # project + finalize must not interleave across threads
            K = len(k_vectors)
            T = self.traj.n_frames if segments is None else segments.length
            if self._shard is not None and self._shard.nranks > 1:
                out = self._shard.run(slot, data, mean_pos_all, k_vectors, groups, flags, T, fetch, with_intensity=want)
            elif not eng.is_resident(slot, data):
                # first call on this array: upload and project, overlapped
                eng.project_upload(slot, data, mean_pos_all, k_vectors, groups, flags)
                out = eng.finalize(T, K, intensity, fetch, with_intensity=want)
            elif fetch:                  # one library call; long complex results leave block by block
                out = eng.calculate(slot, mean_pos_all, k_vectors, groups, flags, with_intensity=want)
            else:
                eng.project(slot, mean_pos_all, k_vectors, groups, flags)
                out = eng.finalize(T, K, intensity, False, with_intensity=want)
        if want:
            return out if out is not None else (None, None)
        return out, None

    # ------------------------------------------------------------------ the seam
    def _calculate_sed_for_group(self, k_vectors_3d: np.ndarray, group_atom_indices: np.ndarray,
                                 mean_pos_all: np.ndarray) -> np.ndarray:
        """Complex SED (T,K,3) of one atom group -- the reference's :58-84, on the GPU."""
        n_t = self.traj.n_frames
        idx = np.asarray(group_atom_indices)
        if idx.size == 0 or len(k_vectors_3d) == 0:
            return np.zeros((n_t, len(k_vectors_3d), 3), dtype=np.complex64)
        return self._run_device(np.asarray(k_vectors_3d), self._device_groups([idx]), False,
                                mean_pos_all)[0]

    # ------------------------------------------------------------------ k generators
    def get_k_path(self, direction_spec: Union[str, int, float, List[float], Dict[str, float], np.ndarray],
                   bz_coverage: float, n_k: int, lat_param: Optional[float] = None
                   ) -> Tuple[np.ndarray, np.ndarray]:
        """(|k| (n_k,), k (n_k,3)) float32 along a direction (reference :86-125)."""
        k_hat = parse_direction(direction_spec)
        if lat_param is None or lat_param <= 1e-6:
            # extent of the reciprocal cell along k_hat: largest |k_hat . b_i|  (:94-104)
            proj = [float(abs(np.dot(k_hat, b))) for b in (self.b1, self.b2, self.b3)]
            extent = max(proj)
            if extent > 1e-6:
                logger.info("Using directional reciprocal lattice projection (%.3f 2pi/A) for k-path.", extent)
            else:
                len_a1 = np.linalg.norm(self.a1)
                if not len_a1 > 1e-6:
                    raise ValueError("Invalid/small lattice_param for k-path & reciprocal projections "
                                     "too small for auto-detection.")
                extent = 2 * np.pi / len_a1
                logger.warning("Reciprocal projections too small, using |a1| fallback.")
        else:
            extent = 2 * np.pi / lat_param
        k_max = bz_coverage * extent
        if n_k < 1:
            raise ValueError("n_k (k-points) must be >= 1.")
        if n_k > 1:
            k_mags = np.linspace(0, k_max, n_k, dtype=np.float32)
        else:
            k_mags = np.array([0.0 if np.isclose(k_max, 0) else k_max], dtype=np.float32)
        return k_mags, np.outer(k_mags, k_hat).astype(np.float32)

    def get_k_grid(self, plane: str, k_range_x: Tuple[float, float], k_range_y: Tuple[float, float],
                   n_kx: int, n_ky: int, k_fixed_val: float = 0.0
                   ) -> Tuple[np.ndarray, np.ndarray, Tuple[int, int]]:
        """(empty, k (n_kx*n_ky,3) float32, (n_kx,n_ky)); the first range is the slow index
        (reference :127-180)."""
        if n_kx <= 0 or n_ky <= 0:
            raise ValueError("Number of k-points (n_kx, n_ky) must be positive.")
        # column of the k-vector fed by (first range, second range, fixed value)
        columns = {"xy": (0, 1, 2), "yz": (1, 2, 0), "zx": (2, 0, 1)}.get(plane.lower())
        if columns is None:
            raise ValueError(f"Invalid plane specified: {plane}. Must be 'xy', 'yz', or 'zx'.")
        first = np.linspace(k_range_x[0], k_range_x[1], n_kx, dtype=np.float32)
        second = np.linspace(k_range_y[0], k_range_y[1], n_ky, dtype=np.float32)
        k_vecs = np.empty((n_kx, n_ky, 3), dtype=np.float32)
        k_vecs[:, :, columns[0]] = first[:, None]
        k_vecs[:, :, columns[1]] = second[None, :]
        k_vecs[:, :, columns[2]] = k_fixed_val
        return np.array([], dtype=np.float32), k_vecs.reshape(-1, 3), (n_kx, n_ky)

    # ------------------------------------------------------------------ atom groups
    def _resolve_groups(self, basis_atom_indices, basis_atom_types, summation_mode) -> List[np.ndarray]:
        """Atom-index arrays, one per group, with the reference's precedence and fallbacks
        (:208-266): types win over indices; flat type lists split per type only when
        incoherent; groups without atoms are dropped; nothing left -> all atoms."""
        n_atoms = self.traj.n_atoms
        groups: List[np.ndarray] = []

        def nested(seq, what):
            if all(isinstance(v, list) for v in seq):
                return True
            if all(isinstance(v, int) for v in seq):
                return False
            raise ValueError(f"{what} must be a list of ints or a list of lists of ints.")

        if basis_atom_types is not None:
            if basis_atom_indices is not None:
                logger.warning("Both basis_atom_types and basis_atom_indices provided. Using basis_atom_types.")
            type_sets: List[List[int]] = []
            if isinstance(basis_atom_types, list) and basis_atom_types:
                if nested(basis_atom_types, "basis_atom_types"):
                    type_sets = basis_atom_types
                elif summation_mode == "incoherent":
                    type_sets = [[t] for t in basis_atom_types]
                else:
                    type_sets = [list(basis_atom_types)]
            elif isinstance(basis_atom_types, int):
                type_sets = [[basis_atom_types]]
            for ts in type_sets:
                members = np.flatnonzero(np.isin(self.traj.types, ts))
                if members.size:
                    groups.append(members)
                else:
                    logger.warning("No atoms found for type group %s. Skipping.", ts)
        elif basis_atom_indices is not None:
            lists: List[np.ndarray] = []
            if isinstance(basis_atom_indices, list):
                if basis_atom_indices:
                    if nested(basis_atom_indices, "basis_atom_indices"):
                        lists = [np.asarray(sub, dtype=int) for sub in basis_atom_indices]
                    else:
                        lists = [np.asarray(basis_atom_indices, dtype=int)]
            elif isinstance(basis_atom_indices, np.ndarray):
                if basis_atom_indices.ndim == 1 and basis_atom_indices.size > 0:
                    lists = [basis_atom_indices.astype(int)]
                else:
                    logger.warning("Unsupported np.ndarray format for basis_atom_indices. "
                                   "Using all atoms if no other basis defined.")
            for members in lists:
                if members.size == 0:
                    continue
                if np.any(members >= n_atoms) or np.any(members < 0):
                    raise ValueError("Atom indices in basis out of bounds.")
                groups.append(members)

        if not groups:
            groups.append(np.arange(n_atoms))
            if summation_mode == "incoherent" and n_atoms > 0:
                logger.info("Using all atoms. Incoherent sum will effectively be a coherent sum of all atoms.")
        return groups

    # ------------------------------------------------------------------ calculate
    def calculate(self, k_points_mags: np.ndarray, k_vectors_3d: np.ndarray,
                  basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                  basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None,
                  summation_mode: str = 'coherent',
                  k_grid_shape: Optional[Tuple[int, int]] = None,
                  k_chunk_size: int = 500, *, atom_weights: Optional[np.ndarray] = None,
                  segments: Optional[Segments] = None) -> SED:
        """SED of the trajectory at the given k-vectors (reference :182-336).

        coherent (or a single group): `sed` is (T,K,3) complex64; incoherent with several
        groups: (T,K) float32 = sum_g sum_c |S_g|^2.  `k_chunk_size` is accepted for
        compatibility; the GPU handles all k-points in one pass over the trajectory
        instead of re-gathering it per chunk (:287-290), which the reference itself only
        matches to ~8e-7.

        `atom_weights` (keyword only; not in the reference): (N,) real finite weights, one per atom of
        the trajectory.  Every group's projection becomes sum_a w_a d[t,a,c] exp(i k.r_a), the phase
        still from the unweighted mean positions; the rest is unchanged.  With w_a = sqrt(m_a)
        (`psa_amd.mass_weights`) and one group per basis type, the incoherent sum is the mass-weighted
        SED sum_b m_b |...|^2.  None: the unweighted result, bit for bit.

        `segments` (keyword only; not in the reference): a `psa_amd.Segments` -- the segment-averaged (Welch)
        intensity instead (psa_amd/segments.py): `sed` is (L,K) float32, `freqs` np.fft.fftfreq(L, dt_ps),
        `is_complex` False, in either mode (coherent: the groups' union as one group; incoherent: summed over the
        groups).  A sharded calculator refuses it (NotImplementedError).  None: the full-length result.
        """
        if summation_mode not in _MODES:
            raise ValueError(f"summation_mode must be 'coherent' or 'incoherent', got {summation_mode}")
        weights = None if atom_weights is None else check_atom_weights(atom_weights, self.traj.n_atoms)
        if segments is not None:
            if not isinstance(segments, Segments):
                raise TypeError(f"segments must be a psa_amd.Segments, got {type(segments).__name__}")
            if self._shard is not None and self._shard.nranks > 1:
                raise NotImplementedError("segment-averaged spectra are not available on a sharded calculator")
        n_t, n_atoms = self.traj.n_frames, self.traj.n_atoms
        if n_t == 0 or n_atoms == 0:
            logger.warning("Cannot calculate SED: 0 frames or 0 atoms.")
            return SED(np.array([], dtype=np.complex64).reshape(0, 0, 3), np.array([], dtype=np.float32),
                       k_points_mags, k_vectors_3d, k_grid_shape=k_grid_shape, is_complex=True, phase=None)

        if segments is not None:
            segments.count(n_t)                          # ValueError if L > T
        mean_pos_all = self._mean_positions()
        freqs = np.fft.fftfreq(n_t, d=self.dt_ps)
        groups = self._resolve_groups(basis_atom_indices, basis_atom_types, summation_mode)
        is_complex = summation_mode == "coherent" or len(groups) <= 1
        n_k = len(k_vectors_3d)

        if segments is not None:
            # the (one) coherent group is projected like an incoherent one of a single group: an intensity
            if is_complex and len(groups) > 1:
                groups = [np.unique(np.concatenate(groups)).astype(int)]
            data = np.zeros((segments.length, 0), np.float32) if n_k == 0 else self._run_device(
                np.asarray(k_vectors_3d), self._device_groups(groups), True, mean_pos_all, atom_weights=weights,
                segments=segments)[0]
            return SED(data, np.fft.fftfreq(segments.length, d=self.dt_ps), k_points_mags, k_vectors_3d,
                       k_grid_shape=k_grid_shape, is_complex=False, phase=None)

        if n_k == 0:
            logger.warning("k_vectors_3d is empty. Returning SED object with empty SED data.")
            shape = (n_t, 0, 3) if is_complex else (n_t, 0)
            data, inten = np.zeros(shape, dtype=np.complex64 if is_complex else np.float32), None
        elif is_complex:
            # several coherent groups act as their sorted union (:297-298)
            members = np.unique(np.concatenate(groups)).astype(int) if len(groups) > 1 else groups[0]
            data, inten = self._run_device(np.asarray(k_vectors_3d), self._device_groups([members]), False,
                                           mean_pos_all, atom_weights=weights)
        else:
            data, inten = self._run_device(np.asarray(k_vectors_3d), self._device_groups(groups), True,
                                           mean_pos_all, atom_weights=weights)
        sed = SED(data, freqs, k_points_mags, k_vectors_3d, k_grid_shape=k_grid_shape,
                  is_complex=is_complex, phase=None)
        if inten is not None and isinstance(data, np.ndarray):
            sed._attach_intensity(inten)                 # `sed.intensity` is free: it came with the result
        from . import sed as _sed_module
        if (_sed_module._FAST_INTENSITY and is_complex and n_k and isinstance(data, np.ndarray) and data.ndim == 3
                and self._shard is None and hasattr(self._engine, "intensity_source")):
            # `sed.intensity` right after the calculation is served from the result still on the device
            sed._device_intensity = self._engine.intensity_source(data)
        return sed

    # ------------------------------------------------------------------ density of states
    def calculate_vdos(self, basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                       basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                       atom_weights: Optional[np.ndarray] = None, segments: Optional[Segments] = None) -> VDOS:
        """Vibrational density of states (not in the reference; definition in psa_amd/vdos.py): the power spectrum of
        each atom's own velocity series (displacement series with `use_displacements=True`) summed over the atoms of
        each group, computed on the GPU from the array resident in HBM.

        Groups are resolved like those of an incoherent `calculate`: `basis_atom_types=[1, 2]` gives the two partial
        densities of states, nothing gives all atoms as one group.  They must be disjoint (ValueError).
        `atom_weights`: as for `calculate`; they enter squared, so `psa_amd.mass_weights` gives sum_a m_a |v_a(w)|^2.
        `segments`: a `psa_amd.Segments` for the Welch average; None is one boxcar segment of all frames.  A sharded
        calculator refuses (NotImplementedError).  Returns a `psa_amd.VDOS` with `dos` (L // 2 + 1, G, 3) float32.
        """
        weights = None if atom_weights is None else check_atom_weights(atom_weights, self.traj.n_atoms)
        if segments is not None and not isinstance(segments, Segments):
            raise TypeError(f"segments must be a psa_amd.Segments, got {type(segments).__name__}")
        if self._shard is not None and self._shard.nranks > 1:
            raise NotImplementedError("the density of states is not available on a sharded calculator")
        n_t, n_atoms = self.traj.n_frames, self.traj.n_atoms
        if n_t == 0 or n_atoms == 0:
            logger.warning("Cannot calculate VDOS: 0 frames or 0 atoms.")
            return VDOS(np.zeros((0, 0, 3), np.float32), np.zeros(0, np.float64), [])
        if segments is not None:
            segments.count(n_t)                          # ValueError if L > T
        groups = self._resolve_groups(basis_atom_indices, basis_atom_types, "incoherent")
        members = np.concatenate(groups)
        if np.unique(members).size != members.size:
            raise ValueError("atom groups of a density of states must be disjoint (an atom is listed twice)")
        L = n_t if segments is None else segments.length
        slot, data, flags = self._data_slot()
        mean_pos_all = self._mean_positions() if self.use_displacements else None
        eng = self.engine
        with self._engine_state(weights, segments):  # (segments before the upload: its FFT primer then builds length L)
            eng.ensure_resident(slot, data)      # later SED calls find it resident
            dos = eng.vdos(slot, mean_pos_all, self._device_groups(groups), flags)
        return VDOS(dos, np.fft.rfftfreq(L, d=self.dt_ps), [np.asarray(g) for g in groups])

    # ------------------------------------------------------------------ dynamic structure factor, currents
    def calculate_dynamic_spectra(self, k_points_mags: np.ndarray, k_vectors_3d: np.ndarray,
                                  basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                  basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                  atom_weights: Optional[np.ndarray] = None, segments: Optional[Segments] = None,
                                  currents: bool = True) -> DynamicSpectra:
        """Dynamic structure factor and longitudinal / transverse current correlations (not in the reference;
        definition in psa_amd/dynamic.py): the spectra of rho(k,t) = sum_a w_a exp(i k.r_a(t)) and
        j(k,t) = sum_a w_a v_a(t) exp(i k.r_a(t)), the phase from the positions of every frame, computed on the GPU
        from the positions and velocities resident in HBM.

        The atom set is resolved like that of a coherent `calculate` (several groups act as their union).  The
        positions are used as stored whatever `use_displacements` says.  `atom_weights` as for `calculate`
        (scattering lengths; `psa_amd.mass_weights`).  `segments`: a `psa_amd.Segments` for the Welch average; None is
        one boxcar segment of all frames; TypeError for anything else, ValueError if L > T.  `currents=False` computes
        the density alone (a quarter of the work) and needs no velocities.  A sharded calculator refuses
        (NotImplementedError).  Returns a `psa_amd.DynamicSpectra` with (L, K) float32 fields."""
        weights = self._dynamic_arguments(atom_weights, segments, "the dynamic spectra")
        k_vectors = np.asarray(k_vectors_3d, np.float32)
        if k_vectors.ndim != 2 or k_vectors.shape[1] != 3:
            raise ValueError(f"k_vectors_3d must be (K, 3), got {k_vectors.shape}")
        if not np.all(np.isfinite(k_vectors)):
            raise ValueError("k_vectors_3d must be finite")
        n_k = k_vectors.shape[0]
        L, freqs = self._dynamic_lengths(segments)
        if self._dynamic_nothing(n_k, "dynamic spectra"):
            zero = np.zeros((L, n_k), np.float32)
            return DynamicSpectra(zero, zero.copy() if currents else None, zero.copy() if currents else None, freqs,
                                  k_points_mags, k_vectors_3d, np.zeros(0, int), 0.0, self.dt_ps)
        out, atoms, norm = self._dynamic_run(basis_atom_indices, basis_atom_types, weights, segments, currents,
                                             lambda eng, listed: eng.dynamic_spectra(k_vectors, listed, currents))
        lon, tra = (out[1], out[2]) if currents else (None, None)
        return DynamicSpectra(out[0], lon, tra, freqs, k_points_mags, k_vectors_3d, atoms, norm, self.dt_ps)

    # what calculate_dynamic_spectra and `_reciprocal` (the ten methods on the box's lattice) share: the checks of the
    # weights, the segments and the sharding; the lengths; the empty inputs; the atom set, the residency and the call
    def _dynamic_arguments(self, atom_weights, segments, what):
        weights = None if atom_weights is None else check_atom_weights(atom_weights, self.traj.n_atoms)
        if segments is not None and not isinstance(segments, Segments):
            raise TypeError(f"segments must be a psa_amd.Segments, got {type(segments).__name__}")
        if self._shard is not None and self._shard.nranks > 1:
            raise NotImplementedError(f"{what} are not available on a sharded calculator")
        return weights

    def _dynamic_lengths(self, segments):
        n_t = self.traj.n_frames
        if segments is not None and n_t:
            segments.count(n_t)                          # ValueError if L > T
        L = n_t if segments is None else segments.length
        return L, (np.fft.fftfreq(L, d=self.dt_ps) if L else np.zeros(0, np.float64))

    def _dynamic_nothing(self, n_k, what):
        if self.traj.n_frames == 0 or self.traj.n_atoms == 0 or n_k == 0:
            logger.warning(f"Cannot calculate {what}: 0 frames, 0 atoms or 0 k-vectors.")
            return True
        return False

    def _dynamic_run(self, basis_atom_indices, basis_atom_types, weights, segments, currents, call, max_atoms=None, seed=0,
                     species=False):
        """(what `call(engine, atom list or None)` returns, the atom-index array, sum_a w_a^2 over it); `max_atoms`: that
        many atoms of the resolved set, drawn by `seed` (the self spectra).  `species`: the partial spectra -- `call`
        gets the species' atom lists, and they and their norms are returned"""
        if species:
            atoms, norm = self._partial_species(basis_atom_indices, basis_atom_types, weights)
            listed = atoms
        else:
            groups = self._resolve_groups(basis_atom_indices, basis_atom_types, "coherent")
            atoms = np.unique(np.concatenate(groups)).astype(int) if len(groups) > 1 else groups[0]
            atoms = np.asarray(draw_atoms(atoms, max_atoms, seed))
            w2 = np.ones(self.traj.n_atoms, np.float64) if weights is None else weights.astype(np.float64) ** 2
            norm = float(np.sum(w2[atoms]))
            listed = self._device_groups([atoms])    # None: all atoms in order
            listed = None if listed is None else listed[0]
        eng = self.engine
        with self._engine_state(weights, segments):  # (segments before the upload: its FFT primer then builds length L)
            eng.ensure_resident(_hip.SLOT_POSITIONS, self.traj.positions)
            if currents:
                eng.ensure_resident(_hip.SLOT_VELOCITIES, self.traj.velocities)
            return call(eng, listed), atoms, norm

    # ------------------------------------------------------------------ spectra on the box's reciprocal lattice
    def _lattice_indices(self, indices):
        n = np.asarray(indices)
        if n.ndim != 2 or n.shape[1] != 3:
            raise ValueError(f"indices must be (K, 3), got {n.shape}")
        if n.size and not (np.issubdtype(n.dtype, np.integer) or np.all(n == np.rint(n))):
            raise ValueError("indices must be integers")
        n = n.astype(np.int64)
        if n.size and int(np.max(np.abs(n))) > _hip.LAT_MAX_INDEX:
            raise ValueError(f"indices up to |n_j| = {_hip.LAT_MAX_INDEX} are served, got {int(np.max(np.abs(n)))}")
        return n.astype(np.int32)

    # the two sources of vectors: (box inverse, indices (K, 3), bin of each or None, n_bins, the result's fields about them)
    def _lattice_vectors(self, indices):
        n = self._lattice_indices(indices)
        inv = lattice.box_inverse(self.traj.box_matrix)
        k = lattice.lattice_k(n, inv)
        return inv, n, None, 0, dict(k_points=np.linalg.norm(k, axis=1), k_vectors=k)

    def _powder_shells(self, q_edges, max_per_bin, seed):
        """the half space of every shell, its bins and the draw"""
        edges = np.asarray(q_edges, np.float64).ravel()
        lattice.shell_bins(np.zeros(0), edges, max_per_bin=max_per_bin)     # ValueError for bad edges or a bad cap
        n_bins = edges.size - 1
        inv = lattice.box_inverse(self.traj.box_matrix)
        reach = lattice.index_reach(self.traj.box_matrix, edges[-1])
        if np.max(reach) > _hip.LAT_MAX_INDEX:
            raise ValueError(f"indices up to |n_j| = {_hip.LAT_MAX_INDEX} are served: q_edges reach |n_j| = {int(np.max(reach))}")
        n_all, _, q_all = lattice.commensurate_vectors(self.traj.box_matrix, edges[-1], edges[0], half_space=True)
        bins, selected, available, used = lattice.shell_bins(q_all, edges, max_per_bin=max_per_bin, seed=seed)
        n, b, q = n_all[selected], bins[selected], q_all[selected]
        q_mean = np.full(n_bins, np.nan)
        np.divide(np.bincount(b, weights=q, minlength=n_bins), used, out=q_mean, where=used > 0)
        return inv, n, b, n_bins, dict(q=q_mean, q_edges=edges, counts=2 * used, available=2 * available, indices=n, bin_index=b)

    def _reciprocal(self, name, kind, family, source, basis_atom_indices, basis_atom_types, atom_weights, segments, *,
                    currents=False, lags=None, max_atoms=None, seed=0):
        """The one body of the ten methods on the box's reciprocal lattice.  `name`: the method's, as its messages spell
        it; `kind`: "spectra" or "correlations" (`lags`); `family`: "coherent" (1 or 3 fields by `currents`), "self"
        (density alone, `max_atoms` of the atoms drawn by `seed`) or "partial" (species, a pair axis); `source()`: the
        vectors, `_lattice_vectors` or `_powder_shells`.  The refusals come in the order of the statements below -- the
        order users see -- and all of them before the engine is touched."""
        weights = self._dynamic_arguments(atom_weights, segments, f"the {name}")   # weights, type of segments, sharded
        if kind == "spectra":
            vectors = source()                               # shape, integers, reach; edges, max_per_bin; the box
            rows, freqs = self._dynamic_lengths(segments)    # L > T
            axis = dict(freqs=freqs)
        else:
            check_boxcar(segments)                           # a tapered window
            L, _ = self._dynamic_lengths(segments)           # L > T
            rows = check_lags(lags, L) if L else 0          # no frames: nothing to correlate, whatever `lags`
            n_seg = 1 if segments is None else segments.count(self.traj.n_frames)
            axis = dict(times=np.arange(rows) * float(self.dt_ps), origins=n_seg * (L - np.arange(rows, dtype=np.int64)))
            vectors = source()                               # (as above)
        inv, n, bin_of, n_bins, about = vectors
        if family == "self":
            check_max_atoms(max_atoms)
        if self._dynamic_nothing(n.shape[0], name):
            pair_axis, atoms, norm = ((1,), [np.zeros(0, int)], np.zeros(1)) if family == "partial" else ((), np.zeros(0, int), 0.0)
            out = np.zeros((3 if currents else 1,) + pair_axis + (rows, n.shape[0] if bin_of is None else n_bins), np.float32)
        else:
            lag = () if kind == "spectra" else (rows,)

            def call(eng, listed):
                if family == "partial":
                    return eng.partial_spectra(inv, n, listed, bin_of, n_bins, currents)
                if family == "self":
                    entry = eng.self_spectra if kind == "spectra" else eng.self_correlations
                    return entry(inv, n, *lag, bin_of, n_bins, listed)[None]
                entry = eng.lattice_spectra if kind == "spectra" else eng.lattice_correlations
                return entry(inv, n, *lag, bin_of, n_bins, listed, currents)
            out, atoms, norm = self._dynamic_run(basis_atom_indices, basis_atom_types, weights, segments, currents, call,
                                                 max_atoms, seed, species=family == "partial")
        head = (out[0],) + ((out[1], out[2]) if currents else (None, None))
        if family == "partial":
            tail = dict(pairs=pair_table(len(atoms)), groups=atoms, weight_norms=norm, **axis, **about, dt_ps=self.dt_ps)
            return PartialSpectra(*head, **tail) if bin_of is None else PowderPartialSpectra(*head, **tail)
        tail = dict(atoms=atoms, weight_norm=norm, **axis, **about, dt_ps=self.dt_ps)
        if kind == "spectra":
            return DynamicSpectra(*head, **tail) if bin_of is None else PowderSpectra(*head, **tail)
        return TimeCorrelations(*head, **tail) if bin_of is None else PowderTimeCorrelations(*head, **tail)

    def calculate_lattice_spectra(self, indices: np.ndarray,
                                  basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                  basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                  atom_weights: Optional[np.ndarray] = None, segments: Optional[Segments] = None,
                                  currents: bool = True) -> DynamicSpectra:
        """The dynamic spectra of `calculate_dynamic_spectra` on the reciprocal lattice of the simulation box (not in
        the reference; definition in psa_amd/lattice.py): k = n_1 G_1 + n_2 G_2 + n_3 G_3 for the integer `indices`
        (K, 3), |n_j| <= 64, G the reciprocal vectors of `traj.box_matrix`; the phase is exp(2 pi i n.s) of the
        fractional coordinates, exact for a commensurate vector where a float32 k is not.  Vectors are projected as
        given: n = 0 is allowed, pairs (n, -n) are not folded.

        Atom set, `atom_weights`, `segments`, `currents`, residency, the empty inputs and the sharded refusal are those
        of `calculate_dynamic_spectra`.  Returns a `psa_amd.DynamicSpectra` whose `k_vectors` are n.G in float64 and
        `k_points` their lengths."""
        return self._reciprocal("lattice spectra", "spectra", "coherent", lambda: self._lattice_vectors(indices),
                                basis_atom_indices, basis_atom_types, atom_weights, segments, currents=currents)

    def calculate_powder_spectra(self, q_edges: np.ndarray,
                                 basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                 basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                 atom_weights: Optional[np.ndarray] = None, segments: Optional[Segments] = None,
                                 currents: bool = True, max_per_bin: Optional[int] = None, seed: int = 0) -> PowderSpectra:
        """Powder-averaged dynamic spectra (not in the reference; definition in psa_amd/lattice.py): S(Q, w), C_L(Q, w)
        and C_T(Q, w) averaged over all vectors of the box's reciprocal lattice in each shell
        q_edges[b] <= |k| < q_edges[b + 1] -- the spectra of a liquid, a glass or a superionic conductor.  The half
        space of every shell is projected on the GPU, -n supplied by the frequency mirror, and the shells are summed
        there in float64.  `max_per_bin` caps the half-space vectors drawn per shell (a seeded draw without
        replacement: `seed`); None takes them all.  ValueError where a shell reaches past |n_j| = 64.

        Atom set, `atom_weights`, `segments`, `currents`, residency, the empty inputs and the sharded refusal are those
        of `calculate_dynamic_spectra`.  Returns a `psa_amd.PowderSpectra` with (L, n_bins) float32 fields."""
        return self._reciprocal("powder spectra", "spectra", "coherent", lambda: self._powder_shells(q_edges, max_per_bin, seed),
                                basis_atom_indices, basis_atom_types, atom_weights, segments, currents=currents)

    # ------------------------------------------------------------------ the self (incoherent) part on that lattice
    def calculate_self_spectra(self, indices: np.ndarray,
                               basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                               basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                               atom_weights: Optional[np.ndarray] = None, segments: Optional[Segments] = None,
                               max_atoms: Optional[int] = None, seed: int = 0) -> DynamicSpectra:
        """The self (incoherent) dynamic structure factor on the reciprocal lattice of the simulation box (not in the
        reference; definition in psa_amd/self_spectra.py): density[o,n] = 1/(n_seg U L^2) sum_a sum_s
        |FFT(win w_a exp(2 pi i n.s_a))|^2 for the integer `indices` (K, 3), |n_j| <= 64 -- a sum over atoms of moduli,
        what an incoherent scatterer shows (`atom_weights` = b_inc), correct on wrapped coordinates as stored.

        `max_atoms` draws that many atoms of the resolved set without replacement by np.random.default_rng(`seed`)
        (the work is linear in the atoms, the statistical error falls as 1/sqrt of them); `atoms` and `weight_norm` of
        the result then describe the atoms used.  Only the positions are made resident.  Atom set, `atom_weights`,
        `segments`, the empty inputs and the sharded refusal are those of `calculate_lattice_spectra`.  Returns a
        `psa_amd.DynamicSpectra` whose two current fields are None."""
        return self._reciprocal("self spectra", "spectra", "self", lambda: self._lattice_vectors(indices),
                                basis_atom_indices, basis_atom_types, atom_weights, segments, max_atoms=max_atoms, seed=seed)

    def calculate_powder_self_spectra(self, q_edges: np.ndarray,
                                      basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                      basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                      atom_weights: Optional[np.ndarray] = None, segments: Optional[Segments] = None,
                                      max_per_bin: Optional[int] = None, max_atoms: Optional[int] = None,
                                      seed: int = 0) -> PowderSpectra:
        """The powder average of `calculate_self_spectra` (definition in psa_amd/self_spectra.py): S_self(Q, w) averaged
        over all vectors of the box's reciprocal lattice in each shell q_edges[b] <= |k| < q_edges[b + 1].  Shells,
        `max_per_bin`, counts and the empty shell are those of `calculate_powder_spectra`; `max_atoms` and everything
        else those of `calculate_self_spectra` (`seed` serves both draws).  Returns a `psa_amd.PowderSpectra` whose two
        current fields are None."""
        return self._reciprocal("powder self spectra", "spectra", "self", lambda: self._powder_shells(q_edges, max_per_bin, seed),
                                basis_atom_indices, basis_atom_types, atom_weights, segments, max_atoms=max_atoms, seed=seed)

    # ------------------------------------------------------------------ time correlations on that lattice
    def calculate_lattice_correlations(self, indices: np.ndarray,
                                       basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                       basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                       atom_weights: Optional[np.ndarray] = None, lags: Optional[int] = None,
                                       segments: Optional[Segments] = None, currents: bool = True) -> TimeCorrelations:
        """The intermediate scattering function F(k,t) and the current correlations C_L(k,t), C_T(k,t) on the reciprocal
        lattice of the simulation box (not in the reference; definition in psa_amd/correlations.py): the linear,
        unbiased time correlation of the series whose spectra `calculate_lattice_spectra` gives, at the lags
        0 .. `lags` - 1 (default L // 2; ValueError outside [1, L]).  `segments`: a boxcar `psa_amd.Segments` -- every
        segment is correlated on its own and the lags averaged over n_seg (L - t) time origins --, None for one segment
        of all frames; a tapered window is refused (ValueError) before anything is uploaded.

        Vectors, atom set, `atom_weights`, `currents`, residency, the empty inputs and the sharded refusal are those of
        `calculate_lattice_spectra`.  Returns a `psa_amd.TimeCorrelations` with (n_lags, K) float32 fields."""
        return self._reciprocal("lattice correlations", "correlations", "coherent", lambda: self._lattice_vectors(indices),
                                basis_atom_indices, basis_atom_types, atom_weights, segments, currents=currents, lags=lags)

    def calculate_powder_correlations(self, q_edges: np.ndarray,
                                      basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                      basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                      atom_weights: Optional[np.ndarray] = None, lags: Optional[int] = None,
                                      segments: Optional[Segments] = None, currents: bool = True,
                                      max_per_bin: Optional[int] = None, seed: int = 0) -> PowderTimeCorrelations:
        """The powder average of `calculate_lattice_correlations`: F(Q,t), C_L(Q,t), C_T(Q,t) averaged over all vectors of
        the box's reciprocal lattice in each shell q_edges[b] <= |k| < q_edges[b + 1].  The half space is projected; the
        mean over the full sphere is real and the half-space members alone give it.  Shells, `max_per_bin`, `seed`,
        counts and the empty shell are those of `calculate_powder_spectra`; `lags`, `segments` and everything else those
        of `calculate_lattice_correlations`.  Returns a `psa_amd.PowderTimeCorrelations` with (n_lags, n_bins) fields."""
        return self._reciprocal("powder correlations", "correlations", "coherent",
                                lambda: self._powder_shells(q_edges, max_per_bin, seed), basis_atom_indices, basis_atom_types,
                                atom_weights, segments, currents=currents, lags=lags)

    def calculate_self_correlations(self, indices: np.ndarray,
                                    basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                    basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                    atom_weights: Optional[np.ndarray] = None, lags: Optional[int] = None,
                                    segments: Optional[Segments] = None, max_atoms: Optional[int] = None,
                                    seed: int = 0) -> TimeCorrelations:
        """The self intermediate scattering function F_s(k,t) on the reciprocal lattice of the simulation box (definition
        in psa_amd/correlations.py): per atom the linear, unbiased time correlation of w_a exp(2 pi i n.s_a(t)), summed
        over the atoms -- F_s(n, 0) = sum_a w_a^2 --, correct on wrapped coordinates as stored.  `lags` and `segments` as
        for `calculate_lattice_correlations`; vectors, atom set, `atom_weights`, `max_atoms`, `seed` and everything else
        as for `calculate_self_spectra`.  Returns a `psa_amd.TimeCorrelations` whose two current fields are None."""
        return self._reciprocal("self correlations", "correlations", "self", lambda: self._lattice_vectors(indices),
                                basis_atom_indices, basis_atom_types, atom_weights, segments, lags=lags, max_atoms=max_atoms,
                                seed=seed)

    def calculate_powder_self_correlations(self, q_edges: np.ndarray,
                                           basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                           basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                           atom_weights: Optional[np.ndarray] = None, lags: Optional[int] = None,
                                           segments: Optional[Segments] = None, max_per_bin: Optional[int] = None,
                                           max_atoms: Optional[int] = None, seed: int = 0) -> PowderTimeCorrelations:
        """The powder average of `calculate_self_correlations`: F_s(Q,t) averaged over all vectors of the box's reciprocal
        lattice in each shell.  Shells, `max_per_bin`, counts and the empty shell are those of
        `calculate_powder_spectra`; everything else as for `calculate_self_correlations` (`seed` serves both draws).
        Returns a `psa_amd.PowderTimeCorrelations` whose two current fields are None."""
        return self._reciprocal("powder self correlations", "correlations", "self",
                                lambda: self._powder_shells(q_edges, max_per_bin, seed), basis_atom_indices, basis_atom_types,
                                atom_weights, segments, lags=lags, max_atoms=max_atoms, seed=seed)

    # ------------------------------------------------------------------ displacements in real space
    def _displacement_groups(self, basis_atom_indices, basis_atom_types, origin_step, unwrap, max_atoms, seed, what):
        """(origin_step, the groups' atom-index arrays after the draw) of a displacement call, after its refusals"""
        step = check_origin_step(origin_step)
        if not isinstance(unwrap, (bool, np.bool_)):
            raise TypeError(f"unwrap must be a bool, got {type(unwrap).__name__}")
        check_max_atoms(max_atoms)
        if self._shard is not None and self._shard.nranks > 1:
            raise NotImplementedError(f"{what} is not available on a sharded calculator")
        if self.traj.n_frames == 0 or self.traj.n_atoms == 0:
            return step, None
        groups = self._resolve_groups(basis_atom_indices, basis_atom_types, "incoherent")
        if len(groups) > _hip.MSD_MAX_GROUPS:
            raise ValueError(f"at most {_hip.MSD_MAX_GROUPS} atom groups are served, got {len(groups)}")
        members = np.concatenate(groups)
        if np.unique(members).size != members.size:
            raise ValueError(f"atom groups of {what} must be disjoint (an atom is listed twice)")
        return step, [np.asarray(draw_atoms(g, max_atoms, seed)) for g in groups]

    def _displacement_run(self, call):
        lattice.box_inverse(self.traj.box_matrix)                # ValueError for a box that is not finite or singular
        eng = self.engine
        eng.ensure_resident(_hip.SLOT_POSITIONS, self.traj.positions)
        return call(eng, np.asarray(self.traj.box_matrix, np.float32).astype(np.float64))

    def calculate_msd(self, basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                      basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *, lags: Optional[int] = None,
                      origin_step: int = 1, unwrap: bool = True, max_atoms: Optional[int] = None,
                      seed: int = 0) -> MeanSquareDisplacement:
        """Mean-square displacement and non-Gaussian parameter of atom groups (not in the reference; definition in
        psa_amd/displacements.py): msd[t,g] = <|u[o+t,a] - u[o,a]|^2> over the time origins o = 0, origin_step, ... and
        the atoms of group g, its three components, the fourth moment and alpha2 = 3 <D^4> / (5 <D^2>^2) - 1, computed on
        the GPU from the positions resident in HBM by a direct sum over origins.

        The positions are used as stored: `unwrap=True` (default) recovers the displacements of a wrapped trajectory
        from the box (no atom may move half a box length or more between two stored frames; an unwrapped trajectory
        passes through unchanged), `unwrap=False` skips that search.  Groups are resolved like those of
        `calculate_vdos`: `basis_atom_types=[1, 2]` gives one curve per species, nothing gives all atoms; they must be
        disjoint, at most 8.  `lags`: number of lags t = 0 .. lags - 1 (None: T // 2); `max_atoms` draws that many atoms
        of every group by `seed`, as the self spectra do.  A sharded calculator refuses (NotImplementedError).
        Returns a `psa_amd.MeanSquareDisplacement`; `.diffusion(fit=(t0_ps, t1_ps))` fits D."""
        n_t = self.traj.n_frames
        n_lags = check_lags(lags, n_t) if n_t else 0
        step, groups = self._displacement_groups(basis_atom_indices, basis_atom_types, origin_step, unwrap, max_atoms, seed,
                                                 "the mean-square displacement")
        times = np.arange(n_lags, dtype=np.float64) * (self.dt_ps if self.dt_ps is not None else 1.0)
        if groups is None:
            logger.warning("Cannot calculate the mean-square displacement: 0 frames or 0 atoms.")
            zero = np.zeros((n_lags, 1), np.float64)
            return MeanSquareDisplacement(zero, np.zeros((n_lags, 1, 3)), zero.copy(), np.full((n_lags, 1), np.nan), times,
                                          np.zeros(n_lags, np.int64), [np.zeros(0, int)], np.zeros(1, np.int64), self.dt_ps)
        out = self._displacement_run(lambda eng, box: eng.displacement_moments(box, n_lags, groups, step, bool(unwrap)))
        msd = out[:, :, :3].sum(axis=2)
        return MeanSquareDisplacement(msd, out[:, :, :3].copy(), out[:, :, 3].copy(), alpha2(msd, out[:, :, 3]), times,
                                      origin_counts(n_t, n_lags, step), groups, np.array([g.size for g in groups], np.int64),
                                      self.dt_ps)

    def calculate_van_hove(self, lag_frames, r_max: float, n_r: int = 200,
                           basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                           basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *, origin_step: int = 1,
                           unwrap: bool = True, max_atoms: Optional[int] = None, seed: int = 0) -> VanHoveSelf:
        """The self van Hove function G_s(r,t) of atom groups at the lags `lag_frames` (frames, at most 64, each in
        [0, T - 1]) (not in the reference; definition in psa_amd/displacements.py): the histogram of |u[o+t,a] - u[o,a]|
        over origins and atoms in `n_r` <= 1024 bins of width r_max / n_r, longer displacements counted in `overflow`.
        Integer counts: sum_i counts + overflow = samples exactly.  Unwrapping, groups, `origin_step`, `max_atoms` and
        the sharded refusal are those of `calculate_msd`.  Returns a `psa_amd.VanHoveSelf` with `radial_density`
        (4 pi r^2 G_s) and `g_s`."""
        n_t = self.traj.n_frames
        tau = check_lag_frames(lag_frames, _hip.MSD_MAX_VH_LAGS, n_t)
        n_r = check_count("n_r", n_r, _hip.MSD_MAX_BINS)
        dr, edges, centres = radial_bins(r_max, n_r)
        step, groups = self._displacement_groups(basis_atom_indices, basis_atom_types, origin_step, unwrap, max_atoms, seed,
                                                 "the van Hove function")
        times = tau.astype(np.float64) * (self.dt_ps if self.dt_ps is not None else 1.0)
        if groups is None:
            logger.warning("Cannot calculate the van Hove function: 0 frames or 0 atoms.")
            return VanHoveSelf(np.zeros((tau.size, 1, n_r), np.uint64), np.zeros((tau.size, 1), np.uint64), edges, centres,
                               np.zeros((tau.size, 1), np.int64), tau, times, [np.zeros(0, int)], self.dt_ps)
        out = self._displacement_run(lambda eng, box: eng.van_hove_self(box, tau, dr, n_r, groups, step, bool(unwrap)))
        n_o = (n_t - 1 - tau) // step + 1
        samples = n_o[:, None] * np.array([g.size for g in groups], np.int64)[None, :]
        return VanHoveSelf(out[:, :, :n_r].copy(), out[:, :, n_r].copy(), edges, centres, samples, tau, times, groups, self.dt_ps)

    def calculate_overlap(self, lag_frames, cutoff: float,
                          basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                          basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *, origin_step: int = 1,
                          unwrap: bool = True, max_atoms: Optional[int] = None, seed: int = 0,
                          per_origin: bool = False) -> DynamicOverlap:
        """The self-overlap function and the four-point susceptibility chi_4(t) of atom groups at the lags `lag_frames`
        (frames, at most 256, each in [0, T - 1]) (not in the reference; definition in psa_amd/overlap.py): per lag and
        time origin the number Q of atoms of the group with |u[o+t,a] - u[o,a]| < `cutoff`, and its sum and sum of squares
        over the origins, as exact integers computed on the GPU.  `.q` is the mean overlap, `.chi4` the variance of Q over
        the origins per atom, `.peak()` its largest value and the time t* of it -- the lifetime of the dynamic
        heterogeneity.  `per_origin=True` also returns Q per origin.  Unwrapping, groups, `origin_step`, `max_atoms` and
        the sharded refusal are those of `calculate_van_hove`.  Returns a `psa_amd.DynamicOverlap`."""
        n_t = self.traj.n_frames
        tau = check_lag_frames(lag_frames, _hip.OVERLAP_MAX_LAGS, n_t)
        if isinstance(cutoff, (bool, np.bool_)) or not isinstance(cutoff, (int, float, np.integer, np.floating)) \
                or not (np.isfinite(cutoff) and float(cutoff) > 0.0):
            raise ValueError(f"cutoff must be positive and finite, got {cutoff!r}")
        if not isinstance(per_origin, (bool, np.bool_)):
            raise TypeError(f"per_origin must be a bool, got {type(per_origin).__name__}")
        step, groups = self._displacement_groups(basis_atom_indices, basis_atom_types, origin_step, unwrap, max_atoms, seed,
                                                 "the self-overlap")
        times = tau.astype(np.float64) * (self.dt_ps if self.dt_ps is not None else 1.0)
        if groups is None:
            logger.warning("Cannot calculate the self-overlap: 0 frames or 0 atoms.")
            n_o = np.zeros(tau.size, np.int64) if n_t == 0 else (n_t - 1 - tau) // step + 1
            table = np.zeros((tau.size, 1, int(n_o.max(initial=0))), np.uint32) if per_origin else None
            return DynamicOverlap(np.zeros((tau.size, 1), np.uint64), np.zeros((tau.size, 1), np.uint64), n_o,
                                  np.zeros(1, np.int64), float(cutoff), tau, times, [np.zeros(0, int)], table, self.dt_ps)
        out, table = self._displacement_run(lambda eng, box: eng.self_overlap(box, tau, float(cutoff), groups, step, bool(unwrap),
                                                                              bool(per_origin)))
        return DynamicOverlap(out[:, :, 0].copy(), out[:, :, 1].copy(), (n_t - 1 - tau) // step + 1,
                              np.array([g.size for g in groups], np.int64), float(cutoff), tau, times, groups, table, self.dt_ps)

    # ------------------------------------------------------------------ pair distributions in real space
    def _pair_call(self, tau, r_max, n_r, basis_atom_indices, basis_atom_types, origin_step, max_atoms, seed, what):
        """(tau int64, n_r, dr, edges, centres, origin_step, the species' atom-index arrays or None, the (n_vh, S, S,
        n_r + 1) counts or None) of a pair call after its refusals -- those of `calculate_van_hove` and the served radius"""
        tau = check_lag_frames(tau, _hip.PAIR_MAX_LAGS, self.traj.n_frames)
        n_r = check_count("n_r", n_r, _hip.PAIR_MAX_BINS)
        served = max_pair_radius(self.traj.box_matrix)           # ValueError for a box that is not finite or singular
        if r_max is None:
            r_max = served
        dr, edges, centres = radial_bins(r_max, n_r)
        if float(r_max) > served:
            raise ValueError(f"r_max = {float(r_max)!r} is beyond the served radius {served!r} (psa_amd.max_pair_radius): "
                             "(1/2 - 2^-12) of the box's least perpendicular width")
        step, groups = self._displacement_groups(basis_atom_indices, basis_atom_types, origin_step, True, max_atoms, seed, what)
        if groups is None:
            logger.warning(f"Cannot calculate {what}: 0 frames or 0 atoms.")
            return tau, n_r, edges, centres, step, None, None
        out = self._displacement_run(lambda eng, box: eng.pair_histogram(box, tau, dr, n_r, groups, step))
        return tau, n_r, edges, centres, step, groups, out

    def _pair_samples(self, tau, step, sizes):
        """(n_o (n_vh,), samples (n_vh, S, S) = n_o N_a (N_b - delta_ab))"""
        n_o = (self.traj.n_frames - 1 - tau) // step + 1
        return n_o, n_o[:, None, None] * sizes[None, :, None] * (sizes[None, None, :] - np.eye(sizes.size, dtype=np.int64)[None])

    def calculate_rdf(self, r_max: Optional[float] = None, n_r: int = 200,
                      basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                      basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *, origin_step: int = 1,
                      max_atoms: Optional[int] = None, seed: int = 0) -> RadialDistribution:
        """The radial distribution function g(r) and its species-resolved partials g_ab(r) (not in the reference;
        definition in psa_amd/pairs.py): the histogram of the minimum-image distance over all ordered pairs of atoms of
        species a and b and the frames 0, origin_step, ..., in `n_r` <= 1024 bins of width r_max / n_r, computed on the
        GPU from the positions resident in HBM.  Integer counts: sum_i counts + overflow = samples exactly, and
        counts[a,b] = counts[b,a].

        The positions are used as stored and nothing is unwrapped: within r_max at most one periodic image of an atom
        lies around another, so the minimum image of a wrapped, an unwrapped or a partly wrapped trajectory is the
        same distance.  `r_max=None` means `psa_amd.max_pair_radius(box)`, (1/2 - 2^-12) of the box's least
        perpendicular width; a larger one is a ValueError.  Species are resolved like the groups of `calculate_vdos`
        (disjoint, at most 8); `max_atoms` draws that many atoms of every species by `seed`.  A sharded calculator
        refuses (NotImplementedError).  Returns a `psa_amd.RadialDistribution` with `g`, `coordination` and `pair(a, b)`."""
        tau, n_r, edges, centres, step, groups, out = self._pair_call([0], r_max, n_r, basis_atom_indices, basis_atom_types,
                                                                      origin_step, max_atoms, seed, "the radial distribution function")
        volume = float(abs(np.linalg.det(np.asarray(self.traj.box_matrix, np.float32).astype(np.float64))))
        if groups is None:
            return RadialDistribution(np.zeros((1, 1, n_r), np.uint64), np.zeros((1, 1), np.uint64), np.zeros((1, 1), np.int64), edges,
                                      centres, volume, [np.zeros(0, int)], np.zeros(1, np.int64), 0)
        sizes = np.array([g.size for g in groups], np.int64)
        n_o, samples = self._pair_samples(tau, step, sizes)
        return RadialDistribution(out[0, :, :, :n_r].copy(), out[0, :, :, n_r].copy(), samples[0], edges, centres, volume, groups, sizes,
                                  int(n_o[0]))

    def calculate_distinct_van_hove(self, lag_frames, r_max: Optional[float] = None, n_r: int = 200,
                                    basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                    basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *, origin_step: int = 1,
                                    max_atoms: Optional[int] = None, seed: int = 0) -> VanHoveDistinct:
        """The distinct van Hove function G_d(r,t) of species pairs at the lags `lag_frames` (frames, at most 64, each in
        [0, T - 1]) (not in the reference; definition in psa_amd/pairs.py): the histogram of |mi(r_B(o + t) - r_A(o))|
        over the ordered pairs B != A of species a and b and the origins o = 0, origin_step, ...; lag 0 is g(r).  The
        (a, b) and (b, a) counts differ at t > 0.  Positions as stored, nothing unwrapped; `r_max`, `n_r`, species,
        `max_atoms` and the refusals are those of `calculate_rdf`.  Returns a `psa_amd.VanHoveDistinct` with `g_d`
        (tends to 1 at large r), `radial_density` (4 pi r^2 G_d) and `coordination`; with `VanHoveSelf` of
        `calculate_van_hove` it completes G = G_s + G_d."""
        tau, n_r, edges, centres, step, groups, out = self._pair_call(lag_frames, r_max, n_r, basis_atom_indices, basis_atom_types,
                                                                      origin_step, max_atoms, seed, "the distinct van Hove function")
        volume = float(abs(np.linalg.det(np.asarray(self.traj.box_matrix, np.float32).astype(np.float64))))
        times = tau.astype(np.float64) * (self.dt_ps if self.dt_ps is not None else 1.0)
        if groups is None:
            z = np.zeros((tau.size, 1, 1), np.int64)
            return VanHoveDistinct(np.zeros((tau.size, 1, 1, n_r), np.uint64), z.astype(np.uint64), z, edges, centres, volume,
                                   [np.zeros(0, int)], np.zeros(1, np.int64), np.zeros(tau.size, np.int64), tau, times, self.dt_ps)
        sizes = np.array([g.size for g in groups], np.int64)
        n_o, samples = self._pair_samples(tau, step, sizes)
        return VanHoveDistinct(out[:, :, :, :n_r].copy(), out[:, :, :, n_r].copy(), samples, edges, centres, volume, groups, sizes, n_o,
                               tau, times, self.dt_ps)

    # ------------------------------------------------------------------ bond angles and coordination
    def calculate_bond_angles(self, r_cut, n_theta: int = 180,
                              basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                              basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                              origin_step: int = 1) -> BondAngleDistribution:
        """Bond-angle distributions of species triplets and the coordination statistics of species pairs (not in the
        reference; definition in psa_amd/angles.py), computed on the GPU from the positions resident in HBM.  An atom b
        of species beta is a neighbour of an atom a of species alpha when their minimum-image distance is below
        `r_cut[alpha][beta]` -- `r_cut` a scalar or a symmetric (S, S) matrix, 0 meaning "no bond between these species",
        no entry beyond `psa_amd.max_pair_radius(box)`.  Over the frames 0, origin_step, ... the angle at a between every
        unordered pair of its neighbours is counted in `n_theta` <= 1024 uniform bins over [0, 180] degrees, per centre
        species and species pair of the neighbours, and the number of beta-neighbours of every alpha-atom in
        `coordination_counts`.  Integer counts, positions as stored, nothing unwrapped.

        Species are resolved like those of `calculate_rdf` (disjoint, at most 8).  A centre holds at most 64 neighbours;
        where a centre has more the call raises ValueError naming the species: choose a smaller `r_cut`
        (`Engine.angle_histogram` returns the numbers instead).  A sharded calculator refuses (NotImplementedError).
        Returns a `psa_amd.BondAngleDistribution` with `density`, `triplet(centre, b, c)`, `coordination_fraction` and
        `mean_coordination`."""
        n_theta = check_count("n_theta", n_theta, _hip.ANGLE_MAX_BINS)
        rc, step, groups = self._shell_inputs(r_cut, basis_atom_indices, basis_atom_types, origin_step, "the bond-angle distribution")
        if groups is None:
            return angles.distribution(np.zeros((1, 1, n_theta + 1), np.uint64), np.zeros((1, 1, _hip.ANGLE_MAX_NEIGHBOURS + 1), np.uint64),
                                       np.zeros(1, np.uint64), n_theta, 0, [np.zeros(0, int)])
        out, coord, truncated = self._displacement_run(lambda eng, box: eng.angle_histogram(box, rc, n_theta, groups, step))
        self._refuse_truncated(truncated)
        return angles.distribution(out, coord, truncated, n_theta, (self.traj.n_frames - 1) // step + 1, groups)

    def _shell_inputs(self, r_cut, basis_atom_indices, basis_atom_types, origin_step, what):
        """(r_cut as an array, origin_step, the species' atom-index arrays or None -- warned: 0 frames or 0 atoms) of a call
        on the neighbour shells (`calculate_bond_angles`, `calculate_bond_order`), after its refusals"""
        rc = np.asarray(r_cut, np.float64)
        if rc.ndim not in (0, 2) or not np.all(np.isfinite(rc)) or np.any(rc < 0.0):
            raise ValueError("r_cut must be a scalar or an (S, S) matrix of finite values that are not negative")
        served = max_pair_radius(self.traj.box_matrix)           # ValueError for a box that is not finite or singular
        if rc.size and float(rc.max()) > served:
            raise ValueError(f"r_cut = {float(rc.max())!r} is beyond the served radius {served!r} (psa_amd.max_pair_radius): "
                             "(1/2 - 2^-12) of the box's least perpendicular width")
        step, groups = self._displacement_groups(basis_atom_indices, basis_atom_types, origin_step, True, None, 0, what)
        if groups is None:
            logger.warning(f"Cannot calculate {what}: 0 frames or 0 atoms.")
            return rc, step, None
        S = len(groups)
        if rc.ndim == 2 and (rc.shape != (S, S) or not np.array_equal(rc, rc.T)):
            raise ValueError(f"r_cut must be a scalar or a symmetric ({S}, {S}) matrix, got shape {rc.shape}")
        return rc, step, groups

    @staticmethod
    def _refuse_truncated(truncated):
        if truncated.any():
            bad = ", ".join(f"species {a}: {int(truncated[a])}" for a in np.flatnonzero(truncated))
            raise ValueError(f"centres with more than {_hip.ANGLE_MAX_NEIGHBOURS} neighbours were left out ({bad} (centre, frame) "
                             "samples): r_cut reaches beyond the first shells, choose a smaller r_cut")

    @staticmethod
    def _check_orders(ls, most, lowest, even):
        """`ls` as an array: 1 to `most` strictly ascending integers in [`lowest`, 12], with `even` none of them odd"""
        orders = np.asarray(ls)
        if (orders.ndim != 1 or not 1 <= orders.size <= most or orders.dtype.kind not in "iu"
                or orders.min() < lowest or orders.max() > _hip.ORDER_MAX_L or np.any(np.diff(orders) <= 0)):
            raise ValueError(f"ls must be 1 to {most} strictly ascending {'even ' if even else ''}integers in [{lowest}, {_hip.ORDER_MAX_L}], got {ls!r}")
        if even and np.any(orders % 2):
            raise ValueError(f"ls must be even, got {ls!r}: for odd l the 3j symbol (l l l; m1 m2 m3) is antisymmetric under an "
                             "exchange of two columns, so W_l vanishes identically")
        return orders

    @staticmethod
    def _check_per_atom(per_atom):
        if not isinstance(per_atom, (bool, np.bool_)):
            raise TypeError(f"per_atom must be a bool, got {type(per_atom).__name__}")

    # ------------------------------------------------------------------ Steinhardt bond-orientational order parameters
    def calculate_bond_order(self, r_cut, ls=(4, 6), n_q: int = 200,
                             basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                             basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                             origin_step: int = 1, per_atom: bool = False) -> BondOrder:
        """The Steinhardt bond-orientational order parameters q_l of every atom's neighbour shell (not in the reference;
        definition in psa_amd/order.py), computed on the GPU from the positions resident in HBM.  The neighbours are those
        of `calculate_bond_angles` -- `r_cut` a scalar or a symmetric (S, S) matrix, 0 meaning "no bond between these
        species", no entry beyond `psa_amd.max_pair_radius(box)` -- of all species together.  Over the frames 0,
        origin_step, ... q_l of every centre is counted per species and order in `n_q` <= 1024 uniform bins over [0, 1];
        `ls`: at most 8 strictly ascending orders in [1, 12].  Integer counts, the same bits for any budget and atom
        order; positions as stored, nothing unwrapped.  `per_atom=True` adds `q_atoms` (n_o, n_a, n_l), `neighbours` and
        `mean` -- the (q_4, q_6) scatter that tells fcc, hcp, bcc and icosahedral shells apart.

        Species are resolved like those of `calculate_bond_angles` (disjoint, at most 8).  A centre with no neighbour or
        with a coincident one is counted in `isolated` or `undefined`; where a centre has more than 64 neighbours the
        call raises ValueError naming the species: choose a smaller `r_cut` (`Engine.bond_order` returns the numbers
        instead).  A sharded calculator refuses (NotImplementedError).  Returns a `psa_amd.BondOrder`."""
        n_q = check_count("n_q", n_q, _hip.ORDER_MAX_BINS)
        orders = self._check_orders(ls, _hip.ORDER_MAX_LS, 1, False)
        self._check_per_atom(per_atom)
        rc, step, groups = self._shell_inputs(r_cut, basis_atom_indices, basis_atom_types, origin_step, "the bond order parameters")
        if groups is None:
            zero = np.zeros(1, np.uint64)
            return order.result(np.zeros((1, orders.size, n_q), np.uint64), zero, zero.copy(), zero.copy(), None, None, orders, n_q, 0,
                                [np.zeros(0, int)])
        out = self._displacement_run(lambda eng, box: eng.bond_order(box, rc, orders, n_q, groups, step, bool(per_atom)))
        self._refuse_truncated(out[1])
        return order.result(*out, orders, n_q, (self.traj.n_frames - 1) // step + 1, groups)

    # ------------------------------------------------------------------ neighbour-averaged q_l, w_l and solid-like bonds
    def calculate_local_order(self, r_cut, ls=(4, 6), n_q: int = 200, n_w: int = 200,
                              basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                              basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                              origin_step: int = 1, w_range: float = 0.2, solid_l: int = 6, solid_threshold: float = 0.7,
                              per_atom: bool = False) -> LocalOrder:
        """The neighbour-averaged q-bar_l of Lechner and Dellago, the third-order invariants w_l and w-bar_l, and the
        solid-like bonds of ten Wolde, Ruiz-Montero and Frenkel (not in the reference; definition in
        psa_amd/local_order.py), computed on the GPU from the positions resident in HBM.  The neighbours, `r_cut`, the
        species and `origin_step` are those of `calculate_bond_order`.  `ls`: at most 4 strictly ascending even orders in
        [2, 12] (W_l of an odd l vanishes identically).  q-bar_l is counted in `n_q` <= 1024 uniform bins over [0, 1], w_l
        and w-bar_l in `n_w` <= 1024 bins over [-w_range, w_range]; a bond a-b is solid-like when the normalised product of
        the vectors q_{solid_l, m} of a and b exceeds `solid_threshold` in (0, 1], and `connections` counts the atoms by
        their number of such bonds.  `per_atom=True` adds `qbar_atoms`, `w_atoms`, `wbar_atoms`, `connections_atoms`,
        `neighbours` and `mean`.

        A centre with no neighbour, a coincident one, or a neighbour that is left out itself is counted in `isolated`,
        `undefined` or `incomplete`; where a centre has more than 64 neighbours the call raises ValueError naming the
        species: choose a smaller `r_cut` (`Engine.local_order` returns the numbers instead).  A sharded calculator
        refuses (NotImplementedError).  Returns a `psa_amd.LocalOrder`."""
        n_q = check_count("n_q", n_q, _hip.LOCAL_MAX_BINS)
        n_w = check_count("n_w", n_w, _hip.LOCAL_MAX_BINS)
        orders = self._check_orders(ls, _hip.LOCAL_MAX_LS, 2, True)
        if isinstance(solid_l, (bool, np.bool_)) or not isinstance(solid_l, (int, np.integer)) or int(solid_l) not in orders.tolist():
            raise ValueError(f"solid_l = {solid_l!r} is not among ls = {orders.tolist()}")
        thr, reach = float(solid_threshold), float(w_range)
        if not 0.0 < thr <= 1.0:
            raise ValueError(f"solid_threshold must lie in (0, 1], got {solid_threshold!r}")
        if not (np.isfinite(reach) and reach > 0.0):
            raise ValueError(f"w_range must be finite and positive, got {w_range!r}")
        self._check_per_atom(per_atom)
        rc, step, groups = self._shell_inputs(r_cut, basis_atom_indices, basis_atom_types, origin_step, "the local order parameters")
        if groups is None:
            zero = np.zeros((1, local_order.row_words(orders.size, n_q, n_w)), np.uint64)
            return local_order.result(zero, None, None, None, None, None, orders, n_q, n_w, reach, int(solid_l), thr, 0, [np.zeros(0, int)])
        table = local_order.w3j_blocks(orders)
        out = self._displacement_run(lambda eng, box: eng.local_order(box, rc, orders, n_q, n_w, table, groups, step, reach, int(solid_l),
                                                                      thr, bool(per_atom)))
        res = local_order.result(*out, orders, n_q, n_w, reach, int(solid_l), thr, (self.traj.n_frames - 1) // step + 1, groups)
        self._refuse_truncated(res.truncated)
        return res

    # ------------------------------------------------------------------ solid-like clusters (the largest crystal nucleus)
    def calculate_solid_clusters(self, r_cut, solid_l: int = 6, solid_threshold: float = 0.7, min_connections: int = 7,
                                 link: str = "neighbours", n_sizes: int = 256,
                                 basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                 basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                 origin_step: int = 1, per_atom: bool = False) -> SolidClusters:
        """The clusters of the solid-like atoms at every time origin (not in the reference; definition in
        psa_amd/clusters.py), computed on the GPU from the positions resident in HBM.  The neighbours, `r_cut`, the species
        and `origin_step` are those of `calculate_local_order`, and so is the number of solid-like bonds of an atom for the
        even order `solid_l` in [2, 12] and `solid_threshold` in (0, 1], bit for bit.  An atom with at least
        `min_connections` (0 .. 64) such bonds is solid; two solid atoms are joined when one lists the other
        (`link="neighbours"`) and, with `link="solid_bonds"`, that bond is solid-like too; a cluster is a connected component,
        its label the smallest column of its members.  `largest` (n_o,) is n_max(t); `size_counts` counts the clusters by size
        over all origins in `n_sizes` <= 4096 exact slots and one for the larger ones.  `per_atom=True` adds `labels`,
        `size_atoms`, `connections_atoms`, `neighbours`, `bond_masks` and `atoms`, and with them `largest_atoms(origin)`.

        Where a centre has more than 64 neighbours the call raises ValueError naming the species: choose a smaller `r_cut`
        (`Engine.solid_clusters` returns the numbers instead).  A sharded calculator refuses (NotImplementedError).
        Returns a `psa_amd.SolidClusters`."""
        n_sizes = check_count("n_sizes", n_sizes, _hip.CLUSTER_MAX_SIZES)
        if (isinstance(solid_l, (bool, np.bool_)) or not isinstance(solid_l, (int, np.integer)) or int(solid_l) % 2
                or not 2 <= int(solid_l) <= _hip.ORDER_MAX_L):
            raise ValueError(f"solid_l must be an even integer in [2, {_hip.ORDER_MAX_L}], got {solid_l!r}")
        thr = float(solid_threshold)
        if not 0.0 < thr <= 1.0:
            raise ValueError(f"solid_threshold must lie in (0, 1], got {solid_threshold!r}")
        if (isinstance(min_connections, (bool, np.bool_)) or not isinstance(min_connections, (int, np.integer))
                or not 0 <= int(min_connections) <= _hip.ANGLE_MAX_NEIGHBOURS):
            raise ValueError(f"min_connections must be an integer in [0, {_hip.ANGLE_MAX_NEIGHBOURS}], got {min_connections!r}")
        code = clusters.link_code(link)
        self._check_per_atom(per_atom)
        rc, step, groups = self._shell_inputs(r_cut, basis_atom_indices, basis_atom_types, origin_step, "the solid-like clusters")
        pars = (int(solid_l), thr, int(min_connections), link, n_sizes)
        if groups is None:
            return clusters.result(clusters.empty(1, n_sizes), *pars, 0, [np.zeros(0, int)])
        out = self._displacement_run(lambda eng, box: eng.solid_clusters(box, rc, int(solid_l), thr, int(min_connections), code, n_sizes,
                                                                         groups, step, bool(per_atom)))
        res = clusters.result(out, *pars, (self.traj.n_frames - 1) // step + 1, groups)
        self._refuse_truncated(res.truncated)
        return res

    # ------------------------------------------------------------------ bond persistence (neighbour lifetimes, cages)
    def calculate_bond_persistence(self, r_cut, lag_frames,
                                   basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                   basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *, r_break=None,
                                   origin_step: int = 1, sample_step: int = 1, continuous: bool = True,
                                   per_atom: bool = False) -> BondPersistence:
        """How long a neighbour stays a neighbour (not in the reference; definition in psa_amd/persistence.py), computed on
        the GPU from the positions resident in HBM.  The neighbours, `r_cut`, the species and `origin_step` are those of
        `calculate_bond_angles`, bit for bit.  The bonds listed at a time origin o are tested again at o + lag for every
        lag of `lag_frames` (1 to 1024 strictly ascending frame lags in [0, T - 1], multiples of `sample_step`): a bond is
        alive while its distance stays below `r_break` -- a scalar or a symmetric (S, S) matrix, at least `r_cut` entry by
        entry, 0 exactly where `r_cut` is, nothing beyond `psa_amd.max_pair_radius(box)`; None: `r_cut`, no hysteresis.
        `intermittent` is the share alive at the lag, `continuous` (unless `continuous=False`) the share alive at every
        frame o + sample_step, o + 2 sample_step, ... up to the lag, `cage(c)` the share of the centres that lost fewer than
        c neighbours, `lifetime()` the 1/e time.  Integer counts, the same bits for any budget and atom order; positions as
        stored, nothing unwrapped.  `per_atom=True` adds `alive_masks`, `unbroken_masks` and `atoms`.

        Where a centre has more than 64 neighbours the call raises ValueError naming the species: choose a smaller `r_cut`
        (`Engine.bond_persistence` returns the numbers instead).  A sharded calculator refuses (NotImplementedError).
        Returns a `psa_amd.BondPersistence`."""
        if isinstance(sample_step, (bool, np.bool_)) or not isinstance(sample_step, (int, np.integer)) or int(sample_step) < 1:
            raise ValueError(f"sample_step must be an integer of at least 1, got {sample_step!r}")
        if not isinstance(continuous, (bool, np.bool_)):
            raise TypeError(f"continuous must be a bool, got {type(continuous).__name__}")
        self._check_per_atom(per_atom)
        n_t = self.traj.n_frames
        tau = persistence.check_lags(lag_frames, n_t, int(sample_step))
        rc, step, groups = self._shell_inputs(r_cut, basis_atom_indices, basis_atom_types, origin_step, "the bond persistence")
        rb = persistence.check_break(r_break, rc)
        served = max_pair_radius(self.traj.box_matrix)
        if rb.size and float(rb.max()) > served:
            raise ValueError(f"r_break = {float(rb.max())!r} is beyond the served radius {served!r} (psa_amd.max_pair_radius): "
                             "(1/2 - 2^-12) of the box's least perpendicular width")
        if groups is None:
            return persistence.result(persistence.empty(1, tau.size), tau, np.zeros(tau.size, np.int64), [np.zeros(0, int)], self.dt_ps,
                                      bool(continuous))
        if rb.ndim == 2 and rb.shape != (len(groups), len(groups)):
            raise ValueError(f"r_break must be a scalar or a symmetric ({len(groups)}, {len(groups)}) matrix, got shape {rb.shape}")
        out = self._displacement_run(lambda eng, box: eng.bond_persistence(box, rc, tau, groups, step, r_break=rb,
                                                                           sample_step=int(sample_step), continuous=bool(continuous),
                                                                           per_atom=bool(per_atom)))
        res = persistence.result(out, tau, (n_t - 1 - tau) // step + 1, groups, self.dt_ps, bool(continuous))
        self._refuse_truncated(res.truncated.sum(axis=0))
        return res

    # ------------------------------------------------------------------ common-neighbour analysis (fcc / hcp / bcc / ico)
    def calculate_common_neighbours(self, r_cut,
                                    basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                    basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                    origin_step: int = 1, per_atom: bool = False) -> CommonNeighbours:
        """Common-neighbour analysis (not in the reference; definition in psa_amd/cna.py), computed on the GPU from the
        positions resident in HBM.  The neighbours, `r_cut`, the species and `origin_step` are those of
        `calculate_bond_angles`, bit for bit, and two neighbours of a centre are bonded by the same test.  Every bond gets
        its signature (j, k, l) -- the common neighbours of its two ends, the bonds among them, the bonds of the largest
        connected piece of those -- and every atom its type at every origin: fcc (12 x 421), hcp (6 x 421 + 6 x 422), bcc
        (8 x 666 + 6 x 444 among 14 neighbours), ico (12 x 555) or other.  `signature_counts`, `type_counts` and with them
        `fraction(type)`, `signature(j, k, l)` and `share(j, k, l)` are integer counts, the same bits for any budget and atom
        order; positions as stored, nothing unwrapped.  `per_atom=True` adds `types`, `neighbours`, `bond_signatures`, `atoms`
        and `atoms_of(origin, type)`.

        Where a centre has more than 64 neighbours the call raises ValueError naming the species: choose a smaller `r_cut`
        (`Engine.common_neighbours` returns the numbers instead).  A sharded calculator refuses (NotImplementedError).
        Returns a `psa_amd.CommonNeighbours`."""
        self._check_per_atom(per_atom)
        rc, step, groups = self._shell_inputs(r_cut, basis_atom_indices, basis_atom_types, origin_step, "the common-neighbour analysis")
        if groups is None:
            return cna.result(cna.empty(1), 0, [np.zeros(0, int)])
        out = self._displacement_run(lambda eng, box: eng.common_neighbours(box, rc, groups, step, bool(per_atom)))
        res = cna.result(out, (self.traj.n_frames - 1) // step + 1, groups)
        self._refuse_truncated(res.truncated)
        return res

    # ------------------------------------------------------------------ adaptive common-neighbour analysis (no radius to tune)
    def calculate_adaptive_common_neighbours(self, r_cut,
                                             basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                             basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                             origin_step: int = 1, per_atom: bool = False) -> AdaptiveCommonNeighbours:
        """Adaptive common-neighbour analysis (not in the reference; definition in psa_amd/acna.py), computed on the GPU from
        the positions resident in HBM.  `r_cut`, the species and `origin_step` are those of `calculate_common_neighbours`,
        but `r_cut` is only a generous candidate radius: it must contain the 14 nearest atoms of every centre (up to the
        third shell, usually) and no more than 64.  Every centre ranks its candidates by distance and takes a cut-off of its
        own: (1 + sqrt 2) / 2 of the mean distance of its 12 nearest, among which the signatures of
        `calculate_common_neighbours` make it fcc, hcp or ico; otherwise the 14 nearest with the cut-off of the two bcc
        shells make it bcc or other.  A strained, expanded or two-phase sample needs no radius tuned by hand.
        `signature_counts`, `type_counts`, `fraction(type)`, `signature(j, k, l)` and `share(j, k, l)` are integer counts, the
        same bits for any budget.  `per_atom=True` adds `types`, `neighbours`, `cutoffs`, `nearest`, `bond_signatures`, `atoms`
        and `atoms_of(origin, type)`.

        Where a centre has more than 64 candidates the call raises ValueError naming the species: choose a smaller `r_cut`
        (`Engine.adaptive_common_neighbours` returns the numbers instead).  A sharded calculator refuses
        (NotImplementedError).  Returns a `psa_amd.AdaptiveCommonNeighbours`."""
        self._check_per_atom(per_atom)
        rc, step, groups = self._shell_inputs(r_cut, basis_atom_indices, basis_atom_types, origin_step,
                                              "the adaptive common-neighbour analysis")
        if groups is None:
            return acna.result(acna.empty(1), 0, [np.zeros(0, int)])
        out = self._displacement_run(lambda eng, box: eng.adaptive_common_neighbours(box, rc, groups, step, bool(per_atom)))
        res = acna.result(out, (self.traj.n_frames - 1) // step + 1, groups)
        self._refuse_truncated(res.truncated)
        return res

    # ------------------------------------------------------------------ partial (species-resolved) spectra on that lattice
    def _partial_species(self, basis_atom_indices, basis_atom_types, weights):
        """(the species' atom-index arrays, sum_a w_a^2 per species): resolved like the groups of `calculate_vdos`"""
        groups = self._resolve_groups(basis_atom_indices, basis_atom_types, "incoherent")
        if len(groups) > MAX_SPECIES:
            raise ValueError(f"at most {MAX_SPECIES} species are served, got {len(groups)}")
        members = np.concatenate(groups)
        if np.unique(members).size != members.size:
            raise ValueError("species of partial spectra must be disjoint (an atom is listed twice)")
        w2 = np.ones(self.traj.n_atoms, np.float64) if weights is None else weights.astype(np.float64) ** 2
        return [np.asarray(g) for g in groups], np.array([float(np.sum(w2[g])) for g in groups])

    def calculate_partial_spectra(self, indices: np.ndarray,
                                  basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                  basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                  atom_weights: Optional[np.ndarray] = None, segments: Optional[Segments] = None,
                                  currents: bool = True) -> PartialSpectra:
        """The partial (species-resolved) dynamic spectra on the reciprocal lattice of the simulation box (not in the
        reference; definition in psa_amd/partial.py): per pair a <= b of species the real parts of F^a conj F^b --
        S_ab(k, w) and the partial current correlations C_L^ab, C_T^ab -- for the integer `indices` (K, 3), from one
        projection of every atom.  `PartialSpectra.combine` forms neutron or X-ray totals, the charge-charge and the
        number-number spectrum from them.

        Species are resolved like the groups of `calculate_vdos`: `basis_atom_types=[1, 2]` gives two species, nothing
        gives all atoms as one.  They must be disjoint and at most 8 (ValueError).  Vectors, `atom_weights`, `segments`,
        `currents`, residency, the empty inputs and the sharded refusal are those of `calculate_lattice_spectra`.
        Returns a `psa_amd.PartialSpectra` with (P, L, K) float32 fields, P = S (S + 1) / 2."""
        return self._reciprocal("partial spectra", "spectra", "partial", lambda: self._lattice_vectors(indices),
                                basis_atom_indices, basis_atom_types, atom_weights, segments, currents=currents)

    def calculate_powder_partial_spectra(self, q_edges: np.ndarray,
                                         basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                         basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                         atom_weights: Optional[np.ndarray] = None, segments: Optional[Segments] = None,
                                         currents: bool = True, max_per_bin: Optional[int] = None,
                                         seed: int = 0) -> PowderPartialSpectra:
        """The powder average of `calculate_partial_spectra` (definition in psa_amd/partial.py): S_ab(Q, w), C_L^ab(Q, w)
        and C_T^ab(Q, w) averaged over all vectors of the box's reciprocal lattice in each shell
        q_edges[b] <= |k| < q_edges[b + 1], the shells summed on the GPU in float64.  Shells, `max_per_bin`, `seed`,
        counts and the empty shell are those of `calculate_powder_spectra`; species and everything else those of
        `calculate_partial_spectra`.  Returns a `psa_amd.PowderPartialSpectra` with (P, L, n_bins) float32 fields."""
        return self._reciprocal("powder partial spectra", "spectra", "partial",
                                lambda: self._powder_shells(q_edges, max_per_bin, seed), basis_atom_indices, basis_atom_types,
                                atom_weights, segments, currents=currents)

    # ------------------------------------------------------------------ mode projection
    def calculate_mode_sed(self, k_points_mags: np.ndarray, k_vectors_3d: np.ndarray, eigenvectors: np.ndarray,
                           basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                           basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                           atom_weights: Optional[np.ndarray] = None, segments: Optional[Segments] = None) -> ModeSED:
        """Mode-projected SED (normal-mode decomposition; not in the reference; definition in psa_amd/modes.py):

            Phi[w,k,nu] = | sum_b sum_c conj(eigenvectors[k,nu,b,c]) S_b[k,c,w] |^2

        where S_b is what `calculate` returns for the atom group b ("site b of the primitive cell in every cell"),
        computed on the GPU without the B group spectra ever leaving HBM.

        The B groups are resolved like those of an incoherent `calculate` (`basis_atom_indices` as a list of index
        lists or arrays -- `psa_amd.site_groups(labels)` makes them from a site index per atom -- or
        `basis_atom_types`); they must be disjoint (ValueError).  `eigenvectors` is (K, M, B, 3) complex, used as
        given: no normalisation, M free.  The phase convention is the projection's, exp(+i k.r_a) with each atom's own
        mean position, and the vectors enter conjugated; converting the vectors of a lattice-dynamics code that uses
        another convention is the caller's business.  Pairs (k, -k) are not folded.  `atom_weights` as for `calculate`
        (`psa_amd.mass_weights` for the mass-weighted mode coordinate).  `segments` (keyword only): a
        `psa_amd.Segments` -- the Welch average of the mode spectra over segments of the projected series, taken
        between the projection and the contraction (psa_amd/modes.py): `sed` is then (L, K, M) and `freqs`
        np.fft.fftfreq(L, dt_ps); TypeError for anything else, ValueError if L > T.  A sharded calculator refuses
        (NotImplementedError).  Returns a `psa_amd.ModeSED` with `sed` (T, K, M) float32."""
        weights, eig, k_vectors, groups, empty = self._mode_inputs(k_points_mags, k_vectors_3d, eigenvectors,
                                                                   basis_atom_indices, basis_atom_types, atom_weights, segments)
        if empty is not None:
            return empty
        freqs = np.fft.fftfreq(self.traj.n_frames if segments is None else segments.length, d=self.dt_ps)
        mean_pos_all = self._mean_positions()
        slot, data, flags = self._data_slot()
        eng = self.engine
        with self._engine_state(weights, segments):  # (segments before the upload: its FFT primer then builds length L)
            eng.ensure_resident(slot, data)      # later SED calls find it resident
            run = eng.sed_modes if segments is None else eng.sed_modes_welch
            phi = run(slot, mean_pos_all, k_vectors, self._device_groups(groups), eig.astype(np.complex64), flags)
        return ModeSED(phi, freqs, k_points_mags, k_vectors_3d, [np.asarray(g) for g in groups])

    def _site_inputs(self, k_vectors_3d, basis_atom_indices, basis_atom_types, atom_weights, segments=None,
                     what="the mode-projected SED"):
        """What every projection of site groups checks and resolves, whatever is done with the B spectra: (weights,
        k_vectors (K, 3) float32, the disjoint groups -- None if the trajectory has no frames or no atoms).  `segments`
        are validated as `calculate` validates them; a sharded calculator refuses."""
        weights = None if atom_weights is None else check_atom_weights(atom_weights, self.traj.n_atoms)
        if segments is not None and not isinstance(segments, Segments):
            raise TypeError(f"segments must be a psa_amd.Segments, got {type(segments).__name__}")
        if self._shard is not None and self._shard.nranks > 1:
            raise NotImplementedError(f"{what} is not available on a sharded calculator")
        k_vectors = np.asarray(k_vectors_3d, np.float32).reshape(-1, 3)
        n_t, n_atoms = self.traj.n_frames, self.traj.n_atoms
        if n_t == 0 or n_atoms == 0:
            return weights, k_vectors, None
        if segments is not None:
            segments.count(n_t)                          # ValueError if L > T
        if (basis_atom_types is None and isinstance(basis_atom_indices, (list, tuple)) and len(basis_atom_indices)
                and all(isinstance(g, np.ndarray) for g in basis_atom_indices)):
            # index arrays (`site_groups`) are taken as they are, with the checks of `_resolve_groups`: no detour
            # through Python lists of a whole crystal's atoms
            groups = [g.astype(int).ravel() for g in basis_atom_indices if g.size]
            if any(np.any(g >= n_atoms) or np.any(g < 0) for g in groups):
                raise ValueError("Atom indices in basis out of bounds.")
            if not groups:
                groups = [np.arange(n_atoms)]
        else:
            groups = self._resolve_groups(basis_atom_indices, basis_atom_types, "incoherent")
        members = np.concatenate(groups)
        if np.unique(members).size != members.size:
            raise ValueError("atom groups of a mode projection must be disjoint (an atom is listed twice)")
        return weights, k_vectors, groups

    def _mode_inputs(self, k_points_mags, k_vectors_3d, eigenvectors, basis_atom_indices, basis_atom_types, atom_weights,
                     segments=None):
        """What the mode projections check and resolve: (weights, eig, k_vectors (K, 3) float32, groups, the empty ModeSED
        to return as it is -- no frames, no atoms or no k-vectors -- or None).  `segments` are validated as `calculate`
        validates them."""
        weights, k_vectors, groups = self._site_inputs(k_vectors_3d, basis_atom_indices, basis_atom_types, atom_weights,
                                                       segments)
        eig = np.asarray(eigenvectors)
        n_t, n_k = self.traj.n_frames, len(k_vectors)
        if groups is None:
            logger.warning("Cannot calculate the mode-projected SED: 0 frames or 0 atoms.")
            return weights, eig, k_vectors, [], ModeSED(np.zeros((0, 0, 0), np.float32), np.zeros(0, np.float64), k_points_mags,
                                                        k_vectors_3d, [])
        if eig.ndim != 4 or eig.shape[0] != n_k or eig.shape[2:] != (len(groups), 3) or eig.shape[1] < 1:
            raise ValueError(f"eigenvectors have shape {eig.shape}, expected (K, M, B, 3) = ({n_k}, M, {len(groups)}, 3) "
                             f"for {n_k} k-vectors and {len(groups)} atom groups")
        if not np.all(np.isfinite(eig)):
            raise ValueError("eigenvectors must be finite")
        if n_k == 0:
            logger.warning("k_vectors_3d is empty. Returning ModeSED object with empty data.")
            n_f = n_t if segments is None else segments.length
            return weights, eig, k_vectors, groups, ModeSED(np.zeros((n_f, 0, eig.shape[1]), np.float32),
                                                            np.fft.fftfreq(n_f, d=self.dt_ps), k_points_mags, k_vectors_3d,
                                                            [np.asarray(g) for g in groups])
        return weights, eig, k_vectors, groups, None

    # ------------------------------------------------------------------ spectral covariance, mode vectors
    def calculate_spectral_covariance(self, k_points_mags: np.ndarray, k_vectors_3d: np.ndarray,
                                      basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                                      basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                                      atom_weights: Optional[np.ndarray] = None, freq_weights: np.ndarray) -> np.ndarray:
        """Spectral covariance of the site projections (not in the reference; definition in psa_amd/covariance.py):

            G^(m)[k,i,j] = sum_w g_m[w] S_i[k,w] conj(S_j[k,w])          i = 3b + c, (n_w, K, 3B, 3B) complex128

        where S_b is what `calculate` returns for the atom group b, reduced over frequency on the GPU without the B
        group spectra ever leaving HBM.  Groups, `atom_weights`, empty inputs and the sharded refusal
        (NotImplementedError) are those of `calculate_mode_sed`.  `freq_weights` (keyword only) is (T,) or (n_w, T) with
        n_w 1 or 2, finite, in FFT order and used as given (`psa_amd.spectral_weights` makes the rows of a moment and a
        band); at most 32 groups (3B <= 96).  A trajectory without frames or atoms gives a (n_w, 0, 0, 0) array, an
        empty k-list (n_w, 0, 3B, 3B)."""
        return self._spectral_covariance(k_vectors_3d, basis_atom_indices, basis_atom_types, atom_weights, freq_weights)[0]

    def _spectral_covariance(self, k_vectors_3d, basis_atom_indices, basis_atom_types, atom_weights, freq_weights):
        """(the covariance, the resolved groups -- None without frames or atoms) of `calculate_spectral_covariance`"""
        g = np.asarray(freq_weights, np.float64)
        if g.ndim == 1:
            g = g[None]
        n_t = self.traj.n_frames
        if g.ndim != 2 or g.shape[1] != n_t or not 1 <= g.shape[0] <= 2:
            raise ValueError(f"freq_weights have shape {np.shape(freq_weights)}, expected (T,) or (n_w, T) with T = {n_t} "
                             f"frames and n_w = 1 or 2")
        if not np.all(np.isfinite(g)):
            raise ValueError("freq_weights must be finite")
        weights, k_vectors, groups = self._site_inputs(k_vectors_3d, basis_atom_indices, basis_atom_types, atom_weights,
                                                       what="the spectral covariance")
        if groups is None:
            logger.warning("Cannot calculate the spectral covariance: 0 frames or 0 atoms.")
            return np.zeros((g.shape[0], 0, 0, 0), np.complex128), None
        n = 3 * len(groups)
        if n > _hip.COV_MAX_ROWS:
            raise ValueError(f"the spectral covariance serves at most {_hip.COV_MAX_ROWS // 3} atom groups, got {len(groups)}")
        if len(k_vectors) == 0:
            logger.warning("k_vectors_3d is empty. Returning an empty covariance.")
            return np.zeros((g.shape[0], 0, n, n), np.complex128), groups
        mean_pos_all = self._mean_positions()
        slot, data, flags = self._data_slot()
        eng = self.engine
        with self._engine_state(weights, None):
            eng.ensure_resident(slot, data)      # later SED calls find it resident
            return eng.sed_covariance(slot, mean_pos_all, k_vectors, self._device_groups(groups), g.astype(np.float32), flags), groups

    def calculate_mode_vectors(self, k_points_mags: np.ndarray, k_vectors_3d: np.ndarray,
                               basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                               basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                               atom_weights: Optional[np.ndarray] = None, band=None) -> ModeVectors:
        """Mode vectors and frequencies from the trajectory itself (definition and caveats in psa_amd/covariance.py):
        the displacement covariance G_u and the velocity covariance G_v of the site projections in one GPU call
        (`calculate_spectral_covariance` with two weight rows: the moments (-2, 0) of a velocity calculator, (0, +2) with
        `use_displacements=True`; `band` = (fmin, fmax) THz restricts both), then `psa_amd.mode_vectors` on the host:
        the eigenvectors of G_u, frequency = sqrt(e^+ G_v e / e^+ G_u e) / 2 pi, ascending.  Pass
        `atom_weights=psa_amd.mass_weights(...)`: the method rests on equipartition of the mass-weighted coordinates.
        Degenerate branches return some basis of their subspace.  Returns a `psa_amd.ModeVectors` whose `eigenvectors`
        (K, 3B, B, 3) complex64 are ready to pass to `calculate_mode_sed` / `calculate_mode_peaks`.  Empty inputs as for
        `calculate_mode_sed`: a trajectory without frames or atoms gives (0, 0, 0, 3) vectors and no groups, an empty
        k-list (0, 3B, B, 3), each with a warning."""
        moments = (0, 2) if self.use_displacements else (-2, 0)
        g = np.stack([spectral_weights(self.traj.n_frames, self.dt_ps, m, band) for m in moments]) if self.traj.n_frames \
            else np.zeros((2, 0), np.float32)
        G, groups = self._spectral_covariance(k_vectors_3d, basis_atom_indices, basis_atom_types, atom_weights, g)
        mv = mode_vectors(G[0], G[1])        # (an empty covariance -- logged above -- gives an empty ModeVectors)
        groups = groups or []
        mv.k_points, mv.k_vectors, mv.groups = k_points_mags, k_vectors_3d, [np.asarray(x) for x in groups]
        return mv

    def calculate_mode_peaks(self, k_points_mags: np.ndarray, k_vectors_3d: np.ndarray, eigenvectors: np.ndarray,
                             basis_atom_indices: Optional[Union[List[int], List[List[int]], np.ndarray]] = None,
                             basis_atom_types: Optional[Union[List[int], List[List[int]]]] = None, *,
                             atom_weights: Optional[np.ndarray] = None, return_sed: bool = False, band=None, centers=None,
                             search=None, window_hwhm: float = 8.0, half_window: Optional[float] = None, max_iter: int = 50,
                             segments: Optional[Segments] = None) -> Union[PeakFit, Tuple[PeakFit, ModeSED]]:
        """Frequency and lifetime of every mode (k, nu): `calculate_mode_sed` and a Lorentzian fit of the peak of each of
        its K x M columns (definition in psa_amd/peaks.py), in one pass on the GPU -- the (T, K, M) spectra are fitted
        where they lie and do not cross to the host unless `return_sed` asks for them.

        The projection's arguments, checks, weights and restrictions are those of `calculate_mode_sed` (not sharded).
        `segments`: as there -- the Welch-averaged (L, K, M) spectra are fitted instead, with the frequency step
        1 / (L dt_ps); on thermal data this is what makes the fits converge (a single periodogram is noise of the
        size of the signal), at the price of resolution: choose L so that a peak's half width spans a few bins.
        `band` = (fmin, fmax) THz searched in every column (default: all positive frequencies);
        `centers` (K, M) THz with `search`: each mode's own interval center +- search, for spectra in which a column
        shows more than its own branch; `window_hwhm`, `half_window`, `max_iter` as for `Engine.fit_peaks`.  Returns a
        `psa_amd.PeakFit` with (K, M) fields (`frequency`, `hwhm`, `lifetime`, `status`, ...); with `return_sed`
        (PeakFit, ModeSED)."""
        weights, eig, k_vectors, groups, empty = self._mode_inputs(k_points_mags, k_vectors_3d, eigenvectors,
                                                                   basis_atom_indices, basis_atom_types, atom_weights, segments)
        if empty is not None:
            raise ValueError("nothing to fit: the trajectory has no frames or atoms, or the k-list is empty")
        n_t = self.traj.n_frames if segments is None else segments.length      # frequency bins of the fitted spectra
        freqs = np.fft.fftfreq(n_t, d=self.dt_ps)
        mean_pos_all = self._mean_positions()
        slot, data, flags = self._data_slot()
        eng = self.engine
        with self._engine_state(weights, segments):  # (segments before the upload: its FFT primer then builds length L)
            eng.ensure_resident(slot, data)      # later SED calls find it resident
            run = eng.sed_modes_fit if segments is None else eng.sed_modes_welch_fit
            fit, phi = run(slot, mean_pos_all, k_vectors, self._device_groups(groups), eig.astype(np.complex64),
                           1.0 / (n_t * self.dt_ps), flags, return_sed=return_sed, band=band, centers=centers,
                           search=search, window_hwhm=window_hwhm, half_window=half_window, max_iter=max_iter)
        if not return_sed:
            return fit
        return fit, ModeSED(phi, freqs, k_points_mags, k_vectors_3d, [np.asarray(g) for g in groups])

    # ------------------------------------------------------------------ chiral phase
    def calculate_chiral_phase(self, Z1: np.ndarray, Z2: np.ndarray, angle_range_opt: str = "C") -> np.ndarray:
        """Phase relation of two complex component arrays as float32 (reference :338-371).

        "C": folded difference of arguments in [-pi/2, pi/2]; "A": angle between the two
        phasors in [0, pi]; "B": signed arcsin of their normalised cross product.  A and B
        are evaluated here as whole-array float32 operations (the reference walks them in
        a Python double loop); entries whose |Z|^2 < 1e-18 are 0.
        """
        if Z1.shape != Z2.shape:
            raise ValueError("Z1 and Z2 shapes must match for chiral phase.")
        if Z1.size == 0:
            return np.array([], dtype=np.float32).reshape(Z1.shape)
        if angle_range_opt == "C":
            diff = np.angle(Z1) - np.angle(Z2)
            diff = (diff + np.pi) % (2 * np.pi) - np.pi
            diff = np.where(diff > np.pi / 2, np.pi - diff, diff)
            diff = np.where(diff < -np.pi / 2, -np.pi - diff, diff)
            return diff.astype(np.float32)
        phase = np.zeros(Z1.shape, dtype=np.float32)
        if angle_range_opt not in ("A", "B"):
            logger.warning("Unknown angle_range_opt '%s'. Angle=0.", angle_range_opt)
            return phase
        re1, im1 = np.float32(1) * Z1.real, np.float32(1) * Z1.imag
        re2, im2 = np.float32(1) * Z2.real, np.float32(1) * Z2.imag
        sq1, sq2 = re1 * re1 + im1 * im1, re2 * re2 + im2 * im2
        usable = (sq1 >= 1e-18) & (sq2 >= 1e-18)
        with np.errstate(invalid="ignore", divide="ignore"):
            norm = np.sqrt(sq1) * np.sqrt(sq2)
            if angle_range_opt == "A":
                full = np.arccos(np.clip((re1 * re2 + im1 * im2) / norm, -1.0, 1.0))
            else:
                full = np.arcsin(np.clip((re1 * im2 - im1 * re2) / norm, -1.0, 1.0))
        phase[usable] = full[usable]
        return phase

    # ------------------------------------------------------------------ composites
    def _finish(self, sed: SED, chiral: bool, chiral_axis: str) -> SED:
        """Attach the option-"C" chiral phase of the component pair for `chiral_axis`
        (psa_gui.py:970-999); computed on the GPU from the result still resident there."""
        if not chiral or sed.sed is None or not sed.is_complex:
            return sed
        if sed.sed.ndim != 3 or sed.sed.shape[1] == 0:
            return sed
        c1, c2 = _CHIRAL_PAIR.get(chiral_axis, _CHIRAL_PAIR["z"])
        sed.phase = self.engine.result_chiral_phase(sed.sed.shape[0], sed.sed.shape[1], c1, c2)
        return sed

    def calculate_kpath_sed(self, direction, bz_coverage: float = 1.0, n_k: int = 100,
                            basis_atom_types=None, summation_mode: str = 'coherent',
                            basis_atom_indices=None, lat_param: Optional[float] = None,
                            chiral: bool = False, chiral_axis: str = 'z',
                            k_chunk_size: int = 500, *, atom_weights: Optional[np.ndarray] = None,
                            segments: Optional[Segments] = None) -> SED:
        """k-path dispersion in one call (README.md:100-106; psa_gui.py:947-999).  `atom_weights`, `segments`:
        as for `calculate` (segments and `chiral` exclude each other: the phase needs complex amplitudes)."""
        if chiral and segments is not None:
            raise ValueError("chiral=True needs complex amplitudes; segment-averaged spectra are intensities")
        if chiral and summation_mode != 'coherent':
            logger.info("Chirality calculation selected, forcing coherent summation mode.")
            summation_mode = 'coherent'
        k_mags, k_vecs = self.get_k_path(direction, bz_coverage, n_k, lat_param=lat_param)
        # the phase is computed from the result still on the device: no other calculation on this
        # engine (another thread, another calculator attached to it) may come in between
        with self.engine.lock:
            sed = self.calculate(k_mags, k_vecs, basis_atom_indices=basis_atom_indices,
                                 basis_atom_types=basis_atom_types, summation_mode=summation_mode,
                                 k_chunk_size=k_chunk_size, atom_weights=atom_weights, segments=segments)
            return self._finish(sed, chiral, chiral_axis)

    def calculate_chiral_sed(self, direction, bz_coverage: float = 1.0, n_k: int = 100,
                             chiral_axis: str = 'z', *, atom_weights: Optional[np.ndarray] = None, **kwargs) -> SED:
        """README.md:117-122: a k-path SED with the chiral phase attached.  `atom_weights`: as for
        `calculate`."""
        return self.calculate_kpath_sed(direction, bz_coverage, n_k, chiral=True,
                                        chiral_axis=chiral_axis, atom_weights=atom_weights, **kwargs)

    def calculate_kgrid_sed(self, plane: str = 'xy', k_ranges=(-1.0, 1.0, -1.0, 1.0),
                            n_kx: int = 20, n_ky: int = 20, k_fixed: float = 0.0,
                            basis_atom_types=None, summation_mode: str = 'coherent',
                            basis_atom_indices=None, chiral: bool = False, chiral_axis: str = 'z',
                            k_chunk_size: int = 500, *, atom_weights: Optional[np.ndarray] = None,
                            segments: Optional[Segments] = None) -> SED:
        """2-D k-grid SED in one call (README.md:135-140; psa_gui.py:2135-2191).
        `k_ranges` = (first_min, first_max, second_min, second_max).  `atom_weights`, `segments`: as for
        `calculate` (segments and `chiral` exclude each other)."""
        if chiral and segments is not None:
            raise ValueError("chiral=True needs complex amplitudes; segment-averaged spectra are intensities")
        if chiral and summation_mode != 'coherent':
            logger.info("Chirality calculation selected for K-Grid, forcing coherent summation mode.")
            summation_mode = 'coherent'
        k_mags, k_vecs, shape = self.get_k_grid(plane, (k_ranges[0], k_ranges[1]),
                                                (k_ranges[2], k_ranges[3]), n_kx, n_ky, k_fixed)
        with self.engine.lock:
            sed = self.calculate(k_mags, k_vecs, basis_atom_indices=basis_atom_indices,
                                 basis_atom_types=basis_atom_types, summation_mode=summation_mode,
                                 k_grid_shape=shape, k_chunk_size=k_chunk_size, atom_weights=atom_weights,
                                 segments=segments)
            return self._finish(sed, chiral, chiral_axis)

    # ------------------------------------------------------------------ iSED
    def _ised_groups(self, basis_atom_idx_ised, basis_atom_types_ised) -> List[np.ndarray]:
        """Atom groups of an iSED reconstruction (reference :389-433): indices win over types; a
        flat index list is one group, a flat type list is one group PER type."""
        n_atoms, kinds = self.traj.n_atoms, self.traj.types.astype(int)
        groups: List[np.ndarray] = []
        if basis_atom_idx_ised and len(basis_atom_idx_ised) > 0:
            nested = isinstance(basis_atom_idx_ised[0], list)
            for members in (basis_atom_idx_ised if nested else [basis_atom_idx_ised]):
                arr = np.asarray(members, dtype=int)
                if np.any(arr >= n_atoms) or np.any(arr < 0):
                    raise ValueError(f"Atom indices in group {members} out of bounds." if nested
                                     else "Atom indices out of bounds.")
                if arr.size:
                    groups.append(arr)
            if basis_atom_types_ised and len(basis_atom_types_ised) > 0:
                logger.warning("iSED: atom_indices and atom_types provided. Using atom_indices.")
        elif basis_atom_types_ised and len(basis_atom_types_ised) > 0:
            nested = isinstance(basis_atom_types_ised[0], list)
            for wanted in (basis_atom_types_ised if nested else [[t] for t in basis_atom_types_ised]):
                members = np.flatnonzero(np.isin(kinds, wanted))
                if members.size:
                    groups.append(members)
                else:
                    logger.warning("No atoms for type group %s in iSED.", wanted)
        else:
            groups.append(np.arange(n_atoms))
        return groups

    def _single_bin(self, k_vector: np.ndarray, members: np.ndarray, i_w: int, mean_pos_all: np.ndarray) -> np.ndarray:
        """S[i_w, k, :] (3 complex64) of one k-vector and one atom group: what `calculate(...).sed[i_w, i_k]`
        would hold (reference :58-84 for one k, one frequency)."""
        members = np.asarray(members)
        if np.any(members >= self.traj.n_atoms) or np.any(members < 0):
            raise ValueError("Atom indices in basis out of bounds.")
        if self._shard is not None and self._shard.nranks > 1:     # sharded engines hold partial data
            sed = self.calculate(np.zeros(1, np.float32), np.asarray(k_vector, np.float32)[None, :],
                                 basis_atom_indices=members)
            return sed.sed[i_w, 0, :]
        slot, data, flags = self._data_slot()
        eng = self.engine
        with eng.lock:
            eng.ensure_resident(slot, data)
            group = self._device_groups([members])
            return eng.single_bin(slot, mean_pos_all, k_vector, None if group is None else group[0], i_w, flags)

    def ised(self, k_dir_spec, k_target: float, w_target: float, char_len_k_path: float,
             nk_on_path: int = 100, bz_cov_ised: float = 1.0,
             basis_atom_idx_ised: Optional[List[int]] = None,
             basis_atom_types_ised: Optional[List[int]] = None,
             rescale_factor: Union[str, float] = 1.0, n_recon_frames: int = 100,
             dump_filepath: str = "iSED_reconstruction.dump",
             plot_dir_ised: Optional[Path] = None, plot_max_freq: Optional[float] = None,
             plot_theme: str = 'light') -> None:
        """Inverse SED (reference :373-588): reconstruct the real-space motion of the mode nearest
        to (k_target, w_target) along a k-path and write it as a LAMMPS dump.  Per atom group the
        complex SED comes from `calculate` -- on the GPU, against the trajectory already resident
        in HBM -- and the amplitude A of the selected (w, k) bin is replayed as
        Re[A exp(i tau - i k r.k_hat)] over one period.  Plotting the input spectrum (the
        reference's optional last step) is outside this package; `plot_dir_ised` is ignored."""
        mean_pos = self._mean_positions()              # np.mean(positions, axis=0, dtype=float32), cached per array
        kinds = self.traj.types.astype(int)
        n_atoms = self.traj.n_atoms
        k_hat = parse_direction(k_dir_spec)
        groups = self._ised_groups(basis_atom_idx_ised, basis_atom_types_ised)
        if not groups:
            logger.error("iSED: No atom groups for reconstruction. Aborting.")
            return
        k_mags, k_vecs = self.get_k_path(direction_spec=k_hat, bz_coverage=bz_cov_ised, n_k=nk_on_path,
                                         lat_param=char_len_k_path)
        i_k = int(np.argmin(np.abs(k_mags - k_target)))
        k_used = k_mags[i_k]
        tau = np.linspace(0, 2 * np.pi, n_recon_frames, endpoint=False)
        along_k = np.dot(mean_pos, k_hat)                 # r . k_hat per atom
        motion = np.zeros((n_recon_frames, n_atoms, 4), dtype=np.float32)   # x, y, z, type
        auto = isinstance(rescale_factor, str) and rescale_factor.lower() == "auto"
        peak, spread_sum, spread_atoms = 0.0, 0.0, 0

        # Of each group's path spectrum the reference consumes ONE bin, sed[i_w, i_k, :] (:483,
        # :494-499).  Only that bin is computed: one k-vector projected over the trajectory and one
        # DFT dot (psa_sed_single_bin) instead of nk_on_path projections and 3 nk_on_path FFTs.
        freqs = np.fft.fftfreq(self.traj.n_frames, d=self.dt_ps)
        i_w = int(np.argmin(np.abs(freqs - w_target)))
        for members in groups:
            amplitude = self._single_bin(k_vecs[i_k], members, i_w, mean_pos)
            carrier = np.exp(1j * tau[:, None] - 1j * k_used * along_k[members][None, :])
            for axis in range(3):
                motion[:, members, axis] += np.real(amplitude[axis] * carrier)
            if auto:
                peak = max(peak, float(np.amax(np.abs(motion[:, members, :3]))))
                thermal = self.traj.positions[:, members, :] - mean_pos[None, members, :]
                spread_sum += np.std(thermal) * len(members)
                spread_atoms += len(members)

        motion[0, :, 3] = kinds
        touched = np.unique(np.concatenate(groups))
        if auto:
            if peak > 1e-9:
                motion[:, touched, :3] /= peak
                typical = spread_sum / spread_atoms if spread_atoms > 0 else 0.0
                if typical > 1e-9:
                    motion[:, touched, :3] *= typical
            else:
                logger.warning("iSED: Max wiggle amp near zero. Auto-rescaling ineffective.")
        elif isinstance(rescale_factor, (int, float)):
            motion[:, touched, :3] *= rescale_factor
        out_to_qdump(dump_filepath, mean_pos[None, :, :] + motion[:, :, :3], motion[0, :, 3].astype(int),
                     self.traj.box_matrix)
        logger.info("iSED reconstruction saved: %s", dump_filepath)
        if plot_dir_ised:
            logger.warning("iSED: plotting the input spectrum is not part of psa_amd; plot_dir_ised ignored.")
