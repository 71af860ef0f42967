"""
ctypes binding of libpsa_hip.so (C ABI: include/psa_hip.h).

This is the only door between the Python host code and the GPU.  There is no CPU
implementation behind it: if the library is not built, or no MI355X is visible, every
entry raises -- the caller is never silently routed somewhere else.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref
from pathlib import Path
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libpsa_hip.so"

SLOT_VELOCITIES, SLOT_POSITIONS = 0, 1
F_DISPLACEMENTS, F_INTENSITY = 0x1, 0x2
K1_AUTO, K1_WAVE, K1_MFMA32, K1_SPLIT_BF16 = 0, 1, 2, 3
OPT_PLANES, OPT_PLANES_BUDGET, OPT_PLANES_EAGER, OPT_PLANES_MIN_K, OPT_FOLD_PAIRS, OPT_FFT_PRIME = 0, 1, 2, 3, 4, 5
OPT_K1_LOADER_WAVES = 6
OPT_K1_WIDE = 7
OPT_K1_LOWRANK = 8
OPT_K1_LOWRANK_MIN_K = 9
OPT_K1_LOWRANK_MIN_LOCAL = 10
OPT_VDOS_WORK_BYTES = 11
OPT_MODES_WORK_BYTES = 12
OPT_DYNAMIC_WORK_BYTES = 13
OPT_K1_LOWRANK_PAIR = 15        # (14 is not assigned)
KMAP_MIRROR = 0x80000000
ABI_VERSION = 6
# the summation structure of the covariance kernel (psa_amd/csrc/covariance.hip), mirrored for the bound of tests/cov64.py
COV_CHAIN = 128     # frequencies one float32 accumulator sums before it is folded
COV_FOLDS = 32      # folds into the second float32 sum per partial slab
COV_TILE = 64       # frequencies per staged tile
COV_CHUNK = COV_CHAIN * COV_FOLDS   # frequencies per workgroup and partial slab
COV_MAX_ROWS = 96   # 3 B served
# the summation structure of the dynamic-spectra kernel (psa_amd/csrc/dynamic.hip), mirrored for the bound of
# tests/dynamic_cases.py
DYN_THREADS = 256   # lanes of a workgroup: k-vectors x atom slices
DYN_ATOMS = 512     # atoms of a frame staged per tile
DYN_CHAIN = 128     # atoms one float32 accumulator sums before it is folded
DYN_FRAMES = 4      # frames per workgroup
DYN_SINCOS_ERR = 2.6e-7      # twice the largest error of v_sin_f32 / v_cos_f32 measured on [-2, 2] turns: 1.253e-7
# the summation structure of the lattice-spectra kernel (psa_amd/csrc/lattice.hip), mirrored for the bound of
# tests/lattice_cases.py
LAT_THREADS = 256   # lanes of a workgroup
LAT_KS = 512        # vectors of a tile: two per lane
LAT_ATOMS = 128     # most atoms of a frame staged per tile
LAT_TABLE = 3584    # entries of the per-atom factor tables in LDS
LAT_CHAIN = 128     # atoms one float32 accumulator sums before it is folded
LAT_FRAMES = 4      # frames per workgroup
LAT_MAX_INDEX = 64  # largest |n_j| served
LAT_MAX_ENTRIES = 3 * (2 * LAT_MAX_INDEX + 1)
PARTIAL_MAX_SPECIES = 8   # most species of a partial-spectra call (psa_amd/csrc/partial.hip): 36 pairs
# the tiles of the self-spectra series kernel (psa_amd/csrc/self.hip), mirrored for the cases of tests/self_cases.py
SELF_THREADS = 256  # lanes of a workgroup: SELF_ATOMS wavefronts, a lane per frame
SELF_ATOMS = 4      # atoms of an atom tile
SELF_FRAMES = 64    # frames of a frame tile
SELF_ENTRIES = 24   # most distinct (axis, m) pairs of a vector tile
SELF_KS = 64        # most vectors of a vector tile
# the tiles and caps of the displacement kernels (psa_amd/csrc/msd.hip), mirrored for the bounds of tests/msd_cases.py
MSD_LAGS = 256         # lags of a lag tile, one per lane
MSD_ORIGINS = 1024     # most origins of an origin tile
MSD_WINDOW = 1280      # most frames of u64 staged per atom, origin tile and lag tile
MSD_MAX_GROUPS = 8     # most atom groups of a call
MSD_MAX_BINS = 1024    # most bins of a van Hove histogram
MSD_MAX_VH_LAGS = 64   # most lags of a van Hove call
MSD_UNWRAP_FRAMES = 64  # frames of an unwrap tile
MSD_UNWRAP_ATOMS = 16   # atoms of an unwrap tile
# the caps of the self-overlap kernels (psa_amd/csrc/overlap.hip)
OVERLAP_MAX_LAGS = 256  # most lags of a self-overlap call
# the tile and caps of the pair kernels (psa_amd/csrc/pair.hip)
PAIR_TILE = 256        # alpha-atoms of a workgroup and beta-atoms of a staged tile
PAIR_MAX_BINS = 1024   # most bins of a pair histogram
PAIR_MAX_LAGS = 64     # most lags of a pair call
PAIR_MAX_SPECIES = 8   # most species of a pair call
# the caps of the angle kernels (psa_amd/csrc/angle.hip)
ANGLE_MAX_NEIGHBOURS = 64   # most neighbours a centre holds, all species together
ANGLE_MAX_BINS = 1024       # most bins of an angle histogram
# the caps of the order kernel (psa_amd/csrc/order.hip)
ORDER_MAX_L = 12        # the largest order l of a Steinhardt parameter q_l
ORDER_MAX_LS = 8        # most orders of a call
ORDER_MAX_BINS = 1024   # most bins of a q histogram
ORDER_SHIFT = 24        # X_l counts units of 2^-24: q_l^2 = X_l / (n^2 2^24)
# the caps of the local order kernels (psa_amd/csrc/qlm.hip)
LOCAL_MAX_LS = 4        # most orders of a call, even ones in [2, ORDER_MAX_L]
LOCAL_MAX_BINS = 1024   # most bins of a q-bar histogram and of a w histogram
LOCAL_SHIFT = 40        # Q_lm counts units of 2^-40
# the caps of the cluster kernels (psa_amd/csrc/cluster.hip)
CLUSTER_MAX_SIZES = 4096    # most exact slots of the cluster-size histogram
CLUSTER_ROW_WORDS = ANGLE_MAX_NEIGHBOURS + 1 + 4   # a species' row: connections[65], truncated, isolated, undefined, incomplete
CLUSTER_LINKS = ("neighbours", "solid_bonds")      # link 0, 1
# the cap of the persistence kernels (psa_amd/csrc/persist.hip)
PERSIST_MAX_LAGS = 1024     # most lags of a call
# the table of the common-neighbour kernels (psa_amd/csrc/cna.hip)
CNA_TABLE = (8, 16, 16)     # the signatures (j, k, l) the table holds: j < 8, k < 16, l < 16
CNA_TYPES = ("other", "fcc", "hcp", "bcc", "ico")   # type 0 .. 4
# the members of the adaptive common-neighbour kernel (psa_amd/csrc/acna.hip)
ACNA_MEMBERS = 14           # the nearest candidates a centre's per-bond rows hold: 12 of test A, 14 of test B
UNIQUE_ID_BYTES = 128
TIMING_NAMES = ("h2d", "phase", "project", "fft", "epilogue", "gather", "transpose", "d2h")

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)
_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
_ctx = C.c_void_p

# name -> (restype, argtypes); must list every symbol include/psa_hip.h declares
SIGNATURES = {
    "psa_abi_version": (C.c_int, []),
    "psa_last_error": (C.c_char_p, []),
    "psa_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "psa_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "psa_host_free": (C.c_int, [C.c_void_p]),
    "psa_create": (C.c_int, [C.c_int, C.POINTER(_ctx)]),
    "psa_destroy": (C.c_int, [_ctx]),
    "psa_synchronize": (C.c_int, [_ctx]),
    "psa_set_k1": (C.c_int, [_ctx, C.c_int]),
    "psa_set_k1_lowrank_fold": (C.c_int, [_ctx, C.c_int]),
    "psa_set_k1_lowrank_nodes": (C.c_int, [_ctx, C.c_int]),
    "psa_set_option": (C.c_int, [_ctx, C.c_int, C.c_int64]),
    "psa_device_info": (C.c_int, [_ctx, C.c_char_p, C.c_int, C.POINTER(C.c_int), _i64p]),
    "psa_data_upload": (C.c_int, [_ctx, C.c_int, _f32p, C.c_int64, C.c_int64]),
    "psa_data_alloc": (C.c_int, [_ctx, C.c_int, C.c_int64, C.c_int64]),
    "psa_data_download": (C.c_int, [_ctx, C.c_int, _f32p, C.c_int64, C.c_int64]),
    "psa_data_release": (C.c_int, [_ctx, C.c_int]),
    "psa_data_shape": (C.c_int, [_ctx, C.c_int, _i64p, _i64p]),
    "psa_data_fill_synthetic": (C.c_int, [_ctx, C.c_int, C.c_uint64, C.c_int64, C.c_int, _f32p, _i32p,
                                          _f32p, _f32p, _f32p, _f32p]),
    "psa_mean_positions": (C.c_int, [_ctx, C.c_int, _f32p]),
    "psa_host_mean_frames": (C.c_int, [_f32p, C.c_int64, C.c_int64, _f32p, C.c_int]),
    "psa_set_atom_weights": (C.c_int, [_ctx, _f32p, C.c_int64]),
    "psa_set_segments": (C.c_int, [_ctx, C.c_int64, C.c_int64, _f32p]),
    "psa_sed_project": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, C.c_int64, C.c_int64,
                                  _i32p, _i64p, C.c_int32, C.c_int32]),
    "psa_sed_project_upload": (C.c_int, [_ctx, C.c_int, _f32p, C.c_int64, C.c_int64, _f32p, _f32p, C.c_int64,
                                         _i32p, _i64p, C.c_int32, C.c_int32]),
    "psa_sed_finalize": (C.c_int, [_ctx, C.c_void_p, C.c_size_t, _f32p, C.c_size_t]),
    "psa_sed_calculate": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p, _i64p,
                                    C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, _f32p, C.c_size_t]),
    "psa_vdos": (C.c_int, [_ctx, C.c_int, _f32p, _i32p, _i64p, C.c_int32, C.c_int32, _f32p, C.c_size_t]),
    "psa_sed_modes": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p, _i64p, C.c_int32, C.c_void_p, C.c_int64,
                                C.c_int32, _f32p, C.c_size_t]),
    "psa_fit_peaks": (C.c_int, [_ctx, _f32p, C.c_int64, C.c_int64, C.c_double, _i32p, C.c_int32, C.c_int32, C.c_void_p,
                                _f32p, _i32p]),
    "psa_sed_modes_fit": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p, _i64p, C.c_int32, C.c_void_p, C.c_int64,
                                    C.c_int32, C.c_double, _i32p, C.c_int32, C.c_int32, C.c_void_p, _f32p, _i32p, _f32p,
                                    C.c_size_t]),
    "psa_sed_modes_welch": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p, _i64p, C.c_int32, C.c_void_p, C.c_int64,
                                      C.c_int32, _f32p, C.c_size_t]),
    "psa_sed_modes_welch_fit": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p, _i64p, C.c_int32, C.c_void_p,
                                          C.c_int64, C.c_int32, C.c_double, _i32p, C.c_int32, C.c_int32, C.c_void_p, _f32p,
                                          _i32p, _f32p, C.c_size_t]),
    "psa_dynamic_spectra": (C.c_int, [_ctx, _f32p, C.c_int64, _i32p, C.c_int64, C.c_int32, _f32p, C.c_size_t]),
    "psa_debug_dynamic_project": (C.c_int, [_ctx, _f32p, C.c_int64, _i32p, C.c_int64, C.c_int32, C.c_void_p]),
    "psa_debug_dynamic_sincos": (C.c_int, [_ctx, _f32p, C.c_int64, _f32p]),
    "psa_lattice_spectra": (C.c_int, [_ctx, _f64p, _i32p, C.c_int64, _i32p, C.c_int64, _i32p, C.c_int64, C.c_int32,
                                      _f32p, C.c_size_t]),
    "psa_debug_lattice_project": (C.c_int, [_ctx, _f64p, _i32p, C.c_int64, _i32p, C.c_int64, C.c_int32, C.c_void_p]),
    "psa_self_spectra": (C.c_int, [_ctx, _f64p, _i32p, C.c_int64, _i32p, C.c_int64, _i32p, C.c_int64, _f32p,
                                   C.c_size_t]),
    "psa_debug_self_series": (C.c_int, [_ctx, _f64p, _i32p, C.c_int64, _i32p, C.c_int64, C.c_void_p]),
    "psa_debug_dynamic_power": (C.c_int, [_ctx, C.c_void_p, _f32p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_float, _f32p]),
    "psa_debug_lattice_shell": (C.c_int, [_ctx, C.c_void_p, _f32p, _i32p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64,
                                          C.c_int64, C.c_int64, C.c_double, _f32p]),
    "psa_debug_self_power": (C.c_int, [_ctx, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _i32p, C.c_int64, C.c_int64,
                                       _f64p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _f32p]),
    "psa_partial_spectra": (C.c_int, [_ctx, _f64p, _i32p, C.c_int64, _i32p, C.c_int64, _i32p, _i64p, C.c_int32,
                                      C.c_int32, _f32p, C.c_size_t]),
    "psa_debug_partial_project": (C.c_int, [_ctx, _f64p, _i32p, C.c_int64, _i32p, _i64p, C.c_int32, C.c_int32,
                                            C.c_void_p]),
    "psa_debug_partial_power": (C.c_int, [_ctx, C.c_void_p, _f32p, _i32p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64,
                                          C.c_int64, C.c_int64, C.c_int64, C.c_double, _f32p]),
    "psa_lattice_correlations": (C.c_int, [_ctx, _f64p, _i32p, C.c_int64, _i32p, C.c_int64, _i32p, C.c_int64,
                                           C.c_int32, C.c_int64, _f32p, C.c_size_t]),
    "psa_self_correlations": (C.c_int, [_ctx, _f64p, _i32p, C.c_int64, _i32p, C.c_int64, _i32p, C.c_int64,
                                        C.c_int64, _f32p, C.c_size_t]),
    "psa_debug_correlation_transform": (C.c_int, [_ctx, _f64p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                  C.c_int64, C.c_int64, C.c_int32, _f32p]),
    "psa_displacement_moments": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, C.c_int64,
                                           C.c_int64, C.c_int32, _f64p, C.c_size_t]),
    "psa_van_hove_self": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _i64p, C.c_int64,
                                    C.c_int64, C.c_int32, C.c_double, C.c_int32, _u64p, C.c_size_t]),
    "psa_self_overlap": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _i64p, C.c_int64,
                                   C.c_int64, C.c_int32, C.c_double, _u64p, C.c_size_t, _u32p, C.c_size_t]),
    "psa_debug_unwrap": (C.c_int, [_ctx, _f64p, _f64p, _i32p, C.c_int64, C.c_int32,
                                   _f64p, _i32p]),
    "psa_pair_histogram": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _i64p, C.c_int64,
                                     C.c_int64, C.c_double, C.c_int32, _u64p, C.c_size_t]),
    "psa_debug_pair_fractions": (C.c_int, [_ctx, _f64p, _i32p, C.c_int64, _f32p]),
    "psa_debug_pair_plan": (C.c_int, [_i64p, C.c_int32, C.c_int32, C.c_int64, _i64p]),
    "psa_angle_histogram": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _f64p,
                                      C.c_int64, C.c_int32, _u64p, C.c_size_t, _u64p, C.c_size_t,
                                      _u64p]),
    "psa_debug_neighbour_lists": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32,
                                            _f64p, C.c_int64, _i32p, _i32p]),
    "psa_bond_order": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _f64p, C.c_int64,
                                 _i32p, C.c_int32, C.c_int32, _u64p, C.c_size_t, _u64p, _u64p, _u64p,
                                 _i64p, _i32p]),
    "psa_local_order": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _f64p, C.c_int64,
                                  _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_double,
                                  _f64p, C.c_int64, _u64p, C.c_size_t, _f64p, _f64p, _f64p, _i32p, _i32p]),
    "psa_debug_qlm": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _f64p, C.c_int64,
                                _i32p, C.c_int32, _i64p]),
    "psa_solid_clusters": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _f64p, C.c_int64,
                                     C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, _u64p, _u64p, _u64p,
                                     _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _u64p]),
    "psa_bond_persistence": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _f64p, _f64p, C.c_int64,
                                       _i64p, C.c_int32, C.c_int64, C.c_int32, _u64p, _u64p, _u64p, C.c_size_t,
                                       _u64p, C.c_size_t, _u64p, C.c_size_t, _u64p, _u64p, C.c_size_t]),
    "psa_common_neighbours": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _f64p, C.c_int64, _u64p, C.c_size_t,
                                        _u64p, _u64p, C.c_size_t, _u64p, _i32p, _i32p, C.c_size_t, C.POINTER(C.c_uint32),
                                        C.c_size_t]),
    "psa_adaptive_common_neighbours": (C.c_int, [_ctx, _f64p, _f64p, _i32p, _i64p, C.c_int32, _f64p, C.c_int64, _u64p, C.c_size_t,
                                                 _u64p, _u64p, C.c_size_t, _u64p, _u64p, _i32p, _i32p, _f32p, C.c_size_t, _i32p,
                                                 C.POINTER(C.c_uint32), C.c_size_t]),
    "psa_debug_cluster_labels": (C.c_int, [_ctx, C.c_int64, C.c_int64, _i32p, _i32p, C.POINTER(C.c_uint8), _u64p, C.c_int32,
                                           C.c_int32, _u64p, _u64p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p]),
    "psa_k_pairs": (C.c_int, [_f32p, C.c_int64, _i32p, _i32p, _i64p]),
    "psa_lowrank_plan": (C.c_int, [_f32p, C.c_int64, _f32p, C.c_int64, _i32p, C.c_int64, _i32p, _f64p,
                                   _f64p, _f32p, _f32p, _f32p]),
    "psa_sed_set_kmap": (C.c_int, [_ctx, _i32p, C.c_int64]),
    "psa_sed_single_bin": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, _i32p, C.c_int64, C.c_int32, C.c_int64, _f32p]),
    "psa_slab_read": (C.c_int, [_ctx, C.c_int64, C.c_int64, C.c_void_p]),
    "psa_slab_write": (C.c_int, [_ctx, C.c_int64, C.c_int64, C.c_void_p]),
    "psa_result_intensity": (C.c_int, [_ctx, _f32p, C.c_size_t]),
    "psa_result_chiral_phase": (C.c_int, [_ctx, C.c_int, C.c_int, _f32p, C.c_size_t]),
    "psa_last_timings": (C.c_int, [_ctx, _f64p]),
    "psa_k1_stats": (C.c_int, [_ctx, _i64p, _f64p]),
    "psa_k1_lowrank_launches": (C.c_int, [_ctx, _i64p]),
    "psa_k1_lowrank_pair_launches": (C.c_int, [_ctx, _i64p]),
    "psa_lowrank_pair_image": (C.c_int, [C.c_int32, _i64p, _i64p]),
    "psa_lowrank_fold_image": (C.c_int, [C.c_int32, _i64p, _i64p]),
    "psa_lowrank_n48_image": (C.c_int, [C.c_int32, _i64p, _i64p]),
    "psa_lowrank_plan_nodes": (C.c_int, [_f32p, C.c_int64, _f32p, C.c_int64, _i32p, C.c_int64, C.c_int32, _i32p, _f64p, _f64p, _f32p,
                                         _f32p, _f32p]),
    "psa_oneoff_stats": (C.c_int, [_ctx, _f64p]),
    "psa_option_info": (C.c_int, [C.c_int, C.POINTER(C.c_int32), _i64p, C.POINTER(C.c_char_p)]),
    "psa_debug_device_buffers": (C.c_int, [_i64p, _i64p]),
    "psa_debug_scratch_info": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int32)]),
    "psa_debug_scratch_fill": (C.c_int, [_ctx, C.c_int, _i64p, _i64p]),
    "psa_debug_phase_table": (C.c_int, [_ctx, _f32p, _f32p, C.c_int64, _i32p, C.c_int64,
                                        C.c_int64, C.c_void_p]),
    "psa_debug_project_only": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p,
                                         C.c_int64, C.c_int32, C.c_void_p]),
    "psa_debug_project_route": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p,
                                          C.c_int64, C.c_int32, C.c_void_p]),
    "psa_debug_project_frames": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p,
                                           C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]),
    "psa_debug_mode_power": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _f32p]),
    "psa_debug_mode_power_welch": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                             C.c_int64, C.c_int64, C.c_float, _f32p]),
    "psa_sed_covariance": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p, _i64p, C.c_int32, _f32p, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_size_t]),
    "psa_debug_covariance": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, _f32p, C.c_int32, C.c_double,
                                       C.c_void_p]),
    "psa_debug_plane_cache": (C.c_int, [_ctx, _i64p, _i64p]),
    "psa_comm_unique_id": (C.c_int, [C.c_void_p]),
    "psa_comm_init": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int]),
    "psa_comm_destroy": (C.c_int, [_ctx]),
    "psa_comm_selftest": (C.c_int, [_ctx]),
    "psa_sed_gather": (C.c_int, [_ctx, C.c_int, _i64p, _i64p]),
    "psa_comm_barrier": (C.c_int, [_ctx]),
    "psa_sed_fs_project": (C.c_int, [_ctx, C.c_int, _f32p, _f32p, C.c_int64, _i32p, C.c_int64, C.c_int32,
                                     C.c_int64, C.c_int64, C.c_int64]),
    "psa_sed_fs_exchange": (C.c_int, [_ctx, _i64p, _i64p, _i64p, _i64p]),
    "psa_sed_fs_read": (C.c_int, [_ctx, C.c_int64, C.c_int64, C.c_void_p]),
    "psa_sed_fs_write": (C.c_int, [_ctx, C.c_int64, C.c_int64, C.c_void_p]),
    "psa_sed_fs_finish": (C.c_int, [_ctx, C.c_int32]),
}


class PeakOpts(C.Structure):
    """psa_peak_opts"""
    _fields_ = [("window_hwhm", C.c_float), ("half_window_bins", C.c_int32), ("max_iter", C.c_int32)]


class PsaHipError(RuntimeError):
    """A libpsa_hip entry point returned a non-zero code."""


_lib = None
_lib_lock = threading.Lock()


def load_library() -> C.CDLL:
    """dlopen libpsa_hip.so and bind every declared symbol.  Raises if it is missing."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = Path(os.environ.get("PSA_HIP_LIBRARY", LIB_PATH))
        if not path.exists():
            raise PsaHipError(
                f"{path} not found: build it with `make -C psa_amd/csrc` (needs hipcc, gfx950). "
                "psa_amd has no CPU fallback.")
        # multi-process runs (psa_amd/dist.py): the host driver of this pool supports dmabuf IPC only, and the
        # HSA runtime reads this when the first HIP call initialises it -- so it is set before the library
        # (and with it HIP) is loaded; a launcher's own setting wins
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        lib = C.CDLL(str(path))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the .so lacks a symbol
            fn.restype, fn.argtypes = res, args
        _lib = lib
        return lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = load_library().psa_last_error().decode("utf-8", "replace")
        if rc == -1 and "out of bounds" in msg:      # same exception type as the reference
            raise ValueError(msg)
        raise PsaHipError(f"{what} failed (rc={rc}): {msg}")


def _f32(a: np.ndarray):
    return a.ctypes.data_as(_f32p)


def _as_f32(a, shape_tail=None) -> np.ndarray:
    arr = np.ascontiguousarray(a, dtype=np.float32)
    if shape_tail is not None and arr.shape[1:] != shape_tail:
        raise ValueError(f"expected (*,{shape_tail}) array, got {arr.shape}")
    return arr


def device_count() -> int:
    n = C.c_int(0)
    _check(load_library().psa_device_count(C.byref(n)), "psa_device_count")
    return n.value


def option_table():
    """[(id, name, default)] of every option of psa_set_option, from the library's own table (psa_option_info; host
    only): the one source of the defaults."""
    lib, rows = load_library(), []
    opt, default, name = C.c_int32(0), C.c_int64(0), C.c_char_p()
    while lib.psa_option_info(len(rows), C.byref(opt), C.byref(default), C.byref(name)) == 0:
        rows.append((opt.value, name.value.decode(), default.value))
    return rows


def device_buffers():
    """(count, bytes) of the device allocations the library's contexts hold right now, process-wide
    (psa_debug_device_buffers; host only).  A closed Engine leaves none behind."""
    n, b = C.c_int64(0), C.c_int64(0)
    _check(load_library().psa_debug_device_buffers(C.byref(n), C.byref(b)), "psa_debug_device_buffers")
    return n.value, b.value


SCRATCH_CLASSES = ("real", "index", "state")


def scratch_table():
    """[(name, class)] of every device buffer of a context, class one of SCRATCH_CLASSES, from the library's own table
    (psa_debug_scratch_info; host only)."""
    lib, rows = load_library(), []
    name, cls = C.c_char_p(), C.c_int32(0)
    while lib.psa_debug_scratch_info(len(rows), C.byref(name), C.byref(cls)) == 0:
        rows.append((name.value.decode(), SCRATCH_CLASSES[cls.value]))
    return rows


def k_pairs(k_vectors):
    """(kmap uint32 (K,), unique_idx int32 (U,)): pairs (k, -k) and repeated vectors of a k-list
    (psa_k_pairs; bit 31 of kmap = the vector is the exact negation of row kmap & 0x7fffffff)."""
    kv = _as_f32(k_vectors, (3,)) if len(k_vectors) else np.zeros((0, 3), np.float32)
    K = kv.shape[0]
    kmap, uidx, n = np.zeros(K, np.int32), np.zeros(K, np.int32), C.c_int64(0)
    _check(load_library().psa_k_pairs(_f32(kv), K, kmap.ctypes.data_as(_i32p), uidx.ctypes.data_as(_i32p), C.byref(n)),
           "psa_k_pairs")
    return kmap.view(np.uint32), uidx[:n.value].copy()


def lowrank_plan(k_vectors, mean_pos_all, idx=None):
    """The low-rank plan of a k-list for one atom group (psa_lowrank_plan; host only): None when the list stays on
    the dense kernels, else a dict with u, k0, x_c, h_x, width, interval, d_bound, dscale, e_bound, dscale_fold (the
    bound on |E| and the scale of the folded image D + E, Engine.set_lowrank_fold), kappa (64,) and C (K, 64) complex64, and
    C's two factors L (K, 64) float32 and phi (K,) complex64."""
    kv = _as_f32(k_vectors, (3,))
    mean = _as_f32(mean_pos_all, (3,))
    K, N = kv.shape[0], mean.shape[0]
    ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
    n_g = N if ix is None else ix.size
    ok, geo = C.c_int32(0), np.zeros(14, np.float64)
    kappa, cm = np.zeros(64, np.float64), np.zeros((K, 64), np.complex64)
    lw, phi = np.zeros((K, 64), np.float32), np.zeros(K, np.complex64)
    _check(load_library().psa_lowrank_plan(_f32(kv), K, _f32(mean), N, None if ix is None else ix.ctypes.data_as(_i32p), n_g,
                                           C.byref(ok), geo.ctypes.data_as(_f64p), kappa.ctypes.data_as(_f64p),
                                           cm.ctypes.data_as(_f32p), _f32(lw), phi.ctypes.data_as(_f32p)), "psa_lowrank_plan")
    if not ok.value:
        return None
    return {"u": geo[0:3].copy(), "k0": geo[3:6].copy(), "x_c": geo[6], "h_x": geo[7], "width": geo[8],
            "interval": int(geo[9]), "d_bound": geo[10], "dscale": geo[11], "e_bound": geo[12],
            "dscale_fold": geo[13], "kappa": kappa, "C": cm, "L": lw, "phi": phi}


def lowrank_plan_nodes(k_vectors, mean_pos_all, idx=None, nodes=48):
    """lowrank_plan for a plan of `nodes` = 48 or 64 Chebyshev nodes (psa_lowrank_plan_nodes; host only;
    Engine.set_k1_lowrank_nodes): kappa (nodes,), C and L (K, nodes), and beside lowrank_plan's keys r_bound -- with 48 nodes
    the largest |P_line - phi L W| over the rows and the group's atoms, which the D image absorbs; dscale_fold then comes
    from d_bound + e_bound + 1e-6, the cap on r_bound."""
    kv = _as_f32(k_vectors, (3,))
    mean = _as_f32(mean_pos_all, (3,))
    K, N, nodes = kv.shape[0], mean.shape[0], int(nodes)
    ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
    n_g = N if ix is None else ix.size
    ok, geo = C.c_int32(0), np.zeros(15, np.float64)
    kappa, cm = np.zeros(nodes, np.float64), np.zeros((K, nodes), np.complex64)
    lw, phi = np.zeros((K, nodes), np.float32), np.zeros(K, np.complex64)
    _check(load_library().psa_lowrank_plan_nodes(_f32(kv), K, _f32(mean), N, None if ix is None else ix.ctypes.data_as(_i32p), n_g,
                                                 nodes, C.byref(ok), geo.ctypes.data_as(_f64p), kappa.ctypes.data_as(_f64p),
                                                 cm.ctypes.data_as(_f32p), _f32(lw), phi.ctypes.data_as(_f32p)),
           "psa_lowrank_plan_nodes")
    if not ok.value:
        return None
    return {"u": geo[0:3].copy(), "k0": geo[3:6].copy(), "x_c": geo[6], "h_x": geo[7], "width": geo[8],
            "interval": int(geo[9]), "d_bound": geo[10], "dscale": geo[11], "e_bound": geo[12],
            "dscale_fold": geo[13], "r_bound": geo[14], "nodes": nodes, "kappa": kappa, "C": cm, "L": lw, "phi": phi}


def lowrank_n48_image(n_stage: int):
    """The D image of the low-rank route's 48-node pair launch (psa_lowrank_n48_image; host only) for n_stage 32-atom
    stages: (index, nbytes) as lowrank_pair_image, rows 0..159 in role A's part and rows 160..511 in role B's."""
    index, nbytes = np.zeros((512, 32 * int(n_stage)), np.int64), C.c_int64(0)
    _check(load_library().psa_lowrank_n48_image(int(n_stage), index.ctypes.data_as(_i64p), C.byref(nbytes)), "psa_lowrank_n48_image")
    return index, nbytes.value


def lowrank_pair_image(n_stage: int):
    """The D image of the low-rank route's pair launch (psa_lowrank_pair_image; host only) for n_stage 32-atom stages:
    (index, nbytes) with index (512, 32 n_stage) int64, the float16 element of (row, atom), and the image's size in
    bytes, padding stages included."""
    index, nbytes = np.zeros((512, 32 * int(n_stage)), np.int64), C.c_int64(0)
    _check(load_library().psa_lowrank_pair_image(int(n_stage), index.ctypes.data_as(_i64p), C.byref(nbytes)), "psa_lowrank_pair_image")
    return index, nbytes.value


def lowrank_fold_image(n_stage: int):
    """The folded D image of the low-rank route's folded pair launch (psa_lowrank_fold_image; host only) for n_stage
    32-atom stages: (index, nbytes) as lowrank_pair_image, rows 0..127 in role A's part and rows 128..511 in role B's."""
    index, nbytes = np.zeros((512, 32 * int(n_stage)), np.int64), C.c_int64(0)
    _check(load_library().psa_lowrank_fold_image(int(n_stage), index.ctypes.data_as(_i64p), C.byref(nbytes)), "psa_lowrank_fold_image")
    return index, nbytes.value


def host_mean_frames(x: np.ndarray, threads: int = 0) -> np.ndarray:
    """np.mean(x, axis=0, dtype=np.float32) of a C-contiguous float32 (T, ...) array, bit for bit, on
    several host threads (psa_host_mean_frames)."""
    if x.dtype != np.float32 or not x.flags.c_contiguous or x.ndim < 2 or x.shape[0] < 1 or x.size == 0:
        raise ValueError("host_mean_frames needs a non-empty C-contiguous float32 array")
    out = np.empty(x.shape[1:], np.float32)
    cols = int(np.prod(x.shape[1:], dtype=np.int64))
    _check(load_library().psa_host_mean_frames(_f32(x), x.shape[0], cols, _f32(out), int(threads)), "psa_host_mean_frames")
    return out


def pack_groups(groups: Optional[Sequence[np.ndarray]]):
    """list of index arrays -> (idx int32, off int64, G) for the ABI; None -> all atoms."""
    if groups is None:
        return None, None, 1
    off = np.zeros(len(groups) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(g) for g in groups])
    idx = (np.concatenate([np.asarray(g).ravel() for g in groups]) if off[-1] > 0
           else np.zeros(0, dtype=np.int64))
    if idx.size and (idx.min() < 0 or idx.max() >= 2 ** 31):
        raise ValueError("Atom indices in basis out of bounds.")
    return np.ascontiguousarray(idx, dtype=np.int32), off, len(groups)


class _PinnedPool:
    """Page-locked host buffers for result arrays, recycled by size.  A buffer goes back to the pool
    when the last NumPy view of it is garbage-collected; at most `keep_bytes` idle bytes are kept."""

    granule = 2 << 20
    min_bytes = 1 << 20                     # smaller results: ordinary memory
    keep_bytes = 4 << 30                    # idle buffers kept for reuse
    max_live_bytes = 16 << 30               # page-locked bytes handed out and not yet collected: beyond
                                            # this, results go to ordinary memory

    def __init__(self):
        self._idle = {}                     # size -> [address, ...]
        self._idle_bytes = 0
        self._live_bytes = 0
        self._lock = threading.Lock()
        self.stats = {"recycled": 0, "allocated": 0, "pageable": 0}    # results of >= min_bytes, by how they were served

    def _give_back(self, address: int, size: int):
        with self._lock:
            self._live_bytes -= size
            if self._idle_bytes + size <= self.keep_bytes:
                self._idle.setdefault(size, []).append(address)
                self._idle_bytes += size
                return
        load_library().psa_host_free(C.c_void_p(address))

    def empty(self, shape, dtype) -> np.ndarray:
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if nbytes < self.min_bytes:
            return np.empty(shape, dtype)
        size = -(-nbytes // self.granule) * self.granule
        with self._lock:
            if self._live_bytes + size > self.max_live_bytes:
                self.stats["pageable"] += 1
                return np.empty(shape, dtype)
            self._live_bytes += size
            stack = self._idle.get(size)
            address = stack.pop() if stack else None
            if address is not None:
                self._idle_bytes -= size
        if address is None:
            p = C.c_void_p()
            try:
                _check(load_library().psa_host_alloc(size, C.byref(p)), "psa_host_alloc")
            except PsaHipError:             # e.g. the locked-memory limit: an ordinary array will do
                with self._lock:
                    self._live_bytes -= size
                    self.stats["pageable"] += 1
                return np.empty(shape, dtype)
            address = p.value
            self.stats["allocated"] += 1
        else:
            self.stats["recycled"] += 1
        block = (C.c_char * size).from_address(address)
        weakref.finalize(block, self._give_back, address, size)     # block dies with its last view
        return np.frombuffer(block, dtype=dtype, count=nbytes // dtype.itemsize).reshape(shape)

    def drain(self):
        with self._lock:
            idle, self._idle, self._idle_bytes = self._idle, {}, 0
        for stack in idle.values():
            for address in stack:
                load_library().psa_host_free(C.c_void_p(address))


_pinned_pool = _PinnedPool()


def pinned_empty(shape, dtype) -> np.ndarray:
    """np.empty in page-locked memory (results of at least 1 MiB); an ordinary writable ndarray."""
    return _pinned_pool.empty(shape, dtype)


_SAMPLE_CACHE = {}


def _sample_positions(shape):
    """(flat positions, the same as per-axis index arrays) of the ~2k elements `_fingerprint` reads of an
    array of this shape; built once per shape."""
    hit = _SAMPLE_CACHE.get(shape)
    if hit is None:
        size = int(np.prod(shape, dtype=np.int64))
        lin = np.arange(0, size, max(1, size // 1021), dtype=np.int64)[:1021]
        if size > 2048:
            lin = np.concatenate([lin, np.sort(np.random.default_rng(size).integers(0, size, 1021)), [size - 1]])
        if len(_SAMPLE_CACHE) > 64:
            _SAMPLE_CACHE.clear()
        hit = _SAMPLE_CACHE[shape] = (lin, np.unravel_index(lin, shape))
    return hit


class Engine:
    """One HIP context (one GPU, one stream) with trajectory arrays resident in HBM."""

    def __init__(self, device: Optional[int] = None):
        self._lib = load_library()
        if device is None:
            device = int(os.environ.get("PSA_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            n = device_count()
            if n == 0:
                raise PsaHipError("no HIP device visible; psa_amd has no CPU fallback")
            device %= n
        h = _ctx()
        _check(self._lib.psa_create(int(device), C.byref(h)), "psa_create")
        self._h = h
        self.device = int(device)
        self._resident = {}          # slot -> (weakref to the array, data pointer, shape, fingerprint)
        self._converted = {}         # slot -> (weakref to a non-float32 source, fingerprint, float32 copy)
        # One calculation = upload + project (+ gather) + finalize on ONE context; callers that may
        # race (the reference GUI computes on worker threads) hold this around the sequence.
        self.lock = threading.RLock()
        self.rank, self.nranks = 0, 1
        self.result_serial = 0       # bumped by every call that replaces the result resident on the device
        self.segment_length = 0      # L of the Welch segments set on the context (set_segments); 0 = none

    # -- lifecycle -------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.psa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(self._lib.psa_synchronize(self._h), "psa_synchronize")

    def set_k1(self, selector: int):
        _check(self._lib.psa_set_k1(self._h, selector), "psa_set_k1")

    def set_lowrank_fold(self, on: bool):
        """The low-rank k-path route with the node table's lo piece folded into the D image (psa_set_k1_lowrank_fold; on in a
        new context).  False: the route as it was, bit for bit."""
        _check(self._lib.psa_set_k1_lowrank_fold(self._h, int(bool(on))), "psa_set_k1_lowrank_fold")

    def set_k1_lowrank_nodes(self, nodes: int):
        """Chebyshev nodes of the folded low-rank k-path route (psa_set_k1_lowrank_nodes): 48 (a new context) or 64.  With 48
        the folded D image also absorbs the interpolation residual and the node rows are 96.  Effective only while the fold
        is on; 64: the folded route as it was, bit for bit."""
        _check(self._lib.psa_set_k1_lowrank_nodes(self._h, int(nodes)), "psa_set_k1_lowrank_nodes")

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cu, mem = C.c_int(0), C.c_int64(0)
        _check(self._lib.psa_device_info(self._h, name, 256, C.byref(cu), C.byref(mem)),
               "psa_device_info")
        return {"name": name.value.decode(), "compute_units": cu.value, "hbm_bytes": mem.value}

    # -- trajectory residency --------------------------------------------------------
    @staticmethod
    def _fingerprint(a: np.ndarray) -> int:
        """Hash of ~2k elements spread over the array: catches in-place edits of a resident
        trajectory (scaling, overwriting, loading new frames into the same buffer) without
        reading it.  Not a proof of equality -- `invalidate()` is the explicit way."""
        if a.size == 0:
            return 0
        # a memory-mapped file (the reference's .npy cache, io/loader.py:48-79) is not sampled --
        # scattered reads of a file that may not sit in the page cache cost a disk seek each --
        # but identified by the file's name, size and modification time
        base = a
        while base is not None and not isinstance(base, np.memmap):
            base = getattr(base, "base", None)
        if base is not None and getattr(base, "filename", None):
            try:
                st = os.stat(base.filename)
                return hash((str(base.filename), st.st_size, st.st_mtime_ns, a.shape, a.strides))
            except OSError:
                pass
        # an even sweep plus scattered positions (an even stride alone can sit on one column of a
        # (T, N, 3) or (T, K, 3) array for ever); positions depend on the shape only and are kept
        lin, idx = _sample_positions(a.shape)
        if a.flags.c_contiguous:
            return hash(a.reshape(-1)[lin].tobytes())                # a gather: never copies the array
        return hash(a[idx].tobytes())

    def _as_device_layout(self, slot: int, array: np.ndarray) -> np.ndarray:
        """The array as C-contiguous float32.  A converted copy is kept (per slot) while the
        source object lives, so that float64 or strided trajectories are not re-converted and
        re-uploaded on every call."""
        if array.ndim != 3 or array.shape[2] != 3:
            raise ValueError("trajectory array must be (frames, atoms, 3)")
        if array.dtype == np.float32 and array.flags.c_contiguous:
            return array
        held = self._converted.get(slot)
        fp = self._fingerprint(array)
        if held is not None and held[0]() is array and held[1] == fp:
            return held[2]
        conv = np.ascontiguousarray(array, dtype=np.float32)
        try:
            self._converted[slot] = (weakref.ref(array), fp, conv)
        except TypeError:
            self._converted.pop(slot, None)
        return conv

    def is_resident(self, slot: int, array: np.ndarray) -> bool:
        """True if this very array (same object, same buffer, same sampled contents) is what the
        slot holds."""
        held = self._resident.get(slot)
        if held is None or held[0] is None:
            return False
        a = array if held[0]() is array else self._as_device_layout(slot, array)
        return (held[0]() is a and held[1:3] == (a.ctypes.data, a.shape) and held[3] == self._fingerprint(a))

    def _note_resident(self, slot: int, a: np.ndarray):
        # a weak reference, not id(): a freed array's id and buffer can be reused
        try:
            ref = weakref.ref(a)
        except TypeError:
            ref = None
        self._resident[slot] = (ref, a.ctypes.data, a.shape, self._fingerprint(a))

    def ensure_resident(self, slot: int, array: np.ndarray):
        """Upload a (T,N,3) array unless this very array is already in the slot."""
        if self.is_resident(slot, array):
            return
        a = self._as_device_layout(slot, array)
        T, N = a.shape[0], a.shape[1]
        _check(self._lib.psa_data_upload(self._h, slot, _f32(a), T, N), "psa_data_upload")
        self._note_resident(slot, a)

    def invalidate(self, slot: Optional[int] = None):
        """Forget what is resident (call after modifying a trajectory array in place)."""
        if slot is None:
            self._resident.clear()
            self._converted.clear()
        else:
            self._resident.pop(slot, None)
            self._converted.pop(slot, None)

    def alloc(self, slot: int, T: int, N: int):
        _check(self._lib.psa_data_alloc(self._h, slot, T, N), "psa_data_alloc")
        self._resident[slot] = (None, None, (T, N, 3), None)

    def fill_synthetic(self, slot: int, seed: int, amp, comp, ct, st, ca, sa, t_offset: int = 0):
        """ct / st hold the rows of the slot's own frames [t_offset, t_offset + T)."""
        amp = np.ascontiguousarray(amp, np.float32)
        comp = np.ascontiguousarray(comp, np.int32)
        tabs = [np.ascontiguousarray(x, np.float32) for x in (ct, st, ca, sa)]
        _check(self._lib.psa_data_fill_synthetic(
            self._h, slot, C.c_uint64(seed), int(t_offset), len(amp), _f32(amp), comp.ctypes.data_as(_i32p),
            *[_f32(t) for t in tabs]), "psa_data_fill_synthetic")

    def set_option(self, option: int, value: int):
        _check(self._lib.psa_set_option(self._h, option, int(value)), "psa_set_option")

    def reset_options(self):
        """Every option back to its default in the library's table (option_table).  The environment overrides that
        psa_create reads (PSA_K1_LOWRANK, PSA_K1_LOWRANK_MIN_K) are ignored: the table's values are set."""
        for option, _, default in option_table():
            self.set_option(option, default)
        self.set_lowrank_fold(True)                  # a switch of its own beside the table: back to a new context's state too

    def scratch_fill(self, byte: int):
        """(buffers, bytes) filled: every byte of the context's real scratch buffers set to `byte`, of its index buffers to
        0, and the context armed so that new allocations and plane sets come filled the same way (psa_debug_scratch_fill);
        byte = -1 disarms.  The result resident on the device is dropped.  A correct call after it returns what it returned
        before."""
        n, b = C.c_int64(0), C.c_int64(0)
        _check(self._lib.psa_debug_scratch_fill(self._h, int(byte), C.byref(n), C.byref(b)), "psa_debug_scratch_fill")
        return n.value, b.value

    def plane_cache(self):
        """(number of cached split-plane sets, their bytes)"""
        n, b = C.c_int64(0), C.c_int64(0)
        _check(self._lib.psa_debug_plane_cache(self._h, C.byref(n), C.byref(b)), "psa_debug_plane_cache")
        return n.value, b.value

    def download(self, slot: int, t0: int, nt: int) -> np.ndarray:
        T, N = self.shape(slot)
        out = np.empty((nt, N, 3), np.float32)
        _check(self._lib.psa_data_download(self._h, slot, _f32(out), t0, nt), "psa_data_download")
        return out

    def release(self, slot: int):
        _check(self._lib.psa_data_release(self._h, slot), "psa_data_release")
        self._resident.pop(slot, None)

    def shape(self, slot: int):
        T, N = C.c_int64(0), C.c_int64(0)
        _check(self._lib.psa_data_shape(self._h, slot, C.byref(T), C.byref(N)), "psa_data_shape")
        return T.value, N.value

    def mean_positions(self, slot: int) -> np.ndarray:
        _, N = self.shape(slot)
        out = np.empty((N, 3), np.float32)
        _check(self._lib.psa_mean_positions(self._h, slot, _f32(out)), "psa_mean_positions")
        return out

    # -- the hot path ----------------------------------------------------------------
    def set_atom_weights(self, weights: Optional[np.ndarray]):
        """Per-atom weights of every later projection on this context (psa_set_atom_weights): q = sum_a w_a d_a
        exp(i k.r_a).  None clears them.  The resident arrays and their split planes are not touched."""
        if weights is None:
            _check(self._lib.psa_set_atom_weights(self._h, None, 0), "psa_set_atom_weights")
            return
        w = np.ascontiguousarray(weights, np.float32)
        if w.ndim != 1 or w.size == 0:
            raise ValueError(f"atom weights must be a non-empty (N,) array, got shape {w.shape}")
        if not np.all(np.isfinite(w)):
            raise ValueError("atom weights must be finite")
        _check(self._lib.psa_set_atom_weights(self._h, _f32(w), w.shape[0]), "psa_set_atom_weights")

    def set_segments(self, segments):
        """Welch segments of every later intensity projection on this context (psa_set_segments): a
        `psa_amd.Segments`, or None to clear them.  While they are set, results are (L, K) float32."""
        if segments is None:
            _check(self._lib.psa_set_segments(self._h, 0, 0, None), "psa_set_segments")
            self.segment_length = 0
            return
        w = np.ascontiguousarray(segments.window_array(), np.float32)
        _check(self._lib.psa_set_segments(self._h, segments.length, segments.hop, _f32(w)), "psa_set_segments")
        self.segment_length = segments.length

    def project(self, slot, mean_pos_all, k_vectors, groups=None, flags=0,
                K_total=None, k_offset=0):
        mean = _as_f32(mean_pos_all, (3,))
        kv = _as_f32(k_vectors, (3,)) if len(k_vectors) else np.zeros((0, 3), np.float32)
        idx, off, G = pack_groups(groups)
        K_local = kv.shape[0]
        self.result_serial += 1
        _check(self._lib.psa_sed_project(
            self._h, slot, _f32(mean), _f32(kv), K_local,
            K_local if K_total is None else K_total, k_offset,
            idx.ctypes.data_as(_i32p) if idx is not None else None,
            off.ctypes.data_as(_i64p) if off is not None else None, G, flags),
            "psa_sed_project")

    def project_upload(self, slot, array, mean_pos_all, k_vectors, groups=None, flags=0):
        """`ensure_resident` + `project` for an array that is not in HBM yet, overlapped: frames are
        projected as their chunk lands (psa_sed_project_upload)."""
        a = self._as_device_layout(slot, array)
        mean = _as_f32(mean_pos_all, (3,))
        kv = _as_f32(k_vectors, (3,))
        idx, off, G = pack_groups(groups)
        self._resident.pop(slot, None)
        self.result_serial += 1
        _check(self._lib.psa_sed_project_upload(
            self._h, slot, _f32(a), a.shape[0], a.shape[1], _f32(mean), _f32(kv), kv.shape[0],
            idx.ctypes.data_as(_i32p) if idx is not None else None,
            off.ctypes.data_as(_i64p) if off is not None else None, G, flags), "psa_sed_project_upload")
        self._note_resident(slot, a)

    def finalize(self, T: int, K: int, intensity: bool, fetch: bool = True, with_intensity: bool = False):
        """(T,K) / (T,K,3) is what the caller expects: the library refuses (PSA_EINVAL) if the
        result resident on the device has another size.  with_intensity (complex results): returns
        (sed, sum_c |sed|^2) -- the (T,K) float32 intensity comes out of the same pass on the device."""
        if not fetch:
            _check(self._lib.psa_sed_finalize(self._h, None, 0, None, 0), "psa_sed_finalize")
            return (None, None) if with_intensity else None
        out = pinned_empty((T, K), np.float32) if intensity else pinned_empty((T, K, 3), np.complex64)
        inten = pinned_empty((T, K), np.float32) if with_intensity and not intensity else None
        _check(self._lib.psa_sed_finalize(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes,
                                          _f32(inten) if inten is not None else None,
                                          inten.nbytes if inten is not None else 0), "psa_sed_finalize")
        return (out, inten) if with_intensity else out

    def single_bin(self, slot, mean_pos_all, k_vector, idx, i_w: int, flags=0) -> np.ndarray:
        """S[i_w, k, :] of one k-vector and one atom group as (3,) complex64."""
        mean = _as_f32(mean_pos_all, (3,))
        kv = np.ascontiguousarray(k_vector, np.float32).reshape(3)
        ii = None if idx is None else np.ascontiguousarray(idx, np.int32)
        out = np.empty(3, np.complex64)
        _check(self._lib.psa_sed_single_bin(
            self._h, slot, _f32(mean), _f32(kv), ii.ctypes.data_as(_i32p) if ii is not None else None,
            0 if ii is None else len(ii), flags, int(i_w), out.ctypes.data_as(_f32p)), "psa_sed_single_bin")
        return out

    def calculate(self, slot, mean_pos_all, k_vectors, groups=None, flags=0, with_intensity: bool = False):
        """project + finalize in one library call (psa_sed_calculate): a complex result of a long
        k-list is produced block by block, each block's D2H copy overlapping the next projection.
        with_intensity (complex results): returns (sed, sum_c |sed|^2), the second array computed on the
        device in the pass that writes the first."""
        T, _ = self.shape(slot)
        T = self.segment_length or T                 # frequency bins of the result: L under set_segments
        mean = _as_f32(mean_pos_all, (3,))
        kv = _as_f32(k_vectors, (3,))
        idx, off, G = pack_groups(groups)
        K = kv.shape[0]
        intensity = bool(flags & F_INTENSITY)
        out = pinned_empty((T, K), np.float32) if intensity else pinned_empty((T, K, 3), np.complex64)
        inten = pinned_empty((T, K), np.float32) if with_intensity and not intensity else None
        self.result_serial += 1
        _check(self._lib.psa_sed_calculate(
            self._h, slot, _f32(mean), _f32(kv), K,
            idx.ctypes.data_as(_i32p) if idx is not None else None,
            off.ctypes.data_as(_i64p) if off is not None else None, G, flags,
            out.ctypes.data_as(C.c_void_p), out.nbytes,
            _f32(inten) if inten is not None else None, inten.nbytes if inten is not None else 0), "psa_sed_calculate")
        return (out, inten) if with_intensity else out

    def vdos(self, slot, mean_pos_all, groups=None, flags=0) -> np.ndarray:
        """Vibrational density of states of the resident array (psa_vdos): (L/2+1, G, 3) float32, the power spectrum
        of each atom's own series summed over the atoms of each group (disjoint index arrays; None: all atoms as one
        group), with the context's atom weights and segments (none set: L = T).  `mean_pos_all` is read only under
        F_DISPLACEMENTS.  The result of the SED entry points resident on the device is not touched."""
        T, N = self.shape(slot)
        L = self.segment_length or T
        mean = None if mean_pos_all is None else _as_f32(mean_pos_all, (3,))
        idx, off, G = pack_groups(groups)
        out = np.empty((G, 3, L // 2 + 1), np.float32)
        _check(self._lib.psa_vdos(
            self._h, slot, _f32(mean) if mean is not None else None,
            idx.ctypes.data_as(_i32p) if idx is not None else None,
            off.ctypes.data_as(_i64p) if off is not None else None, G, flags, _f32(out), out.nbytes), "psa_vdos")
        return np.ascontiguousarray(out.transpose(2, 0, 1))

    @staticmethod
    def _index_args(idx):
        """(index array int32 or None -- to be kept alive over the call --, its pointer, n) of an index array or None; an
        empty set keeps a valid pointer (one dummy element)"""
        if idx is None:
            return None, None, 0
        ii = np.ascontiguousarray(idx, np.int32).ravel()
        keep = ii if ii.size else np.zeros(1, np.int32)
        return keep, keep.ctypes.data_as(_i32p), int(ii.size)

    @staticmethod
    def _dynamic_args(k_vectors, idx):
        """(k-vectors (K, 3) float32, index array or None, its pointer, n_g)"""
        return (_as_f32(np.asarray(k_vectors, np.float32).reshape(-1, 3), (3,)),) + Engine._index_args(idx)

    def dynamic_spectra(self, k_vectors, idx=None, currents: bool = True) -> np.ndarray:
        """Dynamic spectra of the resident positions (and velocities) slots (psa_dynamic_spectra): (3, L, K) float32 --
        density, longitudinal, transverse -- or (1, L, K) with `currents=False`; the phase of every term is
        exp(i k.r_a(t)) with the position of that frame.  `idx`: one atom set (None: all atoms).  The context's atom
        weights and segments apply (none set: L = T).  The result of the SED entry points resident on the device is
        not touched."""
        T, _ = self.shape(SLOT_POSITIONS)
        L = self.segment_length or T
        kv, keep, ip, n_g = self._dynamic_args(k_vectors, idx)
        out = np.empty((3 if currents else 1, L, kv.shape[0]), np.float32)
        _check(self._lib.psa_dynamic_spectra(self._h, _f32(kv), kv.shape[0], ip, n_g, 1 if currents else 0, _f32(out), out.nbytes),
               "psa_dynamic_spectra")
        return out

    def debug_dynamic_project(self, k_vectors, idx=None, currents: bool = True) -> np.ndarray:
        """The kernel of `dynamic_spectra` alone: q (K, NC, T) complex64 before the window and the FFT, NC = 4 with
        currents (density, j_x, j_y, j_z), else 1."""
        T, _ = self.shape(SLOT_POSITIONS)
        kv, keep, ip, n_g = self._dynamic_args(k_vectors, idx)
        out = np.empty((kv.shape[0], 4 if currents else 1, T), np.complex64)
        _check(self._lib.psa_debug_dynamic_project(self._h, _f32(kv), kv.shape[0], ip, n_g, 1 if currents else 0,
                                                   out.ctypes.data_as(C.c_void_p)), "psa_debug_dynamic_project")
        return out

    def debug_dynamic_sincos(self, turns) -> np.ndarray:
        """(n, 2) float32: sine and cosine of 2 pi x as that kernel computes them, x in turns, |x| <= 2"""
        x = np.ascontiguousarray(turns, np.float32).ravel()
        out = np.empty((x.size, 2), np.float32)
        _check(self._lib.psa_debug_dynamic_sincos(self._h, _f32(x), x.size, _f32(out)), "psa_debug_dynamic_sincos")
        return out

    def _lattice_args(self, box_inverse, indices, idx=None, species=None):
        """The front half of a call on the box's lattice: (K, the leading arguments (handle, Hinv (3, 3) float64, indices
        (K, 3) int32, K), the atom arguments -- (pointer, n_g) of the index array `idx`, or (atoms, offsets, S) of
        `species` --, the arrays behind the pointers, to be kept alive over the call)"""
        inv = np.ascontiguousarray(box_inverse, np.float64)
        if inv.shape != (3, 3):
            raise ValueError(f"box_inverse must be (3, 3), got {inv.shape}")
        n = np.ascontiguousarray(np.asarray(indices, np.int32).reshape(-1, 3))
        if species is None:
            keep, *atoms = self._index_args(idx)
        else:
            flat, off, S = self._species_args(species)
            keep, atoms = (flat, off), (flat.ctypes.data_as(_i32p), off.ctypes.data_as(_i64p), S)
        return n.shape[0], (self._h, inv.ctypes.data_as(_f64p), n.ctypes.data_as(_i32p), n.shape[0]), tuple(atoms), (inv, n, keep)

    @staticmethod
    def _bins_args(bin_of, K):
        """(`bin_of` (K,) int32 or None -- the per-vector form --, its pointer)"""
        if bin_of is None:
            return None, None
        bins = np.ascontiguousarray(bin_of, np.int32).ravel()
        if bins.size != K:
            raise ValueError(f"bin_of has {bins.size} entries for {K} vectors")
        return bins, bins.ctypes.data_as(_i32p)

    def _lattice_call(self, entry, lead, rows, box_inverse, indices, bin_of, n_bins, *middle, idx=None, species=None):
        """One call of a spectra or correlations entry on the box's lattice: the arguments are the front half of
        `_lattice_args`, (`bin_of`, `n_bins`), the atom arguments, `middle`, (out, its bytes); out is `lead` (+ the pairs of `species`) + (rows, K -- with `bin_of`: n_bins) float32."""
        K, front, atoms, alive = self._lattice_args(box_inverse, indices, idx, species)
        bins, bp = self._bins_args(bin_of, K)
        if species is not None:
            lead += (atoms[2] * (atoms[2] + 1) // 2,)
        out = np.empty(lead + (rows, K if bins is None else int(n_bins)), np.float32)
        _check(getattr(self._lib, entry)(*front, bp, int(n_bins), *atoms, *middle, _f32(out), out.nbytes), entry)
        return out

    def lattice_spectra(self, box_inverse, indices, bin_of=None, n_bins=0, idx=None, currents: bool = True) -> np.ndarray:
        """Dynamic spectra on the box's reciprocal lattice (psa_lattice_spectra): k = n.G with integer `indices` (K, 3),
        `box_inverse` the float64 inverse of the box matrix (rows = box vectors).  `bin_of` None: per vector, (3, L, K)
        float32 -- density, longitudinal, transverse -- or (1, L, K) with `currents=False`.  `bin_of` (K,) with `n_bins`:
        the shell form, (3 or 1, L, n_bins), every vector a half-space member standing for itself and its partner -n.
        Atom set, weights and segments as for `dynamic_spectra`."""
        T, _ = self.shape(SLOT_POSITIONS)
        return self._lattice_call("psa_lattice_spectra", (3 if currents else 1,), self.segment_length or T, box_inverse, indices,
                                  bin_of, n_bins, 1 if currents else 0, idx=idx)

    def debug_lattice_project(self, box_inverse, indices, idx=None, currents: bool = True) -> np.ndarray:
        """The projection kernel of `lattice_spectra` alone: q (K, NC, T) complex64 before the window and the FFT, NC = 4
        with currents (density, j_x, j_y, j_z), else 1."""
        T, _ = self.shape(SLOT_POSITIONS)
        K, front, atoms, alive = self._lattice_args(box_inverse, indices, idx)
        out = np.empty((K, 4 if currents else 1, T), np.complex64)
        _check(self._lib.psa_debug_lattice_project(*front, *atoms, 1 if currents else 0, out.ctypes.data_as(C.c_void_p)),
               "psa_debug_lattice_project")
        return out

    def self_spectra(self, box_inverse, indices, bin_of=None, n_bins=0, idx=None) -> np.ndarray:
        """The self (incoherent) dynamic structure factor on the box's reciprocal lattice (psa_self_spectra): per atom
        z = w_a exp(2 pi i n.s_a(t)), its power summed over the atoms.  `bin_of` None: per vector, (L, K) float32;
        `bin_of` (K,) with `n_bins`: the shell form, (L, n_bins), every vector a half-space member standing for itself and
        its partner -n.  Arguments, atom set, weights and segments as for `lattice_spectra`; only positions are read."""
        T, _ = self.shape(SLOT_POSITIONS)
        return self._lattice_call("psa_self_spectra", (), self.segment_length or T, box_inverse, indices, bin_of, n_bins, idx=idx)

    def debug_self_series(self, box_inverse, indices, idx=None) -> np.ndarray:
        """The series kernel of `self_spectra` alone: z (n_g, K, T) complex64 before the window and the FFT, atoms in the
        order of the set, vectors in the caller's order."""
        T, N = self.shape(SLOT_POSITIONS)
        K, front, atoms, alive = self._lattice_args(box_inverse, indices, idx)
        out = np.empty((N if idx is None else atoms[1], K, T), np.complex64)
        _check(self._lib.psa_debug_self_series(*front, *atoms, out.ctypes.data_as(C.c_void_p)), "psa_debug_self_series")
        return out

    def debug_dynamic_power(self, segments, k_vectors, scale: float = 1.0, k_block: int = 0, seg_block: int = 0) -> np.ndarray:
        """The power pass of `dynamic_spectra` alone (psa_debug_dynamic_power): transformed segments (K, NC, ns, L)
        complex64 taken as they are, NC = 1 or 4 -> (1 or 3, L, K) float32; `k_block`, `seg_block` > 0: sub-blocks of at
        most that many vectors and segments, as a budget-bound call is cut."""
        S = np.ascontiguousarray(segments, np.complex64)
        kv = _as_f32(np.asarray(k_vectors, np.float32).reshape(-1, 3), (3,))
        if S.ndim != 4 or S.shape[0] != kv.shape[0] or S.shape[1] not in (1, 4):
            raise ValueError(f"segments {S.shape} and k_vectors {kv.shape} do not fit (K,1 or 4,ns,L) and (K,3)")
        K, NC, ns, L = S.shape
        out = np.empty((3 if NC == 4 else 1, L, K), np.float32)
        _check(self._lib.psa_debug_dynamic_power(self._h, S.ctypes.data_as(C.c_void_p), _f32(kv), K, 1 if NC == 4 else 0, ns, L,
                                                 int(k_block), int(seg_block), float(scale), _f32(out)), "psa_debug_dynamic_power")
        return out

    def debug_lattice_shell(self, segments, khat, bin_of, n_bins: int, norm: float, k_block: int = 0, seg_block: int = 0
                            ) -> np.ndarray:
        """The shell and finish passes of `lattice_spectra` alone (psa_debug_lattice_shell): transformed segments
        (K, NC, ns, L) complex64 of the vectors in processing order, `khat` (K, 3) float32, `bin_of` (K,) ascending ->
        (1 or 3, L, n_bins) float32 with the bins' scales 1 / (2 n_b norm)."""
        S = np.ascontiguousarray(segments, np.complex64)
        kh = _as_f32(np.asarray(khat, np.float32).reshape(-1, 3), (3,))
        bins = np.ascontiguousarray(bin_of, np.int32).ravel()
        if S.ndim != 4 or S.shape[0] != kh.shape[0] or S.shape[0] != bins.size or S.shape[1] not in (1, 4):
            raise ValueError(f"segments {S.shape}, khat {kh.shape} and bin_of {bins.shape} do not fit (K,1 or 4,ns,L), (K,3), (K,)")
        K, NC, ns, L = S.shape
        out = np.empty((3 if NC == 4 else 1, L, int(n_bins)), np.float32)
        _check(self._lib.psa_debug_lattice_shell(self._h, S.ctypes.data_as(C.c_void_p), _f32(kh), bins.ctypes.data_as(_i32p), K,
                                                 int(n_bins), 1 if NC == 4 else 0, ns, L, int(k_block), int(seg_block), float(norm),
                                                 _f32(out)), "psa_debug_lattice_shell")
        return out

    @staticmethod
    def _species_args(species):
        """(concatenated atom lists int32 -- one dummy entry where all are empty --, offsets (S + 1,) int64, S) of a
        sequence of atom lists; ValueError for none or more than PARTIAL_MAX_SPECIES"""
        lists = [np.ascontiguousarray(g, np.int32).ravel() for g in species]
        if not 1 <= len(lists) <= PARTIAL_MAX_SPECIES:
            raise ValueError(f"1 to {PARTIAL_MAX_SPECIES} species are served, got {len(lists)}")
        off = np.concatenate([[0], np.cumsum([g.size for g in lists])]).astype(np.int64)
        idx = np.concatenate(lists) if off[-1] else np.zeros(1, np.int32)
        return np.ascontiguousarray(idx, np.int32), off, len(lists)

    def partial_spectra(self, box_inverse, indices, species, bin_of=None, n_bins=0, currents: bool = True) -> np.ndarray:
        """Species-resolved dynamic spectra on the box's reciprocal lattice (psa_partial_spectra): `species` is a sequence
        of S <= 8 disjoint atom lists; one entry per pair a <= b in row-major upper-triangle order, P = S (S + 1) / 2.
        `bin_of` None: per vector, (3, P, L, K) float32 -- density, longitudinal, transverse: the real parts of
        F^a conj F^b -- or (1, P, L, K) with `currents=False`; `bin_of` (K,) with `n_bins`: the shell form,
        (3 or 1, P, L, n_bins).  Box, vectors, weights and segments as for `lattice_spectra`."""
        T, _ = self.shape(SLOT_POSITIONS)
        return self._lattice_call("psa_partial_spectra", (3 if currents else 1,), self.segment_length or T, box_inverse, indices,
                                  bin_of, n_bins, 1 if currents else 0, species=species)

    def debug_partial_project(self, box_inverse, indices, species, currents: bool = True) -> np.ndarray:
        """The projections of `partial_spectra` alone: q (K, S, NC, T) complex64 before the window and the FFT, NC = 4 with
        currents (density, j_x, j_y, j_z), else 1."""
        T, _ = self.shape(SLOT_POSITIONS)
        K, front, atoms, alive = self._lattice_args(box_inverse, indices, species=species)
        out = np.empty((K, atoms[2], 4 if currents else 1, T), np.complex64)
        _check(self._lib.psa_debug_partial_project(*front, *atoms, 1 if currents else 0, out.ctypes.data_as(C.c_void_p)),
               "psa_debug_partial_project")
        return out

    def debug_partial_power(self, segments, khat, norm: float, bin_of=None, n_bins: int = 0, k_block: int = 0,
                            seg_block: int = 0) -> np.ndarray:
        """The pair pass of `partial_spectra` alone (psa_debug_partial_power): transformed segments (K, S, NC, ns, L)
        complex64 taken as they are, `khat` (K, 3) float32.  `bin_of` None: per vector, (1 or 3, P, L, K) float32 with the
        scale float32(1 / norm); `bin_of` (K,) ascending: the shell and finish passes, (1 or 3, P, L, n_bins) with the
        bins' scales 1 / (2 n_b norm).  `k_block`, `seg_block` > 0: sub-blocks, as a budget-bound call is cut."""
        Z = np.ascontiguousarray(segments, np.complex64)
        kh = _as_f32(np.asarray(khat, np.float32).reshape(-1, 3), (3,))
        bins = None if bin_of is None else np.ascontiguousarray(bin_of, np.int32).ravel()
        if Z.ndim != 5 or Z.shape[0] != kh.shape[0] or Z.shape[2] not in (1, 4) or (bins is not None and bins.size != Z.shape[0]):
            raise ValueError(f"segments {Z.shape}, khat {kh.shape} and bin_of do not fit (K,S,1 or 4,ns,L), (K,3), (K,)")
        K, S, NC, ns, L = Z.shape
        if not 1 <= S <= PARTIAL_MAX_SPECIES:
            raise ValueError(f"1 to {PARTIAL_MAX_SPECIES} species are served, got {S}")
        out = np.empty((3 if NC == 4 else 1, S * (S + 1) // 2, L, K if bins is None else int(n_bins)), np.float32)
        _check(self._lib.psa_debug_partial_power(self._h, Z.ctypes.data_as(C.c_void_p), _f32(kh),
                                                 None if bins is None else bins.ctypes.data_as(_i32p), K, int(n_bins), S,
                                                 1 if NC == 4 else 0, ns, L, int(k_block), int(seg_block), float(norm), _f32(out)),
               "psa_debug_partial_power")
        return out

    def debug_self_power(self, work, groups, cols: int, scale, mirror: bool, n_chunks: int = 0, atom_block: int = 0,
                         vec_block: int = 0, seg_block: int = 0) -> np.ndarray:
        """The power, reduce and finish passes of `self_spectra` alone (psa_debug_self_power): transformed series
        (na, nv, ns, L) complex64, `groups` (n_groups + 1, 2) int32 = (first vector, column) with the last row (nv, 0),
        `scale` (cols,) float64 -> (L, cols) float32."""
        Z = np.ascontiguousarray(work, np.complex64)
        g = np.ascontiguousarray(groups, np.int32).reshape(-1, 2)
        sc = np.ascontiguousarray(scale, np.float64).ravel()
        if Z.ndim != 4 or g.shape[0] < 2 or sc.size != int(cols):
            raise ValueError(f"work {Z.shape}, groups {g.shape} and scale {sc.shape} do not fit (na,nv,ns,L), (n_groups+1,2), (cols,)")
        na, nv, ns, L = Z.shape
        out = np.empty((L, int(cols)), np.float32)
        _check(self._lib.psa_debug_self_power(self._h, Z.ctypes.data_as(C.c_void_p), na, nv, ns, L, g.ctypes.data_as(_i32p),
                                              g.shape[0] - 1, int(cols), sc.ctypes.data_as(_f64p), 1 if mirror else 0,
                                              int(n_chunks), int(atom_block), int(vec_block), int(seg_block), _f32(out)),
               "psa_debug_self_power")
        return out

    def lattice_correlations(self, box_inverse, indices, n_lags: int, bin_of=None, n_bins=0, idx=None, currents: bool = True
                             ) -> np.ndarray:
        """F(k,t), C_L(k,t), C_T(k,t) on the box's reciprocal lattice (psa_lattice_correlations): the linear, unbiased time
        correlation of every (boxcar) segment at lags 0 .. n_lags - 1.  (3, n_lags, K) float32, or (1, n_lags, K) with
        `currents=False`; with `bin_of` and `n_bins` the shell form, (3 or 1, n_lags, n_bins).  Everything else as for
        `lattice_spectra`."""
        return self._lattice_call("psa_lattice_correlations", (3 if currents else 1,), max(int(n_lags), 0), box_inverse, indices,
                                  bin_of, n_bins, 1 if currents else 0, int(n_lags), idx=idx)

    def self_correlations(self, box_inverse, indices, n_lags: int, bin_of=None, n_bins=0, idx=None) -> np.ndarray:
        """F_s(k,t) on the box's reciprocal lattice (psa_self_correlations): per atom the time correlation of
        z = w_a exp(2 pi i n.s_a(t)), summed over the atoms.  (n_lags, K) float32, or with `bin_of` and `n_bins` the shell
        form, (n_lags, n_bins).  Everything else as for `self_spectra`."""
        return self._lattice_call("psa_self_correlations", (), max(int(n_lags), 0), box_inverse, indices, bin_of, n_bins,
                                  int(n_lags), idx=idx)

    @staticmethod
    def _displacement_args(box, box_inverse, groups):
        """(H, Hinv (3, 3) float64, the groups' atoms concatenated or None, its pointer, the offsets or None, its pointer, G)"""
        H = np.ascontiguousarray(box, np.float64)
        if H.shape != (3, 3):
            raise ValueError(f"box must be (3, 3), got {H.shape}")
        if box_inverse is None:
            try:
                box_inverse = np.linalg.inv(H)
            except np.linalg.LinAlgError as e:
                raise ValueError(f"the box is singular: {e}") from None
        inv = np.ascontiguousarray(box_inverse, np.float64)
        if inv.shape != (3, 3):
            raise ValueError(f"box_inverse must be (3, 3), got {inv.shape}")
        if groups is None:
            return H, inv, None, None, None, None, 1
        lists = [np.asarray(g, np.int32).ravel() for g in groups]
        start = np.zeros(len(lists) + 1, np.int64)
        start[1:] = np.cumsum([g.size for g in lists])
        keep, ip, _ = Engine._index_args(np.concatenate(lists) if lists else np.zeros(0, np.int32))
        return H, inv, keep, ip, start, start.ctypes.data_as(_i64p), len(lists)

    def displacement_moments(self, box, n_lags: int, groups=None, origin_step: int = 1, unwrap: bool = True,
                             box_inverse=None) -> np.ndarray:
        """The moments of the displacement D = u[o + t] - u[o] over time origins and the atoms of each group
        (psa_displacement_moments): (n_lags, G, 4) float64 -- the means of D_x^2, D_y^2, D_z^2 and |D|^4.  `box` the
        (3, 3) box matrix, rows = box vectors (`box_inverse`: its inverse where the caller has one); `groups` None: all
        atoms as one group, else index arrays, disjoint, an empty one gives zeros; origins 0, origin_step, ...;
        `unwrap=False` takes the positions as unwrapped.  Only positions are read."""
        H, inv, keep, ip, start, sp, G = self._displacement_args(box, box_inverse, groups)
        out = np.empty((max(int(n_lags), 0), G, 4), np.float64)
        _check(self._lib.psa_displacement_moments(self._h, H.ctypes.data_as(_f64p), inv.ctypes.data_as(_f64p), ip, sp, G, int(n_lags),
                                                  int(origin_step), 1 if unwrap else 0, out.ctypes.data_as(_f64p), out.nbytes),
               "psa_displacement_moments")
        return out

    def van_hove_self(self, box, lags, dr: float, n_r: int, groups=None, origin_step: int = 1, unwrap: bool = True,
                      box_inverse=None) -> np.ndarray:
        """The self van Hove function as counts (psa_van_hove_self): (n_vh, G, n_r + 1) uint64, bin i = floor(|D| / dr) of
        the displacements over the lag `lags[j]`, the last entry the overflow count.  Everything else as for
        `displacement_moments`."""
        H, inv, keep, ip, start, sp, G = self._displacement_args(box, box_inverse, groups)
        tau = np.ascontiguousarray(lags, np.int64).ravel()
        held = tau if tau.size else np.zeros(1, np.int64)
        out = np.empty((tau.size, G, max(int(n_r), 0) + 1), np.uint64)
        _check(self._lib.psa_van_hove_self(self._h, H.ctypes.data_as(_f64p), inv.ctypes.data_as(_f64p), ip, sp, G,
                                           held.ctypes.data_as(_i64p), tau.size, int(origin_step), 1 if unwrap else 0, float(dr),
                                           int(n_r), out.ctypes.data_as(_u64p), out.nbytes), "psa_van_hove_self")
        return out

    def self_overlap(self, box, lags, cutoff: float, groups=None, origin_step: int = 1, unwrap: bool = True,
                     per_origin: bool = False, box_inverse=None):
        """The self-overlap per time origin and its moments over the origins (psa_self_overlap): (sums (n_lags, G, 2)
        uint64 -- S1 = sum_k Q and S2 = sum_k Q^2 of Q[j,g,k], the atoms of group g within `cutoff` of where they were
        `lags[j]` frames before, at the origin k origin_step --, and with `per_origin` Q itself, (n_lags, G, n_o_max)
        uint32, zero beyond a lag's origins, else None).  Everything else as for `van_hove_self`."""
        H, inv, keep, ip, start, sp, G = self._displacement_args(box, box_inverse, groups)
        tau = np.ascontiguousarray(lags, np.int64).ravel()
        held = tau if tau.size else np.zeros(1, np.int64)
        out = np.empty((tau.size, G, 2), np.uint64)
        table = None
        if per_origin:
            try:
                T = self.shape(SLOT_POSITIONS)[0]
            except PsaHipError:                                  # nothing resident: the call below says so
                T = 0
            n_o_max = (T - 1 - int(tau.min())) // max(int(origin_step), 1) + 1 if tau.size and T else 0
            table = np.empty((tau.size, G, max(n_o_max, 0)), np.uint32)
        _check(self._lib.psa_self_overlap(self._h, H.ctypes.data_as(_f64p), inv.ctypes.data_as(_f64p), ip, sp, G,
                                          held.ctypes.data_as(_i64p), tau.size, int(origin_step), 1 if unwrap else 0, float(cutoff),
                                          out.ctypes.data_as(_u64p), out.nbytes,
                                          None if table is None else table.ctypes.data_as(_u32p),
                                          0 if table is None else table.nbytes), "psa_self_overlap")
        return out, table

    def debug_unwrap(self, box, idx=None, unwrap: bool = True, images: bool = True, box_inverse=None):
        """The unwrap pass alone (psa_debug_unwrap): (u (T, n_g, 3) float64, image counts (T, n_g, 3) int32 or None)."""
        T, N = self.shape(SLOT_POSITIONS)
        H, inv, keep, ip, _, _, _ = self._displacement_args(box, box_inverse, None if idx is None else [idx])
        n_g = N if idx is None else int(np.asarray(idx).size)
        u = np.empty((T, n_g, 3), np.float64)
        img = np.empty((T, n_g, 3), np.int32) if images else None
        _check(self._lib.psa_debug_unwrap(self._h, H.ctypes.data_as(_f64p), inv.ctypes.data_as(_f64p), ip, n_g, 1 if unwrap else 0,
                                          u.ctypes.data_as(_f64p), None if img is None else img.ctypes.data_as(_i32p)),
               "psa_debug_unwrap")
        return u, img

    def pair_histogram(self, box, lags, dr: float, n_r: int, groups=None, origin_step: int = 1, box_inverse=None) -> np.ndarray:
        """The histogram of minimum-image pair distances (psa_pair_histogram): (n_lags, S, S, n_r + 1) uint64, entry
        [j, alpha, beta, i] the number of (a in alpha, b in beta, b != a, origin o) with floor(|mi(r_b(o + lags[j]) -
        r_a(o))| / dr) = i, the last entry the overflow (r_max = n_r dr and beyond).  Lag 0 is g(r), later lags the
        distinct van Hove function.  `box` the (3, 3) box matrix, rows = box vectors; `groups` None: all atoms as one
        species, else index arrays, disjoint; origins 0, origin_step, ...  r_max beyond `psa_amd.max_pair_radius(box)`
        is refused.  Only positions are read, as stored: nothing is unwrapped."""
        H, inv, keep, ip, start, sp, G = self._displacement_args(box, box_inverse, groups)
        tau = np.ascontiguousarray(lags, np.int64).ravel()
        held = tau if tau.size else np.zeros(1, np.int64)
        out = np.empty((tau.size, G, G, max(int(n_r), 0) + 1), np.uint64)
        _check(self._lib.psa_pair_histogram(self._h, H.ctypes.data_as(_f64p), inv.ctypes.data_as(_f64p), ip, sp, G,
                                            held.ctypes.data_as(_i64p), tau.size, int(origin_step), float(dr), int(n_r),
                                            out.ctypes.data_as(_u64p), out.nbytes), "psa_pair_histogram")
        return out

    def debug_pair_fractions(self, box, idx=None, box_inverse=None) -> np.ndarray:
        """The fraction pass of `pair_histogram` alone (psa_debug_pair_fractions): (T, n_g, 3) float32, the fractional
        coordinates of the atoms `idx` (None: all) folded into [-0.5, 0.5]."""
        T, N = self.shape(SLOT_POSITIONS)
        H, inv, keep, ip, _, _, _ = self._displacement_args(box, box_inverse, None if idx is None else [idx])
        n_g = N if idx is None else int(np.asarray(idx).size)
        out = np.empty((T, n_g, 3), np.float32)
        _check(self._lib.psa_debug_pair_fractions(self._h, inv.ctypes.data_as(_f64p), ip, n_g, _f32(out)),
               "psa_debug_pair_fractions")
        return out

    @staticmethod
    def debug_pair_plan(sizes, sym: bool, n_origins: int) -> dict:
        """The workgroup table `pair_histogram` builds for species of these sizes over a block of `n_origins` origins
        (psa_debug_pair_plan; host only): the most beta-tiles of an item, the origin slabs, the items, the most samples
        one item can count."""
        n = np.ascontiguousarray(sizes, np.int64).ravel()
        out = np.zeros(4, np.int64)
        _check(load_library().psa_debug_pair_plan(n.ctypes.data_as(_i64p), n.size, 1 if sym else 0, int(n_origins),
                                                  out.ctypes.data_as(_i64p)), "psa_debug_pair_plan")
        return dict(run=int(out[0]), slabs=int(out[1]), items=int(out[2]), most_samples=int(out[3]))

    @staticmethod
    def _cutoffs(r_cut, S: int) -> np.ndarray:
        """r_cut as the (S, S) float64 matrix of a call: a scalar is every entry"""
        rc = np.asarray(r_cut, np.float64)
        rc = np.full((S, S), float(rc)) if rc.ndim == 0 else np.ascontiguousarray(rc)
        if rc.shape != (S, S):
            raise ValueError(f"r_cut must be a scalar or ({S}, {S}), got {rc.shape}")
        return rc

    def _shell_args(self, box, box_inverse, groups, r_cut, origin_step=None, ls=None):
        """What a shell entry point starts from, by name: head (its leading arguments: handle, box, inverse, atom list, offsets, S,
        r_cut), G, n_a, n_o (with `origin_step`), orders as int32 and their pointer lp (with `ls`), alive (the arrays behind the
        pointers, held as long as the result is)"""
        T, N = self.shape(SLOT_POSITIONS)
        H, inv, keep, ip, start, sp, G = self._displacement_args(box, box_inverse, groups)
        rc = self._cutoffs(r_cut, G)
        orders = None if ls is None else np.ascontiguousarray(ls, np.int32).ravel()
        held = None if ls is None else orders if orders.size else np.zeros(1, np.int32)
        n_a = N if groups is None else int(start[-1])
        n_o = None if origin_step is None else (T - 1) // max(int(origin_step), 1) + 1 if T else 0
        head = (self._h, H.ctypes.data_as(_f64p), inv.ctypes.data_as(_f64p), ip, sp, G, rc.ctypes.data_as(_f64p))
        return SimpleNamespace(head=head, G=G, n_a=n_a, n_o=n_o, orders=orders, lp=None if ls is None else held.ctypes.data_as(_i32p),
                               alive=(H, inv, keep, start, rc, held))

    def angle_histogram(self, box, r_cut, n_theta: int, groups=None, origin_step: int = 1, box_inverse=None):
        """Bond angles and coordination as counts (psa_angle_histogram): (angles (S, P, n_theta + 1) uint64, coord (S, S,
        65) uint64, truncated (S,) uint64).  b is a neighbour of a when b != a and |mi(r_b - r_a)| < r_cut[alpha, beta]
        (`r_cut` a scalar or symmetric (S, S), 0: no bond); angles[alpha, p, i] counts the unordered neighbour pairs of
        the centres of species alpha, filed under the species pair p (upper triangle, row-major) in bin i of `n_theta`
        uniform bins of the angle at the centre, the last entry the undefined angles; coord[alpha, beta, n] the (centre,
        origin) with exactly n beta-neighbours; a centre with more than 64 neighbours is left out of both and counted in
        truncated[alpha].  `box`, `groups`, `origin_step` as for `pair_histogram`.  Only positions are read, as stored."""
        a = self._shell_args(box, box_inverse, groups, r_cut)
        P, n1 = a.G * (a.G + 1) // 2, max(int(n_theta), 0) + 1
        angles = np.empty((a.G, P, n1), np.uint64)
        coord = np.empty((a.G, a.G, ANGLE_MAX_NEIGHBOURS + 1), np.uint64)
        trunc = np.empty(a.G, np.uint64)
        _check(self._lib.psa_angle_histogram(*a.head, int(origin_step), int(n_theta), angles.ctypes.data_as(_u64p), angles.nbytes,
                                             coord.ctypes.data_as(_u64p), coord.nbytes, trunc.ctypes.data_as(_u64p)),
               "psa_angle_histogram")
        return angles, coord, trunc

    def debug_neighbour_lists(self, box, r_cut, frame: int, groups=None, box_inverse=None):
        """The neighbour pass of `angle_histogram` alone at one frame (psa_debug_neighbour_lists): (count (n_a,) int32 the
        true numbers of neighbours, list (n_a, 64) int32 the positions in the concatenated atom list of the first 64,
        ascending, padded with -1)."""
        a = self._shell_args(box, box_inverse, groups, r_cut)
        count = np.zeros(max(a.n_a, 1), np.int32)
        lst = np.full((max(a.n_a, 1), ANGLE_MAX_NEIGHBOURS), -1, np.int32)
        _check(self._lib.psa_debug_neighbour_lists(*a.head, int(frame), count.ctypes.data_as(_i32p), lst.ctypes.data_as(_i32p)),
               "psa_debug_neighbour_lists")
        return count[:a.n_a], lst[:a.n_a]

    def bond_order(self, box, r_cut, ls, n_q: int, groups=None, origin_step: int = 1, per_atom: bool = False, box_inverse=None):
        """The Steinhardt order parameters q_l as counts (psa_bond_order): (hist (S, n_l, n_q) uint64, truncated, isolated,
        undefined (S,) uint64, x, n).  The neighbours are those of `angle_histogram` (`r_cut` a scalar or symmetric (S, S), 0:
        no bond); hist[alpha, j, i] counts the (centre of species alpha, origin) whose q of order ls[j] lies in bin i of
        `n_q` uniform bins over [0, 1]; a centre with more than 64 neighbours, with none, or with a coincident neighbour is
        left out and counted in truncated, isolated or undefined.  `ls`: strictly ascending orders in [1, 12], at most 8.
        With `per_atom`: x (n_o, n_a, n_l) int64, q_l^2 = x / (n^2 2^24) exactly as binned, -1 where the centre is left out,
        and n (n_o, n_a) int32 the true neighbour counts, in list order; else None, None.  `box`, `groups`, `origin_step`
        as for `pair_histogram`.  Only positions are read, as stored."""
        a = self._shell_args(box, box_inverse, groups, r_cut, origin_step, ls)
        hist = np.empty((a.G, a.orders.size, max(int(n_q), 0)), np.uint64)
        trunc, iso, undef = (np.empty(a.G, np.uint64) for _ in range(3))
        x = pinned_empty((a.n_o, a.n_a, a.orders.size), np.int64) if per_atom else None       # (every cell is written by the call)
        n = pinned_empty((a.n_o, a.n_a), np.int32) if per_atom else None
        _check(self._lib.psa_bond_order(*a.head, int(origin_step), a.lp, a.orders.size, int(n_q), hist.ctypes.data_as(_u64p), hist.nbytes,
                                        trunc.ctypes.data_as(_u64p), iso.ctypes.data_as(_u64p), undef.ctypes.data_as(_u64p),
                                        None if x is None else x.ctypes.data_as(_i64p),
                                        None if n is None else n.ctypes.data_as(_i32p)), "psa_bond_order")
        return hist, trunc, iso, undef, x, n

    def local_order(self, box, r_cut, ls, n_q: int, n_w: int, w3j, groups=None, origin_step: int = 1, w_range: float = 0.2,
                    solid_l: int = 6, solid_threshold: float = 0.7, per_atom: bool = False, box_inverse=None):
        """The neighbour-averaged q-bar_l, the third-order invariants w_l, w-bar_l and the solid-like bonds as counts
        (psa_local_order): (hist (S, R) uint64, qbar2, w, wbar, connections, n).  The neighbours are those of `bond_order`;
        `ls`: at most 4 strictly ascending even orders in [2, 12]; `w3j` the 3j symbols of the orders, per order the dense
        (2 l + 1, 2 l + 1) block of (l l l; m1 m2 -m1-m2), concatenated (`psa_amd.wigner_3j_table`).  A species' row of `hist`
        holds qbar (n_l, n_q), w (n_l, n_w), wbar (n_l, n_w), connections (65), truncated, isolated, undefined, incomplete,
        w_outside, w_undefined, wbar_outside, wbar_undefined (n_l each): `psa_amd.local_order.split_row` takes it apart.  With
        `per_atom`: qbar2, w, wbar (n_o, n_a, n_l) float64 (NaN: left out or undefined), connections (n_o, n_a) int32 (-1: left
        out) and n (n_o, n_a) int32 the true neighbour counts, in list order; else None.  `box`, `groups`, `origin_step` as
        for `pair_histogram`.  Only positions are read, as stored."""
        a = self._shell_args(box, box_inverse, groups, r_cut, origin_step, ls)
        table = np.ascontiguousarray(w3j, np.float64).ravel()
        held_3j = table if table.size else np.zeros(1, np.float64)
        n_l = a.orders.size
        row = n_l * max(int(n_q), 0) + 2 * n_l * max(int(n_w), 0) + ANGLE_MAX_NEIGHBOURS + 1 + 4 + 4 * n_l
        hist = np.empty((a.G, row), np.uint64)
        vals = [pinned_empty((a.n_o, a.n_a, n_l), np.float64) if per_atom else None for _ in range(3)]     # (every cell is written by the call)
        xi, n = ((pinned_empty((a.n_o, a.n_a), np.int32) if per_atom else None) for _ in range(2))
        f64 = lambda a: None if a is None else a.ctypes.data_as(_f64p)                                 # noqa: E731
        i32 = lambda a: None if a is None else a.ctypes.data_as(_i32p)                                 # noqa: E731
        _check(self._lib.psa_local_order(*a.head, int(origin_step), a.lp, n_l, int(n_q), int(n_w), float(w_range), int(solid_l),
                                         float(solid_threshold), held_3j.ctypes.data_as(_f64p), table.size, hist.ctypes.data_as(_u64p),
                                         hist.nbytes, f64(vals[0]), f64(vals[1]), f64(vals[2]), i32(xi), i32(n)), "psa_local_order")
        return hist, vals[0], vals[1], vals[2], xi, n

    def solid_clusters(self, box, r_cut, solid_l: int = 6, solid_threshold: float = 0.7, min_connections: int = 7, link: int = 0,
                       n_sizes: int = 256, groups=None, origin_step: int = 1, per_atom: bool = False, box_inverse=None) -> dict:
        """The clusters of the solid atoms per time origin (psa_solid_clusters).  The neighbours, xi and the left-out rules
        are those of `local_order` with ls = (solid_l,), bit for bit; an atom is solid when xi >= `min_connections`; two
        solid atoms are joined when one lists the other (`link` 0) and, with `link` 1, that bond is solid-like; a cluster's
        label is the smallest column of its members, -1 and size 0 for an atom that is not solid.  Returns a dict:
        species_rows (S, 69) uint64 (connections[65], truncated, isolated, undefined, incomplete), size_counts (n_sizes + 2)
        uint64 (slot s: the clusters of exactly s atoms over all origins, the last the larger ones, slot 0 stays 0),
        large_atoms int, n_solid, n_clusters, largest, largest_label (n_o,) int32; with `per_atom` labels, size_atoms,
        connections, n (n_o, n_a) int32 and bond_masks (n_o, n_a) uint64 (bit b: the bond to the b-th neighbour of the list
        is solid-like), else None.  `box`, `groups`, `origin_step` as for `pair_histogram`.  Only positions are read."""
        a = self._shell_args(box, box_inverse, groups, r_cut, origin_step)
        rows = np.empty((a.G, CLUSTER_ROW_WORDS), np.uint64)
        counts = np.empty(min(max(int(n_sizes), 1), CLUSTER_MAX_SIZES) + 2, np.uint64)
        large = np.zeros(1, np.uint64)
        per_origin = [np.empty(max(a.n_o, 1), np.int32) for _ in range(4)]
        atoms = [pinned_empty((a.n_o, a.n_a), np.int32) if per_atom else None for _ in range(4)]    # (every cell is written by the call)
        masks = pinned_empty((a.n_o, a.n_a), np.uint64) if per_atom else None
        i32 = lambda x: None if x is None else x.ctypes.data_as(_i32p)                                 # noqa: E731
        _check(self._lib.psa_solid_clusters(*a.head, int(origin_step), int(solid_l), float(solid_threshold), int(min_connections),
                                            int(link), int(n_sizes), rows.ctypes.data_as(_u64p), counts.ctypes.data_as(_u64p),
                                            large.ctypes.data_as(_u64p), *(i32(x) for x in per_origin), *(i32(x) for x in atoms),
                                            None if masks is None else masks.ctypes.data_as(_u64p)), "psa_solid_clusters")
        return dict(species_rows=rows, size_counts=counts, large_atoms=int(large[0]), n_solid=per_origin[0][:a.n_o],
                    n_clusters=per_origin[1][:a.n_o], largest=per_origin[2][:a.n_o], largest_label=per_origin[3][:a.n_o], labels=atoms[0],
                    size_atoms=atoms[1], connections=atoms[2], n=atoms[3], bond_masks=masks)

    def bond_persistence(self, box, r_cut, lags, groups=None, step: int = 1, *, r_break=None, sample_step: int = 1,
                         continuous: bool = True, per_atom: bool = False, box_inverse=None) -> dict:
        """How long a neighbour stays a neighbour, as counts (psa_bond_persistence).  The pairs that `angle_histogram` lists
        at the origins 0, `step`, ... (`r_cut` a scalar or symmetric (S, S), 0: no bond) are tested again `lags[j]` frames
        later: a bond is alive while its distance stays below `r_break` (default: `r_cut`; >= `r_cut` entry by entry, 0
        exactly where it is).  `lags` strictly ascending in [0, T - 1], multiples of `sample_step`.  Returns a dict: bonds,
        alive, unbroken (n_lags, S, S) uint64 -- the bonds listed at the origins of lag j, those alive at o + lag, those
        alive at every frame o + sample_step, o + 2 sample_step, ... up to o + lag (zeros unless `continuous`) --, lost
        (n_lags, S, 65) uint64 the (centre, origin) by the number of listed neighbours that are not alive, truncated
        (n_lags, S) uint64 the centres with more than 64 neighbours, left out whole; with `per_atom` alive_masks and
        unbroken_masks (n_lags, n_o, n_a) uint64, bit i for the i-th neighbour of `debug_neighbour_lists`, else None.
        `box`, `groups` as for `pair_histogram`.  Only positions are read, as stored."""
        a = self._shell_args(box, box_inverse, groups, r_cut, step)
        rb = a.alive[4] if r_break is None else self._cutoffs(r_break, a.G)
        tau = np.ascontiguousarray(lags, np.int64).ravel()
        held = tau if tau.size else np.zeros(1, np.int64)
        pair = [np.empty((tau.size, a.G, a.G), np.uint64) for _ in range(3)]
        lost = np.empty((tau.size, a.G, ANGLE_MAX_NEIGHBOURS + 1), np.uint64)
        trunc = np.empty((tau.size, a.G), np.uint64)
        masks = [pinned_empty((tau.size, a.n_o, a.n_a), np.uint64) if per_atom else None for _ in range(2)]   # (the call zeroes them)
        u64 = lambda x: None if x is None else x.ctypes.data_as(_u64p)                                # noqa: E731
        _check(self._lib.psa_bond_persistence(*a.head, rb.ctypes.data_as(_f64p), int(step), held.ctypes.data_as(_i64p), tau.size,
                                              int(sample_step), 1 if continuous else 0, *(u64(x) for x in pair), pair[0].nbytes,
                                              u64(lost), lost.nbytes, u64(trunc), trunc.nbytes, u64(masks[0]), u64(masks[1]),
                                              masks[0].nbytes if per_atom else 0), "psa_bond_persistence")
        return dict(bonds=pair[0], alive=pair[1], unbroken=pair[2], lost=lost, truncated=trunc, alive_masks=masks[0],
                    unbroken_masks=masks[1])

    def common_neighbours(self, box, r_cut, groups=None, origin_step: int = 1, per_atom: bool = False, box_inverse=None) -> dict:
        """Common-neighbour analysis as counts (psa_common_neighbours).  The neighbours are those of `angle_histogram` (`r_cut`
        a scalar or symmetric (S, S), 0: no bond); two neighbours of a centre are bonded by the same float32 chain.  The
        bond a-b has the signature (j, k, l): its common neighbours, the bonds among them, the bonds of the largest connected
        piece of those.  Returns a dict: signature_counts (S, 8, 16, 16) uint64 per species of the centre, signature_outside
        (S,) uint64 the bonds beyond the table, type_counts (n_o, S, 5) uint64 the centres by type (`CNA_TYPES`: other, fcc,
        hcp, bcc, ico) at every origin, truncated (S,) uint64 the centres with more than 64 neighbours, left out whole; with
        `per_atom` types (n_o, n_a) int32 (-1: truncated), n (n_o, n_a) int32 the true neighbour counts and bond_signatures
        (n_o, n_a, 64) uint32, j | k << 8 | l << 16 for the i-th neighbour of `debug_neighbour_lists` (0xFFFFFFFF: no bond),
        else None.  `box`, `groups`, `origin_step` as for `pair_histogram`.  Only positions are read, as stored."""
        a = self._shell_args(box, box_inverse, groups, r_cut, origin_step)
        table = np.empty((a.G,) + CNA_TABLE, np.uint64)
        outside, trunc = (np.empty(a.G, np.uint64) for _ in range(2))
        census = np.empty((a.n_o, a.G, len(CNA_TYPES)), np.uint64)
        types, n = ((pinned_empty((a.n_o, a.n_a), np.int32) if per_atom else None) for _ in range(2))   # (every cell is written by the call)
        sigs = pinned_empty((a.n_o, a.n_a, ANGLE_MAX_NEIGHBOURS), np.uint32) if per_atom else None
        u64 = lambda x: x.ctypes.data_as(_u64p)                                                        # noqa: E731
        i32 = lambda x: None if x is None else x.ctypes.data_as(_i32p)                                 # noqa: E731
        _check(self._lib.psa_common_neighbours(*a.head, int(origin_step), u64(table), table.nbytes, u64(outside), u64(census), census.nbytes,
                                               u64(trunc), i32(types), i32(n), types.nbytes if per_atom else 0,
                                               None if sigs is None else sigs.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               sigs.nbytes if per_atom else 0), "psa_common_neighbours")
        return dict(signature_counts=table, signature_outside=outside, type_counts=census, truncated=trunc, types=types, n=n,
                    bond_signatures=sigs)

    def adaptive_common_neighbours(self, box, r_cut, groups=None, origin_step: int = 1, per_atom: bool = False, box_inverse=None) -> dict:
        """Adaptive common-neighbour analysis as counts (psa_adaptive_common_neighbours).  `r_cut` (a scalar or symmetric
        (S, S), 0: not a candidate) is a generous candidate radius: it must only contain the 14 nearest atoms.  The candidates
        are the neighbours of `angle_histogram`; a centre ranks them by distance, takes the cut-off (1 + sqrt 2) / 2 of the
        mean distance of its 12 nearest, and the signatures of `common_neighbours` among those 12 make it fcc, hcp or ico;
        otherwise, with 14 candidates or more, the 14 nearest with the cut-off of the bcc shells make it bcc or other.
        Returns a dict: signature_counts (S, 8, 16, 16), signature_outside (S,), type_counts (n_o, S, 5), truncated (S,) the
        centres with more than 64 candidates, left out whole, short (S,) those with fewer than 12 (other, no bonds), all
        uint64; with `per_atom` types (n_o, n_a) int32 (-1: truncated), n (n_o, n_a) int32 the true candidate counts, cutoffs
        (n_o, n_a) float32 the cut-off of the test that ran last (NaN: none ran), nearest (n_o, n_a, 14) int32 the members'
        columns of the atom list by rank (-1 beyond the last test's members) and bond_signatures (n_o, n_a, 14) uint32, j |
        k << 8 | l << 16 of the bond to that member (0xFFFFFFFF: no bond), else None.  `box`, `groups`, `origin_step` as for
        `pair_histogram`.  Only positions are read, as stored."""
        a = self._shell_args(box, box_inverse, groups, r_cut, origin_step)
        table = np.empty((a.G,) + CNA_TABLE, np.uint64)
        outside, trunc, short = (np.empty(a.G, np.uint64) for _ in range(3))
        census = np.empty((a.n_o, a.G, len(CNA_TYPES)), np.uint64)
        types, n = ((pinned_empty((a.n_o, a.n_a), np.int32) if per_atom else None) for _ in range(2))   # (every cell is written by the call)
        cuts = pinned_empty((a.n_o, a.n_a), np.float32) if per_atom else None
        near = pinned_empty((a.n_o, a.n_a, ACNA_MEMBERS), np.int32) if per_atom else None
        sigs = pinned_empty((a.n_o, a.n_a, ACNA_MEMBERS), np.uint32) if per_atom else None
        u64 = lambda x: x.ctypes.data_as(_u64p)                                                        # noqa: E731
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)                                  # noqa: E731
        _check(self._lib.psa_adaptive_common_neighbours(*a.head, int(origin_step), u64(table), table.nbytes, u64(outside), u64(census),
                                                        census.nbytes, u64(trunc), u64(short), ptr(types, _i32p), ptr(n, _i32p),
                                                        ptr(cuts, _f32p), types.nbytes if per_atom else 0, ptr(near, _i32p),
                                                        ptr(sigs, C.POINTER(C.c_uint32)), sigs.nbytes if per_atom else 0),
               "psa_adaptive_common_neighbours")
        return dict(signature_counts=table, signature_outside=outside, type_counts=census, truncated=trunc, short=short, types=types,
                    n=n, cutoffs=cuts, nearest=near, bond_signatures=sigs)

    def debug_cluster_labels(self, count, lists, solid, bond_masks=None, link: int = 0, n_sizes: int = 256) -> dict:
        """The graph passes of `solid_clusters` alone on a graph of the caller's (psa_debug_cluster_labels): `count` (n_o, n_a)
        in [0, 64], `lists` (n_o, n_a, 64) the neighbours' columns (-1 padding; only the first `count` are read), `solid`
        (n_o, n_a) bool, `bond_masks` (n_o, n_a) uint64 or None (all ones).  Lists that are not symmetric are legal: an edge
        that one end lists joins.  Returns the dict of `solid_clusters` without species_rows, connections, n, bond_masks."""
        cnt = np.ascontiguousarray(count, np.int32)
        if cnt.ndim != 2:
            raise ValueError(f"count must be (n_o, n_a), got {cnt.shape}")
        n_o, n_a = cnt.shape
        lst = np.ascontiguousarray(lists, np.int32)
        sol = np.ascontiguousarray(np.asarray(solid) != 0, np.uint8)
        if lst.shape != (n_o, n_a, ANGLE_MAX_NEIGHBOURS) or sol.shape != (n_o, n_a):
            raise ValueError(f"lists {lst.shape} and solid {sol.shape} do not fit count {cnt.shape} with {ANGLE_MAX_NEIGHBOURS} list positions")
        msk = None if bond_masks is None else np.ascontiguousarray(bond_masks, np.uint64)
        if msk is not None and msk.shape != (n_o, n_a):
            raise ValueError(f"bond_masks {msk.shape} does not fit count {cnt.shape}")
        counts = np.empty(min(max(int(n_sizes), 1), CLUSTER_MAX_SIZES) + 2, np.uint64)
        large = np.zeros(1, np.uint64)
        per_origin = [np.empty(max(n_o, 1), np.int32) for _ in range(4)]
        labels, sizes = (np.empty((n_o, n_a), np.int32) for _ in range(2))
        _check(self._lib.psa_debug_cluster_labels(self._h, n_o, n_a, cnt.ctypes.data_as(_i32p), lst.ctypes.data_as(_i32p),
                                                  sol.ctypes.data_as(C.POINTER(C.c_uint8)), None if msk is None else msk.ctypes.data_as(_u64p),
                                                  int(link), int(n_sizes), counts.ctypes.data_as(_u64p), large.ctypes.data_as(_u64p),
                                                  *(x.ctypes.data_as(_i32p) for x in per_origin), labels.ctypes.data_as(_i32p),
                                                  sizes.ctypes.data_as(_i32p)), "psa_debug_cluster_labels")
        return dict(size_counts=counts, large_atoms=int(large[0]), n_solid=per_origin[0][:n_o], n_clusters=per_origin[1][:n_o],
                    largest=per_origin[2][:n_o], largest_label=per_origin[3][:n_o], labels=labels, size_atoms=sizes)

    def debug_qlm(self, box, r_cut, frame: int, ls, groups=None, box_inverse=None) -> np.ndarray:
        """The first pass of `local_order` alone at one frame (psa_debug_qlm): Q (n_a, sum (l + 1), 2) int64, the vectors
        Q_lm = sum_b round(Yt_lm(d_b) 2^40), m = 0 .. l, (re, im), of every listed atom; a centre that is truncated, isolated
        or undefined has zeros and -1 in Im Q of its first column."""
        a = self._shell_args(box, box_inverse, groups, r_cut, ls=ls)
        cols = int((a.orders.astype(np.int64) + 1).sum())
        q = np.zeros((max(a.n_a, 1), max(cols, 1), 2), np.int64)
        _check(self._lib.psa_debug_qlm(*a.head, int(frame), a.lp, a.orders.size, q.ctypes.data_as(_i64p)), "psa_debug_qlm")
        return q[:a.n_a, :cols]

    def debug_correlation_transform(self, power, L: int, n_seg: int, n_lags: int, as_float32: bool = False) -> np.ndarray:
        """The back-transform of the time correlations alone (psa_debug_correlation_transform): `power` (fields, P, cols)
        float64 -- rounded to float32 first with `as_float32`, the per-vector pass's type -- ->
        (fields, n_lags, cols) float32 = 1 / (P n_seg (L - t)) sum_o power[f, o, col] cos(2 pi o t / P)."""
        X = np.ascontiguousarray(power, np.float64)
        if X.ndim != 3:
            raise ValueError(f"power {X.shape} does not fit (fields, P, cols)")
        fields, P, cols = X.shape
        out = np.empty((fields, max(int(n_lags), 0), cols), np.float32)
        _check(self._lib.psa_debug_correlation_transform(self._h, X.ctypes.data_as(_f64p), fields, P, cols, int(L),
                                                         int(n_seg), int(n_lags), 1 if as_float32 else 0, _f32(out)),
               "psa_debug_correlation_transform")
        return out

    def _modes_args(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, flags):
        """What the four mode entries are called with first (handle ... flags), K and M, and the arrays behind the
        pointers, which the caller holds until the call has returned"""
        mean = _as_f32(mean_pos_all, (3,))
        kv = _as_f32(k_vectors, (3,))
        idx, off, B = pack_groups(groups)
        eig = np.ascontiguousarray(eigenvectors, np.complex64)
        K = kv.shape[0]
        if eig.ndim != 4 or eig.shape[0] != K or eig.shape[2:] != (B, 3) or eig.shape[1] < 1:
            raise ValueError(f"eigenvectors have shape {eig.shape}, expected (K, M, B, 3) = ({K}, M, {B}, 3)")
        M = eig.shape[1]
        head = (self._h, slot, _f32(mean), _f32(kv), K,
                idx.ctypes.data_as(_i32p) if idx is not None else None,
                off.ctypes.data_as(_i64p) if off is not None else None, B,
                eig.ctypes.data_as(C.c_void_p), M, flags)
        return head, K, M, (mean, kv, idx, off, eig)

    def _sed_modes(self, entry, rows, slot, mean_pos_all, k_vectors, groups, eigenvectors, flags):
        """psa_sed_modes / psa_sed_modes_welch (`entry`) into a pinned (rows, K, M) float32 array"""
        head, K, M, _held = self._modes_args(slot, mean_pos_all, k_vectors, groups, eigenvectors, flags)
        out = pinned_empty((rows, K, M), np.float32)
        _check(getattr(self._lib, entry)(*head, _f32(out), out.nbytes), entry)
        return out

    def sed_modes(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, flags=0) -> np.ndarray:
        """Mode-projected SED of the resident array (psa_sed_modes): (T, K, M) float32 = |sum_{b,c} conj(eig) S_b|^2 for
        the B disjoint site groups (index arrays; None: all atoms as one group) and `eigenvectors` (K, M, B, 3)
        complex64, with the context's atom weights; the definition is in psa_amd/modes.py.  The result of the SED entry
        points resident on the device is not touched."""
        return self._sed_modes("psa_sed_modes", self.shape(slot)[0], slot, mean_pos_all, k_vectors, groups, eigenvectors, flags)

    def sed_modes_welch(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, flags=0) -> np.ndarray:
        """`sed_modes` averaged over the context's Welch segments (psa_sed_modes_welch; `set_segments`): (L, K, M)
        float32 = 1/(n_seg U) sum_s |sum_{b,c} conj(eig) F_b,s|^2.  With no segments set: one boxcar segment of all T
        frames, L = T."""
        return self._sed_modes("psa_sed_modes_welch", self.segment_length or self.shape(slot)[0], slot, mean_pos_all, k_vectors,
                               groups, eigenvectors, flags)

    def fit_peaks(self, spectrum, df, *, band=None, centers=None, search=None, window_hwhm=8.0, half_window=None,
                  max_iter=50):
        """Lorentzian fit of the peak of every column of `spectrum` (F, ...) float32 with frequency step `df` THz
        (psa_fit_peaks; definition in psa_amd/peaks.py): a `psa_amd.PeakFit` whose fields have the spectrum's column
        shape.  `band` = (fmin, fmax) THz for all columns (default: the positive half); `centers` (one frequency per
        column) with `search`: each column's own interval; `window_hwhm`: half width of the fit window in units of the
        peak's half width at half maximum, `half_window` THz overrides it; `max_iter`: the iteration cap."""
        from . import peaks
        spec, shape = peaks.spectrum_columns(spectrum)
        F, ncol = spec.shape
        peaks.check_fit_options(window_hwhm, max_iter)
        bands = peaks.peak_bands(F, df, ncol, band, centers, search)
        opts = PeakOpts(float(window_hwhm), peaks.half_window_bins(half_window, df), int(max_iter))
        fit, info = np.empty((ncol, 6), np.float32), np.empty((ncol, 4), np.int32)
        _check(self._lib.psa_fit_peaks(self._h, _f32(spec), F, ncol, float(df), bands.ctypes.data_as(_i32p), 0, 0,
                                       C.byref(opts), _f32(fit), info.ctypes.data_as(_i32p)), "psa_fit_peaks")
        return peaks.PeakFit.from_arrays(fit, info, shape)

    def _sed_modes_fit(self, entry, rows, slot, mean_pos_all, k_vectors, groups, eigenvectors, df, flags, return_sed, band,
                       centers, search, window_hwhm, half_window, max_iter):
        """psa_sed_modes_fit / psa_sed_modes_welch_fit (`entry`) of spectra with `rows` frequency bins"""
        from . import peaks
        head, K, M, _held = self._modes_args(slot, mean_pos_all, k_vectors, groups, eigenvectors, flags)
        peaks.check_fit_options(window_hwhm, max_iter)
        bands = peaks.peak_bands(rows, df, K * M, band, centers, search)
        opts = PeakOpts(float(window_hwhm), peaks.half_window_bins(half_window, df), int(max_iter))
        fit, info = np.empty((K * M, 6), np.float32), np.empty((K * M, 4), np.int32)
        out = pinned_empty((rows, K, M), np.float32) if return_sed else None
        _check(getattr(self._lib, entry)(
            *head, float(df), bands.ctypes.data_as(_i32p), 0, 0, C.byref(opts), _f32(fit), info.ctypes.data_as(_i32p),
            _f32(out) if out is not None else None, out.nbytes if out is not None else 0), entry)
        return peaks.PeakFit.from_arrays(fit, info, (K, M)), out

    def sed_modes_fit(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, df, flags=0, *, return_sed=False, band=None,
                      centers=None, search=None, window_hwhm=8.0, half_window=None, max_iter=50):
        """`sed_modes` and `fit_peaks` of its result in one library call (psa_sed_modes_fit): the (T, K, M) spectra are
        fitted where they lie and cross to the host only with `return_sed`.  Returns (PeakFit with (K, M) fields, the
        spectra or None)."""
        return self._sed_modes_fit("psa_sed_modes_fit", self.shape(slot)[0], slot, mean_pos_all, k_vectors, groups, eigenvectors,
                                   df, flags, return_sed, band, centers, search, window_hwhm, half_window, max_iter)

    def sed_modes_welch_fit(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, df, flags=0, *, return_sed=False,
                            band=None, centers=None, search=None, window_hwhm=8.0, half_window=None, max_iter=50):
        """`sed_modes_welch` and `fit_peaks` of its (L, K, M) result in one library call (psa_sed_modes_welch_fit); `df`
        is the step of the segment transform, 1 / (L dt).  Returns (PeakFit with (K, M) fields, the spectra or None)."""
        return self._sed_modes_fit("psa_sed_modes_welch_fit", self.segment_length or self.shape(slot)[0], slot, mean_pos_all,
                                   k_vectors, groups, eigenvectors, df, flags, return_sed, band, centers, search, window_hwhm,
                                   half_window, max_iter)

    def debug_mode_power(self, spectra: np.ndarray, eigenvectors: np.ndarray) -> np.ndarray:
        """The contraction kernel of `sed_modes` alone (psa_debug_mode_power): spectra (B, K, 3, T) complex64 taken as
        they are, eigenvectors (K, M, B, 3) complex64 -> (T, K, M) float32."""
        S = np.ascontiguousarray(spectra, np.complex64)
        eig = np.ascontiguousarray(eigenvectors, np.complex64)
        B, K, _, T = S.shape
        if S.shape[2] != 3 or eig.ndim != 4 or eig.shape[0] != K or eig.shape[2:] != (B, 3):
            raise ValueError(f"spectra {S.shape} and eigenvectors {eig.shape} do not fit (B,K,3,T) and (K,M,B,3)")
        M = eig.shape[1]
        out = np.empty((T, K, M), np.float32)
        _check(self._lib.psa_debug_mode_power(self._h, S.ctypes.data_as(C.c_void_p), eig.ctypes.data_as(C.c_void_p), B, K, M, T,
                                              _f32(out)), "psa_debug_mode_power")
        return out

    def debug_mode_power_welch(self, segments: np.ndarray, eigenvectors: np.ndarray, scale: float = 1.0, seg_block: int = 0
                               ) -> np.ndarray:
        """The contraction kernel of `sed_modes_welch` alone (psa_debug_mode_power_welch): transformed segments
        (B, K, 3, ns, L) complex64 taken as they are, eigenvectors (K, M, B, 3) complex64 -> (L, K, M) float32 =
        sum_s scale |sum conj(eig) S_s|^2; `seg_block` > 0: launches of at most that many segments."""
        S = np.ascontiguousarray(segments, np.complex64)
        eig = np.ascontiguousarray(eigenvectors, np.complex64)
        if S.ndim != 5 or S.shape[2] != 3 or eig.ndim != 4 or eig.shape[0] != S.shape[1] or eig.shape[2:] != (S.shape[0], 3):
            raise ValueError(f"segments {S.shape} and eigenvectors {eig.shape} do not fit (B,K,3,ns,L) and (K,M,B,3)")
        if int(seg_block) < 0:
            raise ValueError(f"seg_block = {seg_block} must not be negative")
        B, K, _, ns, L = S.shape
        M = eig.shape[1]
        out = np.empty((L, K, M), np.float32)
        _check(self._lib.psa_debug_mode_power_welch(self._h, S.ctypes.data_as(C.c_void_p), eig.ctypes.data_as(C.c_void_p), B, K, M,
                                                    L, ns, int(seg_block), float(scale), _f32(out)),
               "psa_debug_mode_power_welch")
        return out

    def sed_covariance(self, slot, mean_pos_all, k_vectors, groups, freq_weights, flags=0) -> np.ndarray:
        """Spectral covariance of the resident array (psa_sed_covariance): (n_w, K, n, n) complex128 =
        sum_w g_m[w] S_i[k,w] conj(S_j[k,w]) over the n = 3B rows i = 3b + c of the B disjoint site groups (index arrays;
        None: all atoms as one group), with the context's atom weights and `freq_weights` (n_w, T) float32, n_w 1 or 2;
        the definition is in psa_amd/covariance.py.  The result of the SED entry points resident on the device is not
        touched."""
        mean = _as_f32(mean_pos_all, (3,))
        kv = _as_f32(k_vectors, (3,))
        idx, off, B = pack_groups(groups)
        g = np.ascontiguousarray(freq_weights, np.float32)
        T = self.shape(slot)[0]
        if g.ndim != 2 or g.shape[1] != T:
            raise ValueError(f"freq_weights have shape {g.shape}, expected (n_w, T) = (n_w, {T})")
        K, n = kv.shape[0], 3 * B
        out = np.empty((g.shape[0], K, n, n), np.complex128)
        _check(self._lib.psa_sed_covariance(
            self._h, slot, _f32(mean), _f32(kv), K,
            idx.ctypes.data_as(_i32p) if idx is not None else None,
            off.ctypes.data_as(_i64p) if off is not None else None, B, _f32(g), g.shape[0], flags,
            out.ctypes.data_as(C.c_void_p), out.nbytes), "psa_sed_covariance")
        return out

    def debug_covariance(self, spectra: np.ndarray, freq_weights: np.ndarray, scale: float = 1.0) -> np.ndarray:
        """The covariance kernels of `sed_covariance` alone (psa_debug_covariance): spectra (B, K, 3, T) complex64 taken
        as they are, freq_weights (n_w, T) float32 -> (n_w, K, 3B, 3B) complex128 = scale sum_w g S S^+."""
        S = np.ascontiguousarray(spectra, np.complex64)
        g = np.ascontiguousarray(freq_weights, np.float32)
        if S.ndim != 4 or S.shape[2] != 3 or g.ndim != 2 or g.shape[1] != S.shape[3]:
            raise ValueError(f"spectra {S.shape} and freq_weights {g.shape} do not fit (B,K,3,T) and (n_w,T)")
        B, K, _, T = S.shape
        out = np.empty((g.shape[0], K, 3 * B, 3 * B), np.complex128)
        _check(self._lib.psa_debug_covariance(self._h, S.ctypes.data_as(C.c_void_p), B, K, T, _f32(g), g.shape[0], float(scale),
                                              out.ctypes.data_as(C.c_void_p)), "psa_debug_covariance")
        return out

    def set_kmap(self, kmap: np.ndarray):
        """Install the k map of a result whose slab rows were projected from a folded list (`k_pairs`)."""
        m = np.ascontiguousarray(kmap, np.uint32).view(np.int32)
        _check(self._lib.psa_sed_set_kmap(self._h, m.ctypes.data_as(_i32p), len(m)), "psa_sed_set_kmap")

    def slab_read(self, row0: int, nrows: int, T: int, intensity: bool) -> np.ndarray:
        out = np.empty((nrows, T), np.float32) if intensity else np.empty((nrows, 3, T), np.complex64)
        _check(self._lib.psa_slab_read(self._h, row0, nrows, out.ctypes.data_as(C.c_void_p)), "psa_slab_read")
        return out

    def slab_write(self, row0: int, rows: np.ndarray):
        rows = np.ascontiguousarray(rows)
        self.result_serial += 1
        _check(self._lib.psa_slab_write(self._h, row0, rows.shape[0], rows.ctypes.data_as(C.c_void_p)),
               "psa_slab_write")

    def intensity_source(self, array: np.ndarray):
        """A callable for `SED._device_intensity`: given the array now in `SED.sed`, the intensity of
        the complex result resident on the device -- or None if that is no longer this array's
        result (another calculation came in between, the array was replaced or edited)."""
        serial, ref, stamp = self.result_serial, weakref.ref(array), self._fingerprint(array)
        T, K = array.shape[0], array.shape[1]

        def source(current):
            if current is not ref() or self._h is None:
                return None
            with self.lock:
                if self.result_serial != serial or self._fingerprint(current) != stamp:
                    return None
                try:
                    return self.result_intensity(T, K)
                except PsaHipError:
                    return None
        return source

    def result_intensity(self, T: int, K: int) -> np.ndarray:
        out = pinned_empty((T, K), np.float32)
        _check(self._lib.psa_result_intensity(self._h, _f32(out), out.nbytes), "psa_result_intensity")
        return out

    def result_chiral_phase(self, T: int, K: int, c1: int, c2: int) -> np.ndarray:
        out = pinned_empty((T, K), np.float32)
        _check(self._lib.psa_result_chiral_phase(self._h, c1, c2, _f32(out), out.nbytes),
               "psa_result_chiral_phase")
        return out

    def timings(self) -> dict:
        ms = (C.c_double * 8)()
        _check(self._lib.psa_last_timings(self._h, ms), "psa_last_timings")
        return dict(zip(TIMING_NAMES, list(ms)))

    def oneoff_stats(self) -> dict:
        """Host wall clock (ms) of once-per-array / once-per-shape work since the last call."""
        ms = (C.c_double * 4)()
        _check(self._lib.psa_oneoff_stats(self._h, ms), "psa_oneoff_stats")
        return dict(zip(("rocfft_plan", "absmax", "split_planes", "upload"), list(ms)))

    def adopt(self, slot: int, array: np.ndarray):
        """Declare that the slot's device-generated contents (alloc + fill_synthetic) ARE `array` as
        far as residency goes: `calculate` on a Trajectory holding `array` then finds it resident.
        For benchmarks whose trajectory exists only in HBM (`array` can be a zero-stride stand-in)."""
        T, N = self.shape(slot)
        if tuple(array.shape) != (T, N, 3) or array.dtype != np.float32 or not array.flags.c_contiguous and array.strides != (0, 0, 0):
            raise ValueError("stand-in must be a float32 (T, N, 3) array of the slot's shape")
        self._note_resident(slot, array)

    def k1_stats(self):
        n, ms = C.c_int64(0), C.c_double(0.0)
        _check(self._lib.psa_k1_stats(self._h, C.byref(n), C.byref(ms)), "psa_k1_stats")
        return n.value, ms.value

    def lowrank_launches(self) -> int:
        """Projection launches so far that took the low-rank route for k-paths (PSA_OPT_K1_LOWRANK)."""
        n = C.c_int64(0)
        _check(self._lib.psa_k1_lowrank_launches(self._h, C.byref(n)), "psa_k1_lowrank_launches")
        return n.value

    def lowrank_pair_launches(self) -> int:
        """... of which the pair launch projected node rows and D rows in one kernel (PSA_OPT_K1_LOWRANK_PAIR)."""
        n = C.c_int64(0)
        _check(self._lib.psa_k1_lowrank_pair_launches(self._h, C.byref(n)), "psa_k1_lowrank_pair_launches")
        return n.value

    # -- diagnostics -----------------------------------------------------------------
    def debug_phase_table(self, mean_pos_all, k_vectors, idx=None) -> np.ndarray:
        mean = _as_f32(mean_pos_all, (3,))
        kv = _as_f32(k_vectors, (3,))
        N = mean.shape[0]
        ii = None if idx is None else np.ascontiguousarray(idx, np.int32)
        n_g = N if ii is None else len(ii)
        out = np.empty((kv.shape[0], n_g), np.complex64)
        _check(self._lib.psa_debug_phase_table(
            self._h, _f32(mean), _f32(kv), kv.shape[0],
            ii.ctypes.data_as(_i32p) if ii is not None else None, n_g, N,
            out.ctypes.data_as(C.c_void_p)), "psa_debug_phase_table")
        return out

    def debug_project_only(self, slot, mean_pos_all, k_vectors, idx=None, flags=0, frames=None, route=False) -> np.ndarray:
        """q before the FFT, (K,3,T); `frames=(t_begin, t_count)` projects only those frames (the
        other columns are zero).  It never takes the low-rank route for k-paths unless `route=True`: then the
        launch is routed as `project` routes a list of these k-vectors (all frames; psa_debug_project_route) and
        `lowrank_launches` counts it."""
        if route and frames is not None:
            raise ValueError("route=True projects all frames")
        T, N = self.shape(slot)
        mean = _as_f32(mean_pos_all, (3,))
        kv = _as_f32(k_vectors, (3,))
        ii = None if idx is None else np.ascontiguousarray(idx, np.int32)
        n_g = N if ii is None else len(ii)
        out = np.empty((kv.shape[0], 3, T), np.complex64)
        ip = ii.ctypes.data_as(_i32p) if ii is not None else None
        if route:
            _check(self._lib.psa_debug_project_route(
                self._h, slot, _f32(mean), _f32(kv), kv.shape[0], ip, n_g, flags,
                out.ctypes.data_as(C.c_void_p)), "psa_debug_project_route")
        elif frames is None:
            _check(self._lib.psa_debug_project_only(
                self._h, slot, _f32(mean), _f32(kv), kv.shape[0], ip, n_g, flags,
                out.ctypes.data_as(C.c_void_p)), "psa_debug_project_only")
        else:
            _check(self._lib.psa_debug_project_frames(
                self._h, slot, _f32(mean), _f32(kv), kv.shape[0], ip, n_g, flags, int(frames[0]), int(frames[1]),
                out.ctypes.data_as(C.c_void_p)), "psa_debug_project_frames")
        return out

    # -- k-point sharding ------------------------------------------------------------
    @staticmethod
    def new_unique_id() -> bytes:
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        _check(load_library().psa_comm_unique_id(buf), "psa_comm_unique_id")
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, nranks: int):
        buf = C.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        _check(self._lib.psa_comm_init(self._h, buf, rank, nranks), "psa_comm_init")
        self.rank, self.nranks = rank, nranks

    def comm_selftest(self):
        _check(self._lib.psa_comm_selftest(self._h), "psa_comm_selftest")

    def comm_destroy(self):
        _check(self._lib.psa_comm_destroy(self._h), "psa_comm_destroy")
        self.rank, self.nranks = 0, 1

    def gather(self, root: int, k_offsets, k_counts):
        o = np.ascontiguousarray(k_offsets, np.int64)
        n = np.ascontiguousarray(k_counts, np.int64)
        _check(self._lib.psa_sed_gather(self._h, root, o.ctypes.data_as(_i64p),
                                        n.ctypes.data_as(_i64p)), "psa_sed_gather")

    def barrier(self):
        _check(self._lib.psa_comm_barrier(self._h), "psa_comm_barrier")

    # -- frame sharding --------------------------------------------------------------
    def fs_project(self, slot, mean_pos_all, k_vectors, idx, flags, T_total: int, k_offset: int, k_count: int):
        """All K k-vectors on the slot's own frames for one atom group -> q_local on the device."""
        mean = _as_f32(mean_pos_all, (3,))
        kv = _as_f32(k_vectors, (3,))
        ii = None if idx is None else np.ascontiguousarray(idx, np.int32)
        self.result_serial += 1
        _check(self._lib.psa_sed_fs_project(
            self._h, slot, _f32(mean), _f32(kv), kv.shape[0], ii.ctypes.data_as(_i32p) if ii is not None else None,
            0 if ii is None else len(ii), flags, int(T_total), int(k_offset), int(k_count)), "psa_sed_fs_project")

    def fs_exchange(self, t_offsets, t_counts, k_offsets, k_counts):
        arrs = [np.ascontiguousarray(x, np.int64) for x in (t_offsets, t_counts, k_offsets, k_counts)]
        _check(self._lib.psa_sed_fs_exchange(self._h, *[a.ctypes.data_as(_i64p) for a in arrs]), "psa_sed_fs_exchange")

    def fs_read(self, k0: int, nk: int, T_local: int) -> np.ndarray:
        out = np.empty((nk, 3, T_local), np.complex64)
        _check(self._lib.psa_sed_fs_read(self._h, k0, nk, out.ctypes.data_as(C.c_void_p)), "psa_sed_fs_read")
        return out

    def fs_write(self, t0: int, block: np.ndarray):
        block = np.ascontiguousarray(block, np.complex64)
        _check(self._lib.psa_sed_fs_write(self._h, t0, block.shape[2], block.ctypes.data_as(C.c_void_p)),
               "psa_sed_fs_write")

    def fs_finish(self, first_group: bool):
        _check(self._lib.psa_sed_fs_finish(self._h, 1 if first_group else 0), "psa_sed_fs_finish")
