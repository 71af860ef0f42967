"""The cases of the index-width tests (tests/test_bigslot_host.py, tests/test_gpu_bigslot.py): one resident array so
large that a slot address (t N + a) 3 + c formed in 32 bits wraps, probed through a few hundred listed atoms whose whole
time series the host rebuilds from the generator's counter hash (psa_amd/synth.py: counter_noise).

The shape.  N = 2^20 + 3 atoms (odd: rows are not 16-byte aligned, N % 4 != 0), T = 2304 = 2^8 3^2 frames.  One slot is
29.0 GB; 3 T N = 7.25e9 > 2^32 and T N = 2.42e9 > 2^31.  The frames fall into four zones by the index of the first
element of their row, 3 t N:
    Z0  t < 683             nothing crossed
    Z1  683 <= t < 1366     the element index has passed 2^31 (an int wraps)
    Z2  1366 <= t < 2048    the element index has passed 2^32 (an unsigned wraps)
    Z3  t >= 2048           the atom-frame index t N + a has passed 2^31 as well
`zone_starts` derives the limits from N.  A wrap of the atom-frame index in an unsigned needs 51.5 GB per slot and is out
of scope.

The data are independent noise, roughly N(0, 1) within +-3.4, in every frame: nothing like a trajectory, which is what
makes every zone show in every result.  Consequences for the cases: positions are taken as unwrapped in the displacement
entry points (successive frames differ by more than half a box: no unwrapping is defined), and the boxes are sized to the
data (edge about 5).

`fault` is what the host test plants: the listed atoms' frames of one zone replaced by what a wrapped index would read."""
import functools

import numpy as np

from lattice_cases import CUBIC, TRICLINIC
from psa_amd import synth

N = (1 << 20) + 3
T = 2304
SEED_POSITIONS, SEED_VELOCITIES = 20231, 20232
SLOT_BYTES = T * N * 3 * 4

BOX_SCALE = 5.0 / 21.72
BOXES = {"cubic": (CUBIC * np.float32(BOX_SCALE)).astype(np.float32),
         "triclinic": (TRICLINIC * np.float32(BOX_SCALE)).astype(np.float32)}

ORIGIN_STEP = 293                      # origins 0, 293, ..., 2051: three in Z0, two in Z1, two in Z2, one in Z3
LAG_FAR = 2100                         # its one origin at this step is frame 0 (Z0), the partner frame 2100 (Z3)
FAULTS = {1: ("i32",), 2: ("u32", "i32"), 3: ("u32", "i32")}     # per zone: the kinds that change what is read there


# ---- the zones ------------------------------------------------------------------------------------------------------
def zone_starts(n_atoms=N):
    """(0, first frame of Z1, of Z2, of Z3): the first t with 3 t N >= 2^31, 3 t N >= 2^32, t N >= 2^31"""
    up = lambda a, b: -(-a // b)
    return 0, up(1 << 31, 3 * n_atoms), up(1 << 32, 3 * n_atoms), up(1 << 31, n_atoms)


def zone_frames(zone, n_atoms=N, n_frames=T):
    s = zone_starts(n_atoms) + (n_frames,)
    return np.arange(s[zone], s[zone + 1])


def zone_of(frames, n_atoms=N):
    return np.searchsorted(np.asarray(zone_starts(n_atoms)), np.asarray(frames), side="right") - 1


def edge_frames(n_atoms=N, n_frames=T):
    """the first and the last frame of every zone"""
    s = zone_starts(n_atoms)
    return [0, s[1] - 1, s[1], s[2] - 1, s[2], s[3] - 1, s[3], n_frames - 1]


# ---- the twin -------------------------------------------------------------------------------------------------------
def element_index(n_atoms, frames, atoms):
    """(len(frames), len(atoms), 3) uint64: (t N + a) 3 + c"""
    f, a = np.asarray(frames, np.uint64), np.asarray(atoms, np.uint64)
    return ((f[:, None] * np.uint64(n_atoms) + a[None, :]) * np.uint64(3))[:, :, None] + np.arange(3, dtype=np.uint64)


def synthetic_atoms(seed, n_atoms, frames, atoms):
    """(len(frames), len(atoms), 3) float32: the twin of fill_synthetic_kernel with no planted modes, for chosen atoms
    and frames of a (., n_atoms, 3) array"""
    return synth.counter_noise(seed, element_index(n_atoms, frames, atoms))


def fault(data, zone, kind, seed, atoms, n_atoms=N):
    """data (T, len(atoms), 3), the compact series of `atoms` over all frames, with the frames of `zone` replaced by what
    an index wrapped modulo 2^32 (kind "u32") or 2^31 ("i32", standing in for any other in-bounds data) would read"""
    out = np.array(data, np.float32)
    frames = zone_frames(zone, n_atoms, out.shape[0])
    i = element_index(n_atoms, frames, atoms) % np.uint64(1 << {"u32": 32, "i32": 31}[kind])
    out[frames] = synth.counter_noise(seed, i)
    return out


@functools.lru_cache(maxsize=None)
def _compact(seed, atoms):
    out = synthetic_atoms(seed, N, np.arange(T), np.asarray(atoms, np.int64))
    out.setflags(write=False)
    return out


def compact(seed, atoms):
    """(T, len(atoms), 3) float32 of the listed atoms over all frames, computed once per list and left unchanged"""
    return _compact(int(seed), tuple(int(a) for a in atoms))


# ---- the atom lists -------------------------------------------------------------------------------------------------
def atom_list(n, seed, n_atoms=N):
    """n distinct atoms, unsorted: atom 0, the last ten, the rest drawn over the whole range"""
    rng = np.random.default_rng(seed)
    ends = np.concatenate([[0], np.arange(n_atoms - 10, n_atoms)])
    rest = rng.choice(np.arange(1, n_atoms - 10), n - ends.size, replace=False)
    out = np.concatenate([ends, rest])
    rng.shuffle(out)
    return out.astype(np.int32)


def species(atoms, parts):
    """the list cut into `parts` disjoint species of unequal sizes, in list order"""
    n = len(atoms)
    cuts = {2: [n * 2 // 5], 3: [n // 4, n * 5 // 8]}[parts]
    return [np.ascontiguousarray(g) for g in np.split(np.asarray(atoms), cuts)]


def with_duplicate(atoms):
    """the list with its fourth member once more at the end (for the entry points whose lists may repeat atoms)"""
    return np.concatenate([atoms, atoms[3:4]]).astype(np.int32)


def compact_groups(groups):
    """the same groups as positions in the compact array of their concatenation"""
    starts = np.cumsum([0] + [len(g) for g in groups])
    return [np.arange(starts[i], starts[i + 1]) for i in range(len(groups))]


def listed_weights(atoms, seed, n_atoms=N):
    """(weights (n_atoms,) float32 that are 1 but for distinct values in [0.5, 1.5] at the listed atoms, the listed ones)"""
    w = np.ones(n_atoms, np.float32)
    a = np.unique(atoms)
    w[a] = (0.5 + np.random.default_rng(seed).permutation(a.size) / a.size).astype(np.float32)
    return w, w[np.asarray(atoms)]


# ---- the cases ------------------------------------------------------------------------------------------------------
MSD = dict(atoms=atom_list(120, 1), parts=2, step=ORIGIN_STEP, n_lags=T, vh_lags=(0, 1, LAG_FAR), dr=0.1, n_r=64)
PAIR = dict(atoms=atom_list(150, 2), step=ORIGIN_STEP, lags=(0, LAG_FAR), dr=0.03, n_r=64,
            layouts=(("cubic", 2), ("triclinic", 3)))
VDOS = dict(atoms=atom_list(200, 3), parts=3)
DYNAMIC = dict(atoms=atom_list(300, 4), K=5)
MEAN = dict(atoms=atom_list(100, 5))


def z3_window(n_frames=T, n_atoms=N):
    """(T,) float32: a Hann window over the last 256 frames, zero before them -- one segment of all frames that reads
    Z3 alone"""
    w = np.zeros(n_frames, np.float32)
    assert n_frames - 256 >= zone_starts(n_atoms)[3]
    w[n_frames - 256:] = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(256) / 256)).astype(np.float32)
    return w


def segment_layouts():
    """name -> psa_amd.Segments or None: all frames as one segment, one segment windowed onto Z3, Hann segments of 256
    frames at a hop of 128 over all zones"""
    from psa_amd import Segments
    return {"whole": None, "z3": Segments(T, T, z3_window()), "spanning": Segments(256, 128, "hann")}


def layout_args(layout):
    """(window, L, H) of a layout for the float64 references"""
    if layout is None:
        return None, None, None
    return layout.window_array(), layout.length, layout.hop


def mean32(data):
    """the sequential float32 mean over frames that psa_mean_positions promises: frame after frame into one float32
    accumulator, one division by T"""
    acc = np.zeros(data.shape[1:], np.float32)
    for frame in np.asarray(data, np.float32):
        acc = acc + frame
    return acc / np.float32(data.shape[0])


# ---- the references and their allowances, from a compact array -------------------------------------------------------
# Each returns what the GPU test compares with and the allowance it applies: the entry's own, from its *_cases.py.  The
# host test evaluates them on the clean and on the faulted compact array.
def msd_reference(data, case=MSD):
    """(moments64, its bar, counts64, what a count may differ by, borderline samples, all samples) with the positions
    taken as unwrapped"""
    import msd64
    import msd_cases
    groups = compact_groups(species(case["atoms"], case["parts"]))
    u, _, S = msd64.unwrap64(data, BOXES["cubic"], unwrap=False)
    ref = msd64.moments64(u, groups, case["n_lags"], case["step"])
    bar = msd_cases.moments_bar(u, S, groups, case["n_lags"], case["step"])
    counts = msd64.counts64(u, groups, case["vh_lags"], case["step"], case["dr"], case["n_r"])
    allowed, borderline, total = msd_cases.histogram_allowance(u, S, groups, case["vh_lags"], case["step"], case["dr"], case["n_r"])
    return ref, bar, counts, allowed, borderline, total


def pair_reference(data, box, parts, case=PAIR):
    """(counts, allowed, borderline samples, all samples) of pair_cases.reference"""
    import pair_cases
    groups = compact_groups(species(case["atoms"], parts))
    return pair_cases.reference(data, BOXES[box], groups, list(case["lags"]), case["step"], case["dr"], case["n_r"])


def vdos_reference(data, layout, weights, case=VDOS):
    """(vdos64 (F, G, 3), its bound) of the compact velocities with the listed atoms' weights"""
    import vdos64
    import vdos_cases
    groups = compact_groups(species(case["atoms"], case["parts"]))
    window, L, H = layout_args(layout)
    ref = vdos64.vdos64(data, groups, window=window, L=L, H=H, weights=weights)
    L = data.shape[0] if L is None else L
    H = L if H is None else H
    rows = vdos_cases.group_rows(data.shape[1], groups, vdos64.segment_count(data.shape[0], L, H))
    return ref, vdos_cases.bound(ref, L, rows)


def dynamic_k(case=DYNAMIC):
    """K k-vectors of dynamic_cases.k_list without its k = 0: the density's (sum_a w_a)^2 at zero frequency there would
    set the scale of rel_max, and a fault in the positions would hide behind it"""
    import dynamic_cases
    return np.delete(dynamic_cases.k_list(case["K"] + 1, seed=9), 1, axis=0)


def dynamic_reference(pos, vel, weights, case=DYNAMIC):
    """(project64 (K, 4, T), its per-element bound (4, T)) of the compact arrays"""
    import dynamic64
    import dynamic_cases
    ref, absum = dynamic64.project64(pos, vel, dynamic_k(case), None, weights, True, with_abs=True)
    return ref, dynamic_cases.bound(absum, pos.shape[1])


DYNAMIC_SPECTRA_BAR = 1e-5             # rel_max of tests/test_gpu_dynamic.py::test_index_list_small_budget_and_empty_set


def dynamic_spectra_reference(pos, vel, weights, layout, case=DYNAMIC):
    """(density, longitudinal, transverse), each (L, K) float64"""
    import dynamic64
    window, L, H = layout_args(layout)
    return dynamic64.dynamic_spectra64(pos, vel, dynamic_k(case), None, weights, True, window, L, H)


# ---- the spectra on the box's reciprocal lattice ----------------------------------------------------------------------
SPECTRA_BAR = 1e-5                     # rel_max of the lattice, partial and self spectra's own GPU tests against float64
LATTICE = dict(atoms=atom_list(300, 6), parts=3, box="triclinic",
               indices=np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -1, 2], [2, 1, 1]], np.int32))
SELF = dict(atoms=atom_list(100, 7), box="triclinic", indices=LATTICE["indices"][:4])


def box_inverse(case):
    import lattice_cases
    return lattice_cases.inverse(BOXES[case["box"]])


def lattice_reference(pos, vel, weights, case=LATTICE):
    """(lattice64.project64 (K, 4, T), its per-element bound (4, T)) of the compact arrays"""
    import lattice64
    import lattice_cases
    ref, absum = lattice64.project64(pos, vel, case["indices"], box_inverse(case), None, weights, True, with_abs=True)
    return ref, lattice_cases.bound(absum, pos.shape[1])


def lattice_spectra_reference(q, layout, case=LATTICE):
    """(density, longitudinal, transverse), each (L, K) float64, of the projections q (K, 4, T)"""
    import lattice64
    return lattice64.spectra64(q, case["indices"], box_inverse(case), *layout_args(layout))


def partial_spectra_reference(pos, vel, weights, layout, case=LATTICE):
    """(density, longitudinal, transverse), each (P, L, K) float64, of the list's three species"""
    import partial64
    groups = compact_groups(species(case["atoms"], case["parts"]))
    q = partial64.project64(pos, vel, case["indices"], box_inverse(case), groups, weights, True)
    return partial64.spectra64(q, case["indices"], box_inverse(case), *layout_args(layout))


def pair_errors(got, ref):
    """the metric tests/test_gpu_partial.py holds below SPECTRA_BAR"""
    from test_gpu_partial import _pair_errors
    return _pair_errors(got, ref)


def self_reference(pos, weights, case=SELF):
    """(self64.series64 (n_g, K, T), the per-atom bound (n_g, 1, 1))"""
    import self64
    import self_cases
    ref = self64.series64(pos, case["indices"], box_inverse(case), None, weights)
    return ref, self_cases.bound(np.asarray(weights, np.float64))[:, None, None]


def self_spectra_reference(pos, weights, layout, case=SELF):
    """(L, K) float64"""
    import self64
    return self64.density64(pos, case["indices"], box_inverse(case), None, weights, *layout_args(layout))


def column_rel_max(got, ref):
    """the largest rel_max over the columns (vectors), as tests/test_gpu_self.py takes it"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.max(np.abs(got - ref), axis=0) / np.max(np.abs(ref), axis=0)))


# ---- the SED projection on an index-list group ------------------------------------------------------------------------
SED = dict(atoms=with_duplicate(atom_list(333, 10)), parts=2, K=40, bins=(0, 1, 1152, 2303),
           # (form of tests/dense_cases.py, k-vectors, planes built): the gather kernels on the fly, then the list's split planes
           forms=(("pair", 40, False), ("bf16x3", 16, False), ("mfma32", 40, False), ("wave", 40, False),
                  ("planes128", 40, True), ("planes32", 16, True)))
E2E_TOL, E2E_TOL_ROW = 2e-6, 4e-6      # tests/test_gpu_dense_envelope.py::test_calculate_incoherent_two_groups: 2 TOL, 2 TOL_ROW


def sed_inputs(case=SED):
    """(mean positions of all N atoms (N, 3) float32 -- zero but for the listed rows --, the listed rows in list order,
    k (K, 3) float32)"""
    import dense_cases
    atoms = np.asarray(case["atoms"])
    members = np.unique(atoms)
    r_all = np.zeros((N, 3), np.float32)
    r_all[members] = dense_cases.positions(members.size, 17)
    return r_all, r_all[atoms], dense_cases.k_list(case["K"])


def sed_reference(vel, r_listed, k, weights):
    """(ref64.project64 (K, 3, T) of the compact velocities -- a repeated atom counts twice --, the scale B (3, T))"""
    import ref64
    return ref64.project64(vel, r_listed, k, None, weights, False), ref64.scale_B(vel, r_listed, None, weights, False)


# ---- F(k, t), F_s(k, t) and the current correlations: boxcar segments of 256 frames at a hop of 128 over all zones -----
CORRELATION = dict(L=256, H=128, n_lags=64)


def correlation_layout():
    from psa_amd import Segments
    return Segments(CORRELATION["L"], CORRELATION["H"], "boxcar")


def lattice_correlations_reference(q, case=LATTICE):
    """(density, longitudinal, transverse), each (n_lags, K) float64, of the projections q (K, 4, T)"""
    import correlation64
    c = CORRELATION
    return correlation64.fields64(q, case["indices"], box_inverse(case), c["L"], c["H"], c["n_lags"])


def self_correlations_reference(pos, weights, case=SELF):
    """(n_lags, K) float64"""
    import correlation64
    c = CORRELATION
    return correlation64.self_correlations64(pos, case["indices"], box_inverse(case), None, weights, c["L"], c["H"], c["n_lags"])


def correlation_fraction(got, ref):
    """largest error as a fraction of correlation_cases' end-to-end bar PARITY F(0) L / (L - t)"""
    import correlation_cases
    return correlation_cases.worst_fraction(got, ref, CORRELATION["L"])


# ---- the neighbour-shell passes (angle, order, local order, clusters): one fraction pass reads the slot for all of them ----
ANGLE = dict(atoms=atom_list(150, 11), parts=2, box="triclinic", r_cut=0.8, n_theta=45, step=ORIGIN_STEP)


def angle_reference(data, case=ANGLE, frames=None):
    """angle_cases.reference of the compact positions at the case's origins, or (frames given) at those frames alone"""
    import angle_cases
    groups = compact_groups(species(case["atoms"], case["parts"]))
    if frames is not None:
        return angle_cases.reference(data[np.asarray(frames)], BOXES[case["box"]], groups, case["r_cut"], 1, case["n_theta"])
    return angle_cases.reference(data, BOXES[case["box"]], groups, case["r_cut"], case["step"], case["n_theta"])


# ---- the mode-projected SED, its Welch average and the spectral covariance: disjoint site groups ------------------------
MODES = dict(atoms=atom_list(120, 12), parts=3, K=6, M=4, dt_ps=0.002)
MODES_BAR = 1e-5                       # rel_max of tests/test_gpu_modes.py, test_gpu_modes_welch.py, test_gpu_covariance.py


def modes_inputs(case=MODES):
    """(mean positions of all N atoms, the listed rows, k (K, 3), mode vectors (K, M, B, 3) complex64, frequency weights
    (2, T) float32 of the moments -2 and 0)"""
    import modes64
    from psa_amd import spectral_weights
    r_all, r, k = sed_inputs(case)
    eig = modes64.random_unitary(np.random.default_rng(13), case["K"], case["parts"], case["M"])
    g = np.stack([spectral_weights(T, case["dt_ps"], m) for m in (-2, 0)])
    return r_all, r, k, eig, g


def modes_references(vel, weights, layout, case=MODES):
    """(mode_sed64 (T, K, M), mode_welch64 (L, K, M) under `layout`, covariance64 (2, K, 3 B, 3 B)) of the compact velocities"""
    import cov64
    import modes64
    import modes_welch64
    _, r, k, eig, g = modes_inputs(case)
    groups = compact_groups(species(case["atoms"], case["parts"]))
    return (modes64.mode_sed64(vel, r, k, groups, eig, weights), modes_welch64.mode_welch64(vel, r, k, groups, eig, layout, weights)[0],
            cov64.covariance64(vel, r, k, groups, g, weights)[0])


def matrix_rel_max(got, ref):
    """the largest rel_max over the (moment, k-point) matrices, as tests/test_gpu_covariance.py takes it"""
    got, ref = np.asarray(got), np.asarray(ref)
    return max(float(np.max(np.abs(got[m, k] - ref[m, k])) / np.max(np.abs(ref[m, k]))) for m in range(ref.shape[0]) for k in range(ref.shape[1]))


ORDER = dict(ANGLE, ls=(4, 6), n_q=50)


def order_reference(data, case=ORDER):
    """order_cases.reference of the compact positions at the case's origins"""
    import order_cases
    groups = compact_groups(species(case["atoms"], case["parts"]))
    return order_cases.reference(data, BOXES[case["box"]], groups, case["r_cut"], case["step"], list(case["ls"]))


SPARSE_STEP = 700                      # origins 0, 700, 1400, 2100: one in each zone
LOCAL = dict(ANGLE, step=SPARSE_STEP, ls=(4, 6), n_q=50, n_w=50, w_range=0.2, threshold=0.5)
CLUSTER = dict(ANGLE, step=SPARSE_STEP, solid_l=6, threshold=0.4, min_connections=3, links=(0, 1), n_sizes=16)
CLUSTER_KEYS = ("size_counts", "large_atoms", "n_solid", "n_clusters", "largest", "largest_label", "labels", "size_atoms", "connections",
                "n", "bond_masks")


def local_reference(data, case=LOCAL, frames=None):
    """qlm_cases.reference of the compact positions at the case's origins, or (frames given) at those frames alone"""
    import qlm_cases
    groups = compact_groups(species(case["atoms"], case["parts"]))
    ls = list(case["ls"])
    if frames is not None:
        return qlm_cases.reference(data[np.asarray(frames)], BOXES[case["box"]], groups, case["r_cut"], 1, ls, ls[-1], case["threshold"])
    return qlm_cases.reference(data, BOXES[case["box"]], groups, case["r_cut"], case["step"], ls, ls[-1], case["threshold"])


def cluster_twin(data, link, case=CLUSTER):
    """cluster_cases.model: what Engine.solid_clusters(..., per_atom=True) returns, by the twin"""
    import cluster_cases
    groups = compact_groups(species(case["atoms"], case["parts"]))
    return cluster_cases.model(data, BOXES[case["box"]], groups, case["r_cut"], case["step"], case["solid_l"], case["threshold"],
                               case["min_connections"], link, case["n_sizes"])
