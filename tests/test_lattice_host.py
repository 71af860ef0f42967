"""The spectra on the box's reciprocal lattice without a GPU: the enumeration of the commensurate vectors and the shell
bins (psa_amd/lattice.py) against brute force, the projection kernel's bound (tests/lattice_cases.py) against a float32
model of its arithmetic -- and against the arithmetic it must not use --, the fold of a pair (n, -n) with and without
the frequency mirror against the full sphere (tests/lattice64.py), and the argument checks of the Python layer that need
no device."""
import re
from pathlib import Path

import numpy as np
import pytest

import lattice64 as L64
import lattice_cases as C
from psa_amd import (DynamicSpectra, PowderSpectra, SEDCalculator, Segments, Trajectory, _hip, commensurate_vectors,
                     shell_bins)


# ---- (a) the vectors --------------------------------------------------------------------------------------------
def brute_force(box, q_max, q_min, half):
    """the integer cube, vector by vector"""
    inv = C.inverse(box)
    reach = int(np.ceil(q_max * np.max(np.linalg.norm(np.asarray(box, np.float64), axis=1)) / (2 * np.pi))) + 1
    found = set()
    for a in range(-reach, reach + 1):
        for b in range(-reach, reach + 1):
            for c in range(-reach, reach + 1):
                if (a, b, c) == (0, 0, 0):
                    continue
                lead = a if a else b if b else c
                if half and lead < 0:
                    continue
                q = float(np.linalg.norm(2 * np.pi * (np.array([a, b, c], np.float64) @ inv.T)))
                if q_min <= q <= q_max:
                    found.add((a, b, c))
    return found


@pytest.mark.parametrize("box", [C.CUBIC, C.TRICLINIC], ids=["cubic", "triclinic"])
@pytest.mark.parametrize("half", [True, False], ids=["half", "full"])
def test_commensurate_vectors_equal_the_integer_cube(box, half):
    q_max, q_min = 1.3, 0.35
    n, k, q = commensurate_vectors(box, q_max, q_min, half_space=half)
    want = brute_force(box, q_max, q_min, half)
    got = {tuple(int(x) for x in row) for row in n}
    print(f"{len(got)} vectors, brute force {len(want)}")
    assert n.dtype == np.int32 and k.dtype == np.float64 and q.dtype == np.float64
    assert len(got) == n.shape[0] == len(want) and got == want
    assert (0, 0, 0) not in got
    np.testing.assert_allclose(k, L64.lattice_k(n, C.inverse(box)), rtol=0, atol=1e-14)
    np.testing.assert_allclose(q, np.linalg.norm(k, axis=1), rtol=1e-15)
    key = np.rint(q / (q_max * 1e-12))                                     # |k| as the order compares it: to 1e-12 of q_max
    assert np.all(np.diff(key) >= 0)                                       # sorted by |k| ...
    same = np.flatnonzero(np.diff(key) == 0)
    assert all(tuple(n[i]) < tuple(n[i + 1]) for i in same)                # ... then by index
    # vectors equivalent by symmetry sit together whatever the last bits of their norms
    if box is C.CUBIC:
        sq = np.sum(n.astype(np.int64) ** 2, axis=1)
        assert np.all(np.diff(sq) >= 0) and all(tuple(n[i]) < tuple(n[i + 1]) for i in np.flatnonzero(np.diff(sq) == 0))
    if half:
        assert all(tuple(-x for x in v) not in got for v in got)          # exactly one of each pair
        full = {tuple(int(x) for x in row) for row in commensurate_vectors(box, q_max, q_min, half_space=False)[0]}
        assert full == got | {tuple(-x for x in v) for v in got}
    else:
        assert all(tuple(-x for x in v) in got for v in got)              # every -n is present


def test_commensurate_vectors_refuse_bad_input():
    with pytest.raises(ValueError, match="singular"):
        commensurate_vectors(np.zeros((3, 3), np.float32), 1.0)
    with pytest.raises(ValueError, match="q_min"):
        commensurate_vectors(C.CUBIC, 1.0, 2.0)
    with pytest.raises(ValueError, match=r"\(3, 3\)"):
        commensurate_vectors(np.ones((2, 3)), 1.0)


def test_shell_bins_counts_selection_and_an_empty_bin():
    _, _, q = commensurate_vectors(C.CUBIC, 1.0)
    g1 = 2 * np.pi / 21.72
    edges = np.array([0.9 * g1, 1.1 * g1, 1.2 * g1, 1.5 * g1, 2.05 * g1, 3.3 * g1])       # the third holds (1,1,0), ...
    b, sel, avail, used = shell_bins(q, edges)
    want = np.array([np.sum((q >= edges[i]) & (q < edges[i + 1])) for i in range(5)])
    print("available", avail, "used", used)
    assert b.dtype == np.int32 and sel.dtype == bool
    np.testing.assert_array_equal(avail, want)
    np.testing.assert_array_equal(used, want)
    assert avail[0] == 3 and avail[1] == 0 and avail[2] == 6               # (100) x 3 half-space; nothing; (110) x 6
    assert np.all(sel == (b >= 0)) and np.all(b[(q < edges[0]) | (q >= edges[-1])] == -1)
    for i in range(5):
        assert np.all((q[b == i] >= edges[i]) & (q[b == i] < edges[i + 1]))
    # a cap: the draw is the seed's
    b1, s1, a1, u1 = shell_bins(q, edges, max_per_bin=5, seed=7)
    b2, s2, a2, u2 = shell_bins(q, edges, max_per_bin=5, seed=7)
    b3, s3, a3, u3 = shell_bins(q, edges, max_per_bin=5, seed=8)
    np.testing.assert_array_equal(a1, avail)
    np.testing.assert_array_equal(u1, np.minimum(avail, 5))
    assert np.array_equal(s1, s2) and np.array_equal(b1, b) and not np.array_equal(s1, s3)
    assert np.all(b1[s1] >= 0) and np.all(np.bincount(b1[s1], minlength=5) == u1)
    with pytest.raises(ValueError, match="ascending"):
        shell_bins(q, [0.5, 0.5])
    with pytest.raises(ValueError, match="max_per_bin"):
        shell_bins(q, edges, max_per_bin=0)


# ---- (b) the bound can fail ---------------------------------------------------------------------------------------
def _indices(kind):
    if kind == "corners":
        return C.corner_indices()
    if kind == "mixed":
        return C.mixed_indices(6, seed=4)
    return commensurate_vectors(C.TRICLINIC, 0.5)[0][:12]


FAMILIES = [  # atoms, frames, box, shift, index set, weights, index list, currents
    (40, 2, "cubic", 0, "mixed", "unit", False, True),
    (40, 2, "triclinic", 40, "corners", "signed", False, True),           # the family of the proof below
    (33, 2, "triclinic", 40, "mixed", "sqrt_mass", True, False),
    (2 * _hip.LAT_CHAIN + 3, 1, "cubic", 0, "sphere", "unit", True, True),  # two folds and a rest
]


def _family(n, T, box, shift, kind, wk, listed, currents):
    H = C.CUBIC if box == "cubic" else C.TRICLINIC
    inv = C.inverse(H)
    pos, vel = C.trajectory(n, T, seed=n + shift, box=H, shift=shift)
    idx = np.random.default_rng(2).permutation(n)[: n - 3].astype(np.int32) if listed else None
    w = C.weights(wk, n, seed=1)
    ind = _indices(kind)
    ref, absum = L64.project64(pos, vel, ind, inv, idx, w, currents, with_abs=True)
    return pos, vel, ind, inv, idx, w, ref, C.bound(absum, n if idx is None else idx.size)[None]


@pytest.mark.parametrize("family", FAMILIES, ids=[f"n{f[0]}_{f[2]}_{f[4]}_{f[3]}" for f in FAMILIES])
def test_bound_holds_for_the_kernels_arithmetic(family):
    n, T, box, shift, kind, wk, listed, currents = family
    assert C.eps_lat() <= C.EPS_TERM_CAP
    pos, vel, ind, inv, idx, w, ref, lim = _family(*family)
    reach = C.max_abs_phase(pos, ind, inv, idx)
    good, term = C.project_model(pos, vel, ind, inv, idx, w, currents, with_term_error=True)
    frac = float(np.max(np.abs(good - ref) / lim))
    print(f"n = {n}, {box}, {kind}, largest |k.r| {reach:.3e} rad: worst unit-modulus term off by {term:.3e} "
          f"({term / C.eps_lat():.3f} of eps_lat = {C.eps_lat():.3e}), worst element at {frac:.4f} of its bound")
    assert term <= C.eps_lat()
    assert frac <= 1.0


def test_one_float32_per_coordinate_lands_over_the_cap_at_the_largest_indices():
    """The proof that the test can fail, on indices of +-LAT_MAX_INDEX and an unwrapped trajectory: the model of the
    kernel's arithmetic stays inside eps_lat and the bound; the same model with s_j rounded to one float32 has its worst
    unit-modulus term over the cap 2^-18 the project allows a term (the element bound, which also holds 128 u for the
    chain and meets errors of random sign, is not what shows it: the term is)."""
    family = FAMILIES[1]
    assert family[4] == "corners" and family[3] == 40
    pos, vel, ind, inv, idx, w, ref, lim = _family(*family)
    reach = C.max_abs_phase(pos, ind, inv, idx)
    assert np.max(np.abs(ind)) == _hip.LAT_MAX_INDEX and 1e4 <= reach <= 6e4
    good, term_good = C.project_model(pos, vel, ind, inv, idx, w, True, with_term_error=True)
    bad, term_bad = C.project_model(pos, vel, ind, inv, idx, w, True, single=True, with_term_error=True)
    r_good, r_bad = float(np.max(np.abs(good - ref) / lim)), float(np.max(np.abs(bad - ref) / lim))
    print(f"largest |k.r| {reach:.3e} rad: two float32 per coordinate: term {term_good:.3e} = {term_good / C.EPS_TERM_CAP:.3f} of "
          f"the cap, element at {r_good:.4f} of the bound; one float32: term {term_bad:.3e} = {term_bad / C.EPS_TERM_CAP:.2f} x the "
          f"cap, element at {r_bad:.2f} x the bound")
    assert term_good <= C.eps_lat() <= C.EPS_TERM_CAP < term_bad
    assert r_good <= 1.0


def test_constants_mirror_the_kernels():
    text = (Path(_hip.__file__).resolve().parent / "csrc" / "psa_ctx.h").read_text()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (LAT_[A-Z_]+) = (\d+);", text)}
    assert set(found) == {"LAT_THREADS", "LAT_KS", "LAT_ATOMS", "LAT_TABLE", "LAT_CHAIN", "LAT_FRAMES", "LAT_MAX_INDEX"}
    for name, value in found.items():
        assert getattr(_hip, name) == value, name
    assert _hip.LAT_MAX_INDEX >= 64 and _hip.LAT_MAX_ENTRIES == 3 * (2 * _hip.LAT_MAX_INDEX + 1)
    assert _hip.LAT_TABLE // _hip.LAT_MAX_ENTRIES >= 1                      # the widest tile still stages an atom
    assert _hip.ABI_VERSION == 6 and {"psa_lattice_spectra", "psa_debug_lattice_project"} <= set(_hip.SIGNATURES)


# ---- (c) the fold and its mirror ------------------------------------------------------------------------------------
def test_fold_with_the_mirror_is_the_full_sphere_and_without_it_is_not():
    box, T, N = C.TRICLINIC, 64, 30
    inv = C.inverse(box)
    half, _, q = commensurate_vectors(box, 0.62)
    k0 = half[5]
    pos, vel = C.travelling_wave(N, T, box, k0, bin0=5)
    edges = np.linspace(0.2, 0.62, 4)
    b_half, sel, _, used = shell_bins(q, edges)
    half, b_half = half[sel], b_half[sel]
    full, b_full = np.concatenate([half, -half]), np.concatenate([b_half, b_half])
    ref = L64.powder64(pos, vel, full, inv, b_full, 3)
    per = L64.spectra64(L64.project64(pos, vel, half, inv), half, inv)
    good, bad = L64.fold64(per, b_half, 3, mirror=True), L64.fold64(per, b_half, 3, mirror=False)
    for name, r, g, w in zip(("density", "longitudinal", "transverse"), ref, good, bad):
        e_good, e_bad = np.max(np.abs(g - r)) / np.max(r), np.max(np.abs(w - r)) / np.max(r)
        print(f"{name}: fold with the mirror off by {e_good:.2e} of the largest value, without it by {e_bad:.2e}")
        assert e_good <= 1e-12
        assert e_bad > 100 * 1e-5


# ---- (d) the Python layer ---------------------------------------------------------------------------------------------
def _calculator(n_atoms=8, n_frames=16, box=C.CUBIC):
    pos, vel = C.trajectory(n_atoms, n_frames, seed=1, box=box)
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, vel, np.ones(n_atoms, np.int32), np.arange(n_frames, dtype=np.float32), box, np.diag(box).copy(),
                    np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, 4, 4, 4)


@pytest.mark.parametrize("method", ["lattice", "powder"])
def test_argument_checks_need_no_device(method):
    calc = _calculator()
    g1 = 2 * np.pi / 21.72
    first = C.mixed_indices(3, seed=1) if method == "lattice" else np.array([0.5 * g1, 1.5 * g1, 2.5 * g1])
    call = calc.calculate_lattice_spectra if method == "lattice" else calc.calculate_powder_spectra
    with pytest.raises(TypeError, match="Segments"):
        call(first, segments=(8, 4))
    with pytest.raises(ValueError):
        call(first, segments=Segments(32, 16, "hann"))                      # L > T
    with pytest.raises(ValueError, match="atom_weights"):
        call(first, atom_weights=np.ones(7))
    with pytest.raises(ValueError, match="out of bounds"):
        call(first, basis_atom_indices=[0, 8])
    if method == "lattice":
        with pytest.raises(ValueError, match=r"\(K, 3\)"):
            call(first[:, :2])
        with pytest.raises(ValueError, match="integers"):
            call(np.array([[0.5, 1.0, 0.0]]))
        with pytest.raises(ValueError, match="served"):
            call(np.array([[_hip.LAT_MAX_INDEX + 1, 0, 0]]))
    else:
        with pytest.raises(ValueError, match="ascending"):
            call([1.0, 0.5])
        with pytest.raises(ValueError, match="served"):
            call([0.0, (_hip.LAT_MAX_INDEX + 1.01) * g1])
        from psa_amd import lattice                                        # a shell that ends between two indices is served
        assert lattice.index_reach(C.CUBIC, (_hip.LAT_MAX_INDEX + 0.5) * g1).max() == _hip.LAT_MAX_INDEX
        with pytest.raises(ValueError, match="max_per_bin"):
            call(first, max_per_bin=0)

    class TwoRanks:
        nranks, mode, engine = 2, "k", None
    calc._shard = TwoRanks()
    with pytest.raises(NotImplementedError, match="sharded"):
        call(first)
    calc._shard = None
    assert calc._engine is None                                            # nothing above reached for a device


def test_empty_inputs_and_the_result_types():
    calc = _calculator()
    out = calc.calculate_lattice_spectra(np.zeros((0, 3), np.int32), segments=Segments(8, 4, "hann"), currents=False)
    assert isinstance(out, DynamicSpectra) and out.density.shape == (8, 0) and out.longitudinal is None
    assert out.freqs.shape == (8,) and out.k_vectors.shape == (0, 3) and out.dt_ps == 0.002
    g1 = 2 * np.pi / 21.72
    pw = calc.calculate_powder_spectra([0.2 * g1, 0.6 * g1, 0.9 * g1])      # no vector below the first shell |G_1|
    assert isinstance(pw, PowderSpectra) and pw.density.shape == (16, 2) and pw.transverse.shape == (16, 2)
    assert np.all(pw.density == 0) and np.all(pw.counts == 0) and np.all(pw.available == 0) and np.all(np.isnan(pw.q))
    assert pw.indices.shape == (0, 3) and pw.bin_index.shape == (0,) and pw.q_edges.shape == (3,)
    assert calc._engine is None
    empty = SEDCalculator(Trajectory(np.zeros((0, 4, 3), np.float32), np.zeros((0, 4, 3), np.float32), np.ones(4, np.int32),
                                     np.zeros(0, np.float32), C.CUBIC, np.diag(C.CUBIC).copy(), np.zeros(3, np.float32), 0.002), 1, 1, 1)
    pw0 = empty.calculate_powder_spectra([0.9 * g1, 1.1 * g1])
    assert pw0.density.shape == (0, 1) and pw0.counts[0] == 6 and pw0.available[0] == 6 and empty._engine is None
    p = PowderSpectra(np.full((4, 2), 3.0, np.float32), None, None, np.ones(2), np.arange(3.0), np.ones(2, int), np.ones(2, int),
                      np.zeros((2, 3), np.int32), np.zeros(2, np.int32), np.fft.fftfreq(4, 0.5), np.arange(5), 6.0)
    np.testing.assert_allclose(p.structure_factor, 3.0 * 4 * 0.5 / 6.0)     # density L dt / sum w^2, dt from freqs
