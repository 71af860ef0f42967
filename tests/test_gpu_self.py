"""The self (incoherent) spectra on the GPU (psa_self_spectra, `calculate_self_spectra`, `calculate_powder_self_spectra`):
the series kernel element by element inside the bound of tests/self_cases.py at every edge of its tiling, with the same bits
from a repeated call and from a call cut into blocks; the two calculator methods against the float64 restatement
(tests/self64.py) on the explicit full sphere; the shell form against the per-vector form; the invariants -- sum rule, frozen
atoms, ballistic lines, wrapped against unwrapped coordinates --; blockings, the atom draw; every refusal; no trace in a
later calculation.

The kernel's tiles (psa_amd/_hip.py mirrors psa_amd/csrc/self.hip): SELF_ATOMS = 4 atoms per atom tile, SELF_FRAMES = 64
frames per frame tile, vector tiles of at most SELF_KS = 64 vectors with at most SELF_ENTRIES = 24 distinct (axis, index)
pairs.  T = 250 frames is a multiple of none of them."""
import ctypes as Ct

import numpy as np
import pytest

import lattice64 as L64
import self64
import self_cases as S
from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = {"cubic": S.CUBIC, "triclinic": S.TRICLINIC}
T = 250
EDGES = np.array([0.05, 0.2, 0.45, 0.65, 0.85, 1.0, 1.15])                # those of test_gpu_lattice.py: the first shell is empty
SEGMENTS = {"none": None, "hann_64_32": (64, 32, "hann"), "boxcar_64_64": (64, 64, "boxcar")}
N0 = np.array([2, -1, 3], np.int32)


@pytest.fixture(autouse=True)
def _clean(engine):
    reset(engine)
    yield
    reset(engine)


@pytest.fixture(scope="module", autouse=True)
def _forget(engine):
    yield
    engine.invalidate()


def _resident(engine, pos):
    from psa_amd import _hip
    engine.ensure_resident(_hip.SLOT_POSITIONS, pos)


def _calculator(engine, pos, box, dt=0.002, cells=(1, 1, 1), vel=None):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos) if vel is None else vel, np.ones(n, np.int32), np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, *cells).attach(engine=engine)


def _segments(seg):
    from psa_amd import Segments
    return None if SEGMENTS[seg] is None else Segments(*SEGMENTS[seg])


def _window(s):
    return (None, None, None) if s is None else (s.window_array(), s.length, s.hop)


# ---- the series, per element ----------------------------------------------------------------------------------------------
def _index_set(kind, K, box):
    if kind == "corners":
        return S.C.corner_indices()
    if kind == "mixed":
        return S.C.mixed_indices(K, seed=K)
    if kind == "grid":
        return S.grid_indices(K)
    return np.random.default_rng(K).integers(-12, 13, (K, 3)).astype(np.int32)       # "scattered": a new entry with most vectors


_A = S.A
# (atoms, index set, K, box, far from the origin, weights, an index list in permuted order)
SERIES_CASES = [
    (1, "mixed", 1, "cubic", False, "unit", False),
    (_A - 1, "mixed", 2, "triclinic", False, "signed", True),             # holds n = 0
    (_A, "mixed", 4, "cubic", True, "sqrt_mass", False),                  # holds a pair n, -n
    (_A + 1, "corners", 8, "triclinic", True, "unit", True),              # +-64 on every axis, |k.r| ~ 1e4 rad
    (2 * _A + 3, "corners", 8, "cubic", True, "sqrt_mass", True),
    (1, "grid", 64, "triclinic", False, "signed", False),                 # exactly one vector tile
    (_A, "grid", 63, "triclinic", True, "sqrt_mass", True),               # one fewer
    (2 * _A + 3, "grid", 65, "cubic", False, "signed", True),             # one more: two tiles
    (_A + 1, "scattered", 150, "triclinic", False, "unit", False),        # tiles cut by their entries
]


def _series_id(c):
    return f"n{c[0]}_{c[1]}{c[2]}_{c[3]}_{'far' if c[4] else 'near'}_{c[5]}_{'idx' if c[6] else 'all'}"


@pytest.mark.parametrize("case", SERIES_CASES, ids=[_series_id(c) for c in SERIES_CASES])
def test_series_within_bound_same_bits_any_blocking(engine, case):
    from psa_amd import _hip
    n, kind, K, box_name, far, wk, listed = case
    box = BOXES[box_name]
    inv = S.inverse(box)
    ind = _index_set(kind, K, box)
    K = ind.shape[0]
    n_all = n + 5 if listed else n
    pos = S.far(n_all, T, seed=n + K, box=box) if far else S.C.trajectory(n_all, T, seed=n + K, box=box)[0]
    w = S.weights(wk, n_all, seed=2)
    idx = np.random.default_rng(3).permutation(n_all)[:n].astype(np.int32) if listed else None
    reach = S.C.max_abs_phase(pos, ind, inv, idx)
    if far and kind == "corners":
        assert reach >= 1e4
    sizes = S.tiles(ind)
    if kind == "grid":
        assert sizes == ([64, 1] if K == 65 else [K])
    if kind == "scattered":
        assert len(sizes) > 3 and max(sizes) < _hip.SELF_KS               # the table, not SELF_KS, cut these
    _resident(engine, pos)
    engine.set_atom_weights(w)
    got = engine.debug_self_series(inv, ind, idx)
    ref = self64.series64(pos, ind, inv, idx, w)
    assert got.shape == ref.shape == (n, K, T) and got.dtype == np.complex64
    wa = np.ones(n_all) if w is None else w.astype(np.float64)
    lim = S.bound(wa if idx is None else wa[idx])[:, None, None]
    frac = np.abs(got.astype(np.complex128) - ref) / lim
    worst = np.unravel_index(np.argmax(frac), frac.shape)
    print(f"{n} atoms, {K} vectors in tiles {sizes}, largest |k.r| {reach:.3e} rad: worst element {worst} at {frac[worst]:.4f} of "
          f"its bound ({lim[worst[0], 0, 0]:.3e})")
    assert frac.max() <= 1.0
    zero = np.flatnonzero(~ind.any(axis=1))
    assert zero.size >= (1 if kind == "mixed" and K >= 2 else 0)
    assert np.all(got[:, zero].imag == 0)                                  # n = 0: every factor is (1, 0) exactly
    again = engine.debug_self_series(inv, ind, idx)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))      # two identical calls: the same bits
    # a budget of two units (SELF_ATOMS atoms x the largest tile x T frames): blocks of atoms and of vector tiles
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 2 * _hip.SELF_ATOMS * max(sizes) * T * 8)
    blocked = engine.debug_self_series(inv, ind, idx)
    assert np.array_equal(got.view(np.uint32), blocked.view(np.uint32))
    # ... and whatever segments the context holds: the series come before the window
    from psa_amd import Segments
    engine.set_segments(Segments(64, 32, "hann"))
    assert np.array_equal(got.view(np.uint32), engine.debug_self_series(inv, ind, idx).view(np.uint32))


# ---- the calculator against float64 ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(BOXES))
def walk(request):
    """T = 250, N = 130, family (c), the half space of |k| < 1.15 in 6 shells of which the first is empty, sqrt_mass weights;
    the float64 densities of the explicit full sphere, once per segment shape"""
    from psa_amd import commensurate_vectors, shell_bins
    box = BOXES[request.param]
    inv = S.inverse(box)
    half, _, q = commensurate_vectors(box, EDGES[-1], EDGES[0])
    b, sel, avail, used = shell_bins(q, EDGES)
    half, b, q = half[sel], b[sel], q[sel]
    assert 100 <= half.shape[0] <= 300 and avail[0] == 0 and np.all(avail[1:] > 0)
    wrapped, unwrapped, _, _ = S.random_walk(130, T, seed=31, box=box)
    w = S.weights("sqrt_mass", 130, seed=23)
    full, b_full = np.concatenate([half, -half]), np.concatenate([b, b])
    cache = {}

    def ref(seg, pos=wrapped, idx=None):
        key = (seg, id(pos), None if idx is None else tuple(idx))
        if key not in cache:
            cache[key] = self64.density64(pos, full, inv, idx, w, *_window(_segments(seg)))
        return cache[key]
    return dict(box=box, inv=inv, half=half, bins=b, q=q, avail=avail, pos=wrapped, unwrapped=unwrapped, w=w, full=full,
                b_full=b_full, ref=ref, norm=float(np.sum(w.astype(np.float64) ** 2)))


@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_calculators_parity_float64_on_the_full_sphere(engine, walk, seg):
    from psa_amd import DynamicSpectra, PowderSpectra
    s = _segments(seg)
    L = T if s is None else s.length
    calc = _calculator(engine, walk["pos"], walk["box"])
    ref = walk["ref"](seg)
    per = calc.calculate_self_spectra(walk["full"], atom_weights=walk["w"], segments=s)
    assert isinstance(per, DynamicSpectra) and per.density.shape == (L, walk["full"].shape[0]) and per.density.dtype == np.float32
    assert per.longitudinal is None and per.transverse is None
    np.testing.assert_allclose(per.k_vectors, L64.lattice_k(walk["full"], walk["inv"]), rtol=0, atol=1e-13)
    np.testing.assert_allclose(per.freqs, np.fft.fftfreq(L, 0.002))
    assert per.weight_norm == pytest.approx(walk["norm"]) and np.array_equal(per.atoms, np.arange(130))
    cols = np.array([rel_max(per.density[:, k], ref[:, k]) for k in range(ref.shape[1])])
    print(f"{seg}: per vector, rel_max per column: largest {cols.max():.2e}, median {np.median(cols):.2e}")
    assert cols.max() <= 1e-5
    # not the coherent spectrum (a test that passed by returning it would go unnoticed otherwise)
    coh = calc.calculate_lattice_spectra(walk["full"][:8], atom_weights=walk["w"], segments=s, currents=False)
    assert np.max(np.abs(coh.density - per.density[:, :8])) > 0.1 * per.density[:, :8].max()
    # the powder average against the mean over the explicit full sphere, nothing folded
    pw = calc.calculate_powder_self_spectra(EDGES, atom_weights=walk["w"], segments=s)
    want = self64.shell_mean64(ref, walk["b_full"], 6)
    assert isinstance(pw, PowderSpectra) and pw.density.shape == (L, 6) and pw.density.dtype == np.float32
    assert pw.longitudinal is None and pw.transverse is None
    err = rel_max(pw.density, want)
    host = self64.shell_mean64(per.density.astype(np.float64), walk["b_full"], 6)
    shell = rel_max(pw.density, host)
    print(f"{seg}: powder against float64 {err:.2e}; shell form against the per-vector form averaged on the host {shell:.2e}")
    assert err <= 1e-5
    assert shell <= 1e-6
    assert not pw.density[:, 0].any()                                      # the empty shell
    np.testing.assert_array_equal(pw.counts, 2 * np.bincount(walk["bins"], minlength=6))
    np.testing.assert_array_equal(pw.available, 2 * walk["avail"])
    assert np.isnan(pw.q[0])
    np.testing.assert_allclose(pw.q[1:], [walk["q"][walk["bins"] == i].mean() for i in range(1, 6)], rtol=1e-14)
    assert np.array_equal(pw.indices, walk["half"]) and np.array_equal(pw.bin_index, walk["bins"])
    np.testing.assert_allclose(pw.freqs, np.fft.fftfreq(L, 0.002))
    assert pw.weight_norm == pytest.approx(walk["norm"])
    np.testing.assert_allclose(pw.structure_factor, pw.density.astype(np.float64) * L * 0.002 / walk["norm"])


# ---- invariants ---------------------------------------------------------------------------------------------------------------
def test_sum_rule(engine, walk):
    """no segments: sum_o density[o,n] = sum_a w_a^2 for every vector of the random walk"""
    per = _calculator(engine, walk["pos"], walk["box"]).calculate_self_spectra(walk["full"], atom_weights=walk["w"])
    total = per.density.astype(np.float64).sum(0)
    print(f"sum rule: largest deviation {np.max(np.abs(total / per.weight_norm - 1)):.2e}")
    assert np.all(np.abs(total - per.weight_norm) <= 1e-5 * per.weight_norm)


@pytest.mark.parametrize("box_name", list(BOXES))
def test_frozen_atoms(engine, box_name):
    box = BOXES[box_name]
    pos = S.frozen(37, T, seed=5, box=box)
    w = S.weights("signed", 37, seed=6)
    ind = np.concatenate([S.C.mixed_indices(4, seed=4), S.C.corner_indices()[:2]])
    per = _calculator(engine, pos, box).calculate_self_spectra(ind, atom_weights=w)
    total = float(np.sum(w.astype(np.float64) ** 2))
    floor = (float(S.bound(1.0)) * float(np.sum(np.abs(w.astype(np.float64))))) ** 2
    print(f"frozen: bin 0 off by {np.max(np.abs(per.density[0] / total - 1)):.2e}; largest value elsewhere {per.density[1:].max():.3e} "
          f"(allowed {floor:.3e})")
    assert np.all(np.abs(per.density[0] - total) <= 1e-5 * total)
    assert np.all(per.density[1:] <= floor)


@pytest.mark.parametrize("box_name", list(BOXES))
def test_ballistic_lines(engine, box_name):
    """family (b): atom a moves n0.sigma_a T = b_a turns in T frames and is a line of height w_a^2 in bin b_a of column n0,
    wrapped into the box as it goes"""
    box = BOXES[box_name]
    pos, b = S.ballistic(100, T, seed=7, n0=N0, box=box)
    w = S.weights("sqrt_mass", 100, seed=8)
    ind = np.stack([N0, -N0, [1, 0, 0]]).astype(np.int32)
    per = _calculator(engine, pos, box).calculate_self_spectra(ind, atom_weights=w)
    want = np.zeros(T)
    want[b % T] = w.astype(np.float64) ** 2
    print(f"ballistic: {rel_max(per.density[:, 0], want):.2e} of the largest line; mirrored column {rel_max(per.density[:, 1], want[(T - np.arange(T)) % T]):.2e}")
    assert rel_max(per.density[:, 0], want) <= 1e-5
    assert rel_max(per.density[:, 1], want[(T - np.arange(T)) % T]) <= 1e-5   # -n0: the lines at the mirrored frequency


def test_wrapped_against_unwrapped(engine, walk):
    s = _segments("hann_64_32")
    ind = walk["full"][::7]
    ref_w = walk["ref"]("hann_64_32")[:, ::7]
    ref_u = self64.density64(walk["unwrapped"], ind, walk["inv"], None, walk["w"], *_window(s))
    got_w = _calculator(engine, walk["pos"], walk["box"]).calculate_self_spectra(ind, atom_weights=walk["w"], segments=s).density
    got_u = _calculator(engine, walk["unwrapped"], walk["box"]).calculate_self_spectra(ind, atom_weights=walk["w"], segments=s).density
    print(f"wrapped against the unwrapped reference {rel_max(got_w, ref_u):.2e}, unwrapped against the wrapped reference "
          f"{rel_max(got_u, ref_w):.2e}; the two references {rel_max(ref_u, ref_w):.2e}")
    assert rel_max(got_w, ref_u) <= 1e-5
    assert rel_max(got_u, ref_w) <= 1e-5


# ---- blocking, determinism, the atom draw ------------------------------------------------------------------------------------
def test_blockings_repeat_max_atoms(engine, walk):
    from psa_amd import _hip
    s = _segments("hann_64_32")
    _resident(engine, walk["pos"])
    engine.set_atom_weights(walk["w"])
    engine.set_segments(s)
    inv, half, bins = walk["inv"], walk["half"], walk["bins"]
    one = engine.self_spectra(inv, half, bins, 6, None)
    again = engine.self_spectra(inv, half, bins, 6, None)
    assert np.array_equal(one.view(np.uint32), again.view(np.uint32))
    per_one = engine.self_spectra(inv, half, None, 0, None)
    assert np.array_equal(per_one.view(np.uint32), engine.self_spectra(inv, half, None, 0, None).view(np.uint32))
    # 20 units: 20 of the 33 atom tiles, one of several vector tiles, one of 6 segments per block
    sizes = S.tiles(half, bins)
    n_at, n_seg = -(-130 // _hip.SELF_ATOMS), s.count(T)
    assert n_at > 20 and len(sizes) > 1 and n_seg == 6
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 20 * _hip.SELF_ATOMS * max(sizes) * 64 * 8)
    cut = engine.self_spectra(inv, half, bins, 6, None)
    ulp = np.spacing(np.maximum(np.abs(one), np.abs(cut)))
    print(f"shell form, two blockings: largest difference {np.max(np.abs(one - cut) / ulp):.2f} ulp, {np.count_nonzero(one != cut)} of {one.size} differ")
    assert np.all(np.abs(one - cut) <= ulp)
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 20 * _hip.SELF_ATOMS * max(S.tiles(half)) * 64 * 8)
    per_cut = engine.self_spectra(inv, half, None, 0, None)
    ulp = np.spacing(np.maximum(np.abs(per_one), np.abs(per_cut)))
    print(f"per vector, two blockings: largest difference {np.max(np.abs(per_one - per_cut) / ulp):.2f} ulp")
    assert np.all(np.abs(per_one - per_cut) <= ulp)
    reset(engine)
    # an empty atom set gives zeros
    engine.set_segments(s)
    assert not engine.self_spectra(inv, half, bins, 6, np.zeros(0, np.int32)).any()
    assert not engine.self_spectra(inv, half, None, 0, np.zeros(0, np.int32)).any()
    assert engine.debug_self_series(inv, half, np.zeros(0, np.int32)).shape == (0, half.shape[0], T)
    reset(engine)
    # max_atoms
    calc = _calculator(engine, walk["pos"], walk["box"])
    some = calc.calculate_self_spectra(walk["full"], atom_weights=walk["w"], segments=s, max_atoms=40, seed=0)
    assert some.atoms.shape == (40,) and np.unique(some.atoms).size == 40
    assert some.weight_norm == pytest.approx(float(np.sum(walk["w"][some.atoms].astype(np.float64) ** 2)))
    ref = walk["ref"]("hann_64_32", idx=some.atoms)
    cols = np.array([rel_max(some.density[:, k], ref[:, k]) for k in range(ref.shape[1])])
    print(f"max_atoms = 40: rel_max per column, largest {cols.max():.2e}")
    assert cols.max() <= 1e-5
    other = calc.calculate_self_spectra(walk["full"][:3], atom_weights=walk["w"], segments=s, max_atoms=40, seed=1)
    assert other.atoms.shape == (40,) and not np.array_equal(other.atoms, some.atoms)
    pw = calc.calculate_powder_self_spectra(EDGES, atom_weights=walk["w"], segments=s, max_atoms=40, max_per_bin=9, seed=0)
    assert np.array_equal(pw.atoms, some.atoms)
    np.testing.assert_array_equal(pw.counts, 2 * np.minimum(walk["avail"], 9))
    full, b_full = np.concatenate([pw.indices, -pw.indices]), np.concatenate([pw.bin_index, pw.bin_index])
    want = self64.shell_mean64(self64.density64(walk["pos"], full, inv, some.atoms, walk["w"], *_window(s)), b_full, 6)
    assert rel_max(pw.density, want) <= 1e-5


# ---- refusals, and no trace --------------------------------------------------------------------------------------------------
def test_refusals(engine, walk):
    from psa_amd import Segments, _hip
    pos, inv = walk["pos"], np.ascontiguousarray(walk["inv"])
    _resident(engine, pos)
    lib, h = engine._lib, engine._h
    f32p, i32p, f64p = Ct.POINTER(Ct.c_float), Ct.POINTER(Ct.c_int32), Ct.POINTER(Ct.c_double)
    ind = np.ascontiguousarray(walk["half"][:9])
    bins = np.ascontiguousarray(walk["bins"][:9])
    out, sh = np.empty((T, 9), np.float32), np.empty((T, 6), np.float32)
    bp, ip, op, sp = inv.ctypes.data_as(f64p), ind.ctypes.data_as(i32p), out.ctypes.data_as(f32p), sh.ctypes.data_as(f32p)
    binp = bins.ctypes.data_as(i32p)

    def refused(rc, word):
        msg = lib.psa_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    assert lib.psa_self_spectra(h, bp, ip, 9, None, 0, None, 0, op, out.nbytes) == 0
    assert lib.psa_self_spectra(h, bp, ip, 9, binp, 6, None, 0, sp, sh.nbytes) == 0
    refused(lib.psa_self_spectra(h, None, ip, 9, None, 0, None, 0, op, out.nbytes), "null")
    refused(lib.psa_self_spectra(h, bp, None, 9, None, 0, None, 0, op, out.nbytes), "null")
    refused(lib.psa_self_spectra(h, bp, ip, 9, None, 0, None, 0, None, out.nbytes), "null")
    refused(lib.psa_debug_self_series(h, bp, ip, 9, None, 0, None), "null")
    refused(lib.psa_self_spectra(h, bp, ip, 0, None, 0, None, 0, op, out.nbytes), "at least one")
    refused(lib.psa_self_spectra(h, bp, ip, 9, None, 0, None, 0, op, out.nbytes - 4), "out_bytes")
    refused(lib.psa_self_spectra(h, bp, ip, 9, binp, 6, None, 0, op, out.nbytes), "out_bytes")       # the shell form is (L, n_bins)
    refused(lib.psa_self_spectra(h, np.zeros(9).ctypes.data_as(f64p), ip, 9, None, 0, None, 0, op, out.nbytes), "singular")
    far = ind.copy()
    far[4, 1] = -_hip.LAT_MAX_INDEX - 1
    refused(lib.psa_self_spectra(h, bp, far.ctypes.data_as(i32p), 9, None, 0, None, 0, op, out.nbytes), "is served")
    bb = bins.copy()
    bb[2] = 6
    refused(lib.psa_self_spectra(h, bp, ip, 9, bb.ctypes.data_as(i32p), 6, None, 0, sp, sh.nbytes), "outside")
    for bad_n in ((0, 0, 0), (0, -1, 2), (-1, 2, 2)):
        nn = ind.copy()
        nn[7] = bad_n
        refused(lib.psa_self_spectra(h, bp, nn.ctypes.data_as(i32p), 9, binp, 6, None, 0, sp, sh.nbytes), "half-space")
        assert lib.psa_self_spectra(h, bp, nn.ctypes.data_as(i32p), 9, None, 0, None, 0, op, out.nbytes) == 0   # per vector: allowed
    bad = np.array([3, 130], np.int32)
    refused(lib.psa_self_spectra(h, bp, ip, 9, None, 0, bad.ctypes.data_as(i32p), 2, op, out.nbytes), "out of bounds")
    engine.set_atom_weights(np.ones(129, np.float32))
    refused(lib.psa_self_spectra(h, bp, ip, 9, None, 0, None, 0, op, out.nbytes), "weights")
    engine.set_atom_weights(None)
    unit = _hip.SELF_ATOMS * 9 * T * 8                                    # the 9 vectors are one tile
    assert S.tiles(ind) == [9]
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, unit - 1)
    refused(lib.psa_self_spectra(h, bp, ip, 9, None, 0, None, 0, op, out.nbytes), "budget")
    assert str(unit) in lib.psa_last_error().decode()                     # the message names the smallest block's bytes
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, unit)
    assert lib.psa_self_spectra(h, bp, ip, 9, None, 0, None, 0, op, out.nbytes) == 0
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
    engine.set_segments(Segments(512, 256, "hann"))
    big = np.empty((512, 9), np.float32)
    refused(lib.psa_self_spectra(h, bp, ip, 9, None, 0, None, 0, big.ctypes.data_as(f32p), big.nbytes), "segment length")
    engine.set_segments(None)
    engine.release(_hip.SLOT_VELOCITIES)                                  # the self part needs no velocities
    assert lib.psa_self_spectra(h, bp, ip, 9, None, 0, None, 0, op, out.nbytes) == 0
    engine.release(_hip.SLOT_POSITIONS)
    refused(lib.psa_self_spectra(h, bp, ip, 9, None, 0, None, 0, op, out.nbytes), "positions")
    refused(lib.psa_debug_self_series(h, bp, ip, 9, None, 0, out.ctypes.data_as(Ct.c_void_p)), "positions")


def test_no_trace_in_the_other_entry_points(engine, walk):
    """`calculate`, `calculate_powder_spectra` and `calculate_vdos` give the bits they gave before the self calls in between"""
    vel = S.C.trajectory(130, T, seed=41, box=walk["box"])[1]
    calc = _calculator(engine, walk["pos"], walk["box"], cells=(4, 4, 4), vel=vel)
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    for _ in range(2):                      # (the first call uploads and projects at once, the next builds what is cached)
        calc.calculate(mags, vecs)
    s = _segments("hann_64_32")
    before = calc.calculate(mags, vecs)
    pw_before = calc.calculate_powder_spectra(EDGES, segments=s, atom_weights=walk["w"])
    dos_before = calc.calculate_vdos(segments=s, atom_weights=walk["w"])
    engine.timings()                                                       # (reset)
    calc.calculate_powder_self_spectra(EDGES, segments=s, atom_weights=walk["w"])
    timings = engine.timings()
    assert timings["transpose"] > 0 and timings["fft"] > 0 and timings["epilogue"] > 0 and timings["d2h"] > 0
    calc.calculate_self_spectra(walk["half"][:20], max_atoms=17)
    after = calc.calculate(mags, vecs)
    pw_after = calc.calculate_powder_spectra(EDGES, segments=s, atom_weights=walk["w"])
    dos_after = calc.calculate_vdos(segments=s, atom_weights=walk["w"])
    assert np.array_equal(before.sed.view(np.uint32), after.sed.view(np.uint32))
    for name in ("density", "longitudinal", "transverse"):
        assert np.array_equal(getattr(pw_before, name).view(np.uint32), getattr(pw_after, name).view(np.uint32)), name
    assert np.array_equal(dos_before.dos.view(np.uint32), dos_after.dos.view(np.uint32))
