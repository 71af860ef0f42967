"""The spectra on the box's reciprocal lattice on the GPU (psa_lattice_spectra, `calculate_lattice_spectra`,
`calculate_powder_spectra`): the projection kernel element by element inside the bound of tests/lattice_cases.py at every
edge of its tiling, with the same bits from a repeated call and from a call cut into blocks of vectors; the cross-check
with the kernel of psa_dynamic_spectra on float32(n.G); the Bragg peaks of a perfect crystal; the two calculator methods
against the float64 restatement (tests/lattice64.py) on the explicit full sphere, on a travelling wave for which the
frequency mirror of a folded pair matters; the shell form against the per-vector form; every refusal; no trace in a later
calculation.

The kernel's tiles (psa_amd/_hip.py mirrors psa_amd/csrc/lattice.hip): LAT_KS = 512 vectors per tile, two per lane;
LAT_CHAIN = 128 atoms per float32 accumulator; LAT_FRAMES = 4 frames per workgroup; atoms staged in tiles of
A = min(LAT_ATOMS, LAT_TABLE // R) with R the distinct (axis, index) pairs of the tile's vectors."""
import ctypes as Ct

import numpy as np
import pytest

import dynamic64
import dynamic_cases
import lattice64 as L64
import lattice_cases as C
from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = {"cubic": C.CUBIC, "triclinic": C.TRICLINIC}


@pytest.fixture(autouse=True)
def _clean(engine):
    reset(engine)
    yield
    reset(engine)


@pytest.fixture(scope="module", autouse=True)
def _forget(engine):
    yield
    engine.invalidate()


def _resident(engine, pos, vel):
    from psa_amd import _hip
    engine.ensure_resident(_hip.SLOT_POSITIONS, pos)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, vel)


def _sphere(box, K):
    """the K shortest half-space vectors of the box, in the order of commensurate_vectors"""
    from psa_amd import commensurate_vectors
    n = commensurate_vectors(box, 2.6)[0]
    assert n.shape[0] >= K
    return n[:K]


def _index_set(kind, K, box):
    if kind == "halfsphere":                                               # every half-space vector up to |k| = 1.2 / A
        from psa_amd import commensurate_vectors
        return commensurate_vectors(box, 1.2)[0]
    if kind == "corners":
        return C.corner_indices()[:K]
    if kind == "mixed":
        return C.mixed_indices(K, seed=K)
    return _sphere(box, K)


def _tile_atoms(indices):
    """atoms per staged tile for the first tile of a one-block call: the API sorts by index and cuts tiles of LAT_KS"""
    from psa_amd import _hip
    n = np.asarray(indices)
    first = n[np.lexsort((n[:, 2], n[:, 1], n[:, 0]))][:_hip.LAT_KS]
    R = sum(np.unique(first[:, j]).size for j in range(3))
    return min(_hip.LAT_ATOMS, _hip.LAT_TABLE // R)


# ---- the per-element bound ------------------------------------------------------------------------------------------
# (atoms: a number, or ("tile", d) for the atom tile of the index set + d, or ("tiles", d) for two tiles + d; frames; index
#  set; K; box; shift in box vectors; weights; index list; currents)
_CH, _KS = 128, 512
BOUND_CASES = [
    (1, 1, "mixed", 1, "cubic", 0, "unit", False, True),                  # N = 1: the index map; a wrong entry is O(1) off
    (2, 3, "mixed", 2, "triclinic", 0, "signed", False, False),           # holds n = 0
    (1, 4, "corners", 8, "triclinic", 40, "unit", False, True),           # +-64 on every axis, all eight sign patterns
    (1, 5, "sphere", _KS + 1, "cubic", 0, "unit", False, False),          # N = 1 across two tiles of vectors
    (_CH - 1, 3, "corners", 8, "cubic", 40, "sqrt_mass", True, True),
    (_CH, 5, "mixed", 2, "triclinic", 40, "signed", False, True),         # one full chain = one full atom tile
    (_CH + 1, 4, "sphere", _KS - 1, "triclinic", 0, "unit", False, False),
    (("tile", -1), 1, "sphere", _KS, "cubic", 0, "signed", False, True),
    (("tile", 0), 3, "sphere", _KS, "triclinic", 40, "unit", True, True),
    (("tile", 1), 1, "sphere", 2 * _KS, "triclinic", 40, "sqrt_mass", False, True),
    (3 * _CH + 7, 3, "corners", 8, "triclinic", 40, "unit", True, True),  # several tiles, four folds
    (("tiles", 5), 4, "halfsphere", 0, "cubic", 40, "sqrt_mass", True, False),  # the full half-sphere of a small q_max
]


def _case_id(c):
    n = c[0] if isinstance(c[0], int) else f"{c[0][0]}{c[0][1]:+d}"
    return f"n{n}_T{c[1]}_{c[2]}{c[3]}_{c[4]}_s{c[5]}_{c[6]}_{'idx' if c[7] else 'all'}_{'j' if c[8] else 'rho'}"


@pytest.mark.parametrize("case", BOUND_CASES, ids=[_case_id(c) for c in BOUND_CASES])
def test_projection_within_bound_same_bits_any_blocking(engine, case):
    from psa_amd import _hip
    n, T, kind, K, box_name, shift, wk, listed, currents = case
    box = BOXES[box_name]
    inv = C.inverse(box)
    ind = _index_set(kind, K, box)
    K = K or ind.shape[0]
    assert ind.shape == (K, 3) and K >= 1
    if not isinstance(n, int):
        A = _tile_atoms(ind)
        n = A + n[1] if n[0] == "tile" else 2 * A + n[1]
    n_all = n + 5 if listed else n
    pos, vel = C.trajectory(n_all, T, seed=n + K, box=box, shift=shift)
    w = C.weights(wk, n_all, seed=2)
    idx = np.random.default_rng(3).permutation(n_all)[:n].astype(np.int32) if listed else None
    reach = C.max_abs_phase(pos, ind, inv, idx)
    if shift:                                                              # an unwrapped trajectory: 1e3 rad and more
        assert reach >= (3e4 if kind == "corners" else 1e3)
    else:
        assert reach <= 2 * np.pi * 3 * 1.5 * float(np.max(np.abs(ind))) + 1.0
    _resident(engine, pos, vel)
    engine.set_atom_weights(w)
    got = engine.debug_lattice_project(inv, ind, idx, currents)
    ref, absum = L64.project64(pos, vel, ind, inv, idx, w, currents, with_abs=True)
    assert got.shape == ref.shape == (K, 4 if currents else 1, T)
    lim = C.bound(absum, n)[None]
    frac = np.abs(got.astype(np.complex128) - ref) / lim
    worst = np.unravel_index(np.argmax(frac), frac.shape)
    print(f"{n} atoms, {K} vectors, largest |k.r| {reach:.3e} rad: worst element {worst} at {frac[worst]:.4f} of its bound "
          f"({lim[0][worst[1:]]:.3e})")
    assert frac.max() <= 1.0
    if kind == "mixed" and K >= 2:
        assert np.all(got[1].imag == 0)                                   # n = 0: every factor is (1, 0) exactly
    again = engine.debug_lattice_project(inv, ind, idx, currents)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))      # two identical calls: the same bits
    if K >= 2:                                                             # ... and so a call cut into blocks of vectors
        per_k = (4 if currents else 1) * T * 8
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, per_k * max(1, K // 3))
        blocked = engine.debug_lattice_project(inv, ind, idx, currents)
        assert np.array_equal(got.view(np.uint32), blocked.view(np.uint32))


# ---- against the kernel of psa_dynamic_spectra ---------------------------------------------------------------------------
@pytest.mark.parametrize("box_name", list(BOXES))
def test_agrees_with_the_dynamic_kernel_on_rounded_vectors(engine, box_name):
    """debug_dynamic_project on float32(n.G) against debug_lattice_project on n, positions inside the box.  The two differ
    by definition -- the rounded k is not the commensurate one --, so the allowance is the sum of both bounds plus the
    distance of the two float64 references (the allowance of test_gpu_dynamic's frozen-positions test)."""
    box = BOXES[box_name]
    inv = C.inverse(box)
    n, T = 130, 6
    ind = _sphere(box, 150)
    pos, vel = C.trajectory(n, T, seed=9, box=box)
    k32 = L64.lattice_k(ind, inv).astype(np.float32)
    _resident(engine, pos, vel)
    q_lat = engine.debug_lattice_project(inv, ind, None, True).astype(np.complex128)
    q_dyn = engine.debug_dynamic_project(k32, None, True).astype(np.complex128)
    ref_lat, absum = L64.project64(pos, vel, ind, inv, None, None, True, with_abs=True)
    ref_dyn = dynamic64.project64(pos, vel, k32, None, None, True)
    bounds = C.bound(absum, n)[None] + dynamic_cases.bound(absum, n)[None]
    definitional = np.abs(ref_lat - ref_dyn)
    frac = np.abs(q_lat - q_dyn) / (bounds + definitional)
    print(f"{box_name}: definitional term over the sum of both bounds: largest {np.max(definitional / bounds):.3f}; lattice "
          f"against dynamic kernel: worst element at {frac.max():.4f} of the allowance, rel_max {rel_max(q_lat, q_dyn):.2e}")
    assert frac.max() <= 1.0
    assert rel_max(q_lat, q_dyn) < 1e-5


# ---- the calculator --------------------------------------------------------------------------------------------------------
def _calculator(engine, pos, vel, box, dt=0.002, cells=(1, 1, 1)):
    from psa_amd import SEDCalculator, Trajectory
    T, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, vel, np.ones(n, np.int32), np.arange(T, dtype=np.float32), box, np.diag(box).copy(),
                    np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, *cells).attach(engine=engine)


def test_perfect_crystal_bragg_peaks(engine):
    """a simple cubic lattice of c^3 sites in a box of side c a, static, unit weights: bin 0 of the density is N^2 where
    every n_j is a multiple of c, and within the projection's bound of 0 elsewhere"""
    c, a, T = 4, 1.5, 8
    box = np.diag([c * a] * 3).astype(np.float32)
    R = (a * np.stack(np.meshgrid(*[np.arange(c)] * 3, indexing="ij"), -1).reshape(-1, 3)).astype(np.float32)
    N = c ** 3
    pos = np.ascontiguousarray(np.broadcast_to(R, (T, N, 3)))
    vel = np.zeros_like(pos)
    ind = np.stack(np.meshgrid(*[np.arange(-5, 6)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    out = _calculator(engine, pos, vel, box).calculate_lattice_spectra(ind, currents=False)
    bragg = np.all(ind % c == 0, axis=1)
    lim = float(C.bound(N, N))                                             # on |q|: sum |w| = N
    d0 = out.density[0].astype(np.float64)
    print(f"{bragg.sum()} Bragg vectors of {ind.shape[0]}: N^2 = {N * N}, largest deviation {np.max(np.abs(d0[bragg] - N * N)):.3e} "
          f"(allowed {2 * N * lim + lim * lim + N * N * 2.0 ** -23:.3e}); largest value elsewhere {d0[~bragg].max():.3e} "
          f"(allowed {lim * lim * (1 + 2.0 ** -22):.3e})")
    assert bragg.sum() == 27
    assert np.all(np.abs(d0[bragg] - N * N) <= 2 * N * lim + lim * lim + N * N * 2.0 ** -23)
    assert np.all(d0[~bragg] <= lim * lim * (1 + 2.0 ** -22))
    assert np.all(out.density[1:] <= lim * lim * (1 + 2.0 ** -22))         # static: nothing off bin 0
    np.testing.assert_allclose(out.k_vectors, L64.lattice_k(ind, C.inverse(box)), rtol=0, atol=1e-13)


EDGES = np.array([0.05, 0.2, 0.45, 0.65, 0.85, 1.0, 1.15])                # the first shell lies below the shortest vector
SEGMENTS = {"none": None, "hann_64_32": (64, 32, "hann"), "boxcar_64_64": (64, 64, "boxcar")}


@pytest.fixture(scope="module", params=list(BOXES))
def wave(request):
    """T = 256, N = 130, the half-space of |k| < 1.15 in 6 shells of which the first is empty, a travelling wave on one of
    its vectors; the float64 projections of the explicit full sphere, once for every segment shape"""
    from psa_amd import commensurate_vectors, shell_bins
    box = BOXES[request.param]
    inv = C.inverse(box)
    half, _, q = commensurate_vectors(box, EDGES[-1], EDGES[0])
    b, sel, avail, used = shell_bins(q, EDGES)
    half, b, q = half[sel], b[sel], q[sel]
    assert 100 <= half.shape[0] <= 300 and avail[0] == 0 and np.all(avail[1:] > 0)
    k0 = half[np.flatnonzero(b == 2)[3]]
    pos, vel = C.travelling_wave(130, 256, box, k0, bin0=20)
    w = C.weights("sqrt_mass", 130, seed=23)
    full, b_full = np.concatenate([half, -half]), np.concatenate([b, b])
    return dict(box=box, inv=inv, half=half, bins=b, q=q, avail=avail, pos=pos, vel=vel, w=w, full=full, b_full=b_full,
                q_full=L64.project64(pos, vel, full, inv, None, w, True))


def _window(s):
    return (None, None, None) if s is None else (s.window_array(), s.length, s.hop)


@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_calculators_parity_float64_on_the_full_sphere(engine, wave, seg):
    from psa_amd import DynamicSpectra, PowderSpectra, Segments
    s = None if SEGMENTS[seg] is None else Segments(*SEGMENTS[seg])
    L = 256 if s is None else s.length
    calc = _calculator(engine, wave["pos"], wave["vel"], wave["box"])
    per64 = L64.spectra64(wave["q_full"], wave["full"], wave["inv"], *_window(s))
    # per vector, the explicit full sphere
    per = calc.calculate_lattice_spectra(wave["full"], atom_weights=wave["w"], segments=s)
    assert isinstance(per, DynamicSpectra) and per.density.shape == (L, wave["full"].shape[0]) and per.density.dtype == np.float32
    np.testing.assert_allclose(per.k_vectors, L64.lattice_k(wave["full"], wave["inv"]), rtol=0, atol=1e-13)
    errs = {f"vector {name}": rel_max(got, ref) for name, got, ref in zip(("density", "longitudinal", "transverse"),
                                                                         (per.density, per.longitudinal, per.transverse), per64)}
    # the powder average against the mean over the explicit full sphere, nothing folded
    pw = calc.calculate_powder_spectra(EDGES, atom_weights=wave["w"], segments=s)
    ref = L64.shell_mean64(per64, wave["b_full"], 6)
    assert isinstance(pw, PowderSpectra) and pw.density.shape == (L, 6) and pw.density.dtype == np.float32
    for name, got, want in zip(("density", "longitudinal", "transverse"), (pw.density, pw.longitudinal, pw.transverse), ref):
        errs[f"powder {name}"] = rel_max(got, want)
    print(f"{seg}: {errs}")
    assert max(errs.values()) <= 1e-5
    assert not pw.density[:, 0].any() and not pw.longitudinal[:, 0].any() and not pw.transverse[:, 0].any()    # the empty shell
    np.testing.assert_array_equal(pw.counts, 2 * np.bincount(wave["bins"], minlength=6))
    np.testing.assert_array_equal(pw.available, 2 * wave["avail"])
    assert np.isnan(pw.q[0])
    np.testing.assert_allclose(pw.q[1:], [wave["q"][wave["bins"] == i].mean() for i in range(1, 6)], rtol=1e-14)
    assert np.array_equal(pw.indices, wave["half"]) and np.array_equal(pw.bin_index, wave["bins"])
    np.testing.assert_allclose(pw.freqs, np.fft.fftfreq(L, 0.002))
    assert pw.weight_norm == pytest.approx(float(np.sum(wave["w"].astype(np.float64) ** 2)))
    # the shell form against the per-vector form averaged on the host in float64
    host = L64.shell_mean64([x.astype(np.float64) for x in (per.density, per.longitudinal, per.transverse)], wave["b_full"], 6)
    shell = {name: rel_max(got, want) for name, got, want in zip(("density", "longitudinal", "transverse"),
                                                                (pw.density, pw.longitudinal, pw.transverse), host)}
    print(f"{seg}: shell form against per-vector form: {shell}")
    assert max(shell.values()) <= 1e-6


def test_max_per_bin_blockings_repeat(engine, wave):
    from psa_amd import Segments, _hip
    s = Segments(64, 32, "hann")
    calc = _calculator(engine, wave["pos"], wave["vel"], wave["box"])
    pw = calc.calculate_powder_spectra(EDGES, atom_weights=wave["w"], segments=s, max_per_bin=9, seed=3)
    np.testing.assert_array_equal(pw.counts, 2 * np.minimum(wave["avail"], 9))
    np.testing.assert_array_equal(pw.available, 2 * wave["avail"])
    assert pw.indices.shape[0] == int(np.minimum(wave["avail"], 9).sum())
    full, b_full = np.concatenate([pw.indices, -pw.indices]), np.concatenate([pw.bin_index, pw.bin_index])
    ref = L64.powder64(wave["pos"], wave["vel"], full, wave["inv"], b_full, 6, None, wave["w"], True, *_window(s))
    errs = {name: rel_max(got, want) for name, got, want in zip(("density", "longitudinal", "transverse"),
                                                               (pw.density, pw.longitudinal, pw.transverse), ref)}
    print(f"max_per_bin = 9: {errs}")
    assert max(errs.values()) <= 1e-5
    other = calc.calculate_powder_spectra(EDGES, atom_weights=wave["w"], segments=s, max_per_bin=9, seed=4)
    assert not np.array_equal(other.indices, pw.indices)
    # the engine: a repeat gives the same bits; two blockings of the vectors and the segments agree to one float32 ulp
    _resident(engine, wave["pos"], wave["vel"])
    engine.set_atom_weights(wave["w"])
    engine.set_segments(s)
    one = engine.lattice_spectra(wave["inv"], wave["half"], wave["bins"], 6, None, True)
    again = engine.lattice_spectra(wave["inv"], wave["half"], wave["bins"], 6, None, True)
    assert np.array_equal(one.view(np.uint32), again.view(np.uint32))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 * 8 * (37 * 256 + 50 * 64))       # 37 vectors of q, 50 (vector, segment) units
    cut = engine.lattice_spectra(wave["inv"], wave["half"], wave["bins"], 6, None, True)
    ulp = np.spacing(np.maximum(np.abs(one), np.abs(cut)))
    print(f"two blockings: largest difference {np.max(np.abs(one - cut) / ulp):.2f} ulp, {np.count_nonzero(one != cut)} of {one.size} differ")
    assert np.all(np.abs(one - cut) <= ulp)
    per_one = engine.lattice_spectra(wave["inv"], wave["half"], None, 0, None, True)
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
    per_all = engine.lattice_spectra(wave["inv"], wave["half"], None, 0, None, True)
    assert max(rel_max(per_one[i], per_all[i]) for i in range(3)) <= 2e-6  # later sub-blocks add in float32, as for the dynamic spectra
    # an atom subset; an empty set gives zeros
    idx = np.random.default_rng(5).permutation(130)[:77].astype(np.int32)
    sub = engine.lattice_spectra(wave["inv"], wave["half"], wave["bins"], 6, idx, True)
    ref = L64.powder64(wave["pos"], wave["vel"], wave["full"], wave["inv"], wave["b_full"], 6, idx, wave["w"], True, *_window(s))
    assert max(rel_max(sub[i], ref[i]) for i in range(3)) <= 1e-5
    assert not engine.lattice_spectra(wave["inv"], wave["half"], wave["bins"], 6, np.zeros(0, np.int32), True).any()
    assert not engine.debug_lattice_project(wave["inv"], wave["half"], np.zeros(0, np.int32), False).any()


# ---- refusals, and no trace ---------------------------------------------------------------------------------------------------
def test_refusals(engine, wave):
    from psa_amd import Segments, _hip
    pos, vel, inv = wave["pos"], wave["vel"], np.ascontiguousarray(wave["inv"])
    _resident(engine, pos, vel)
    lib, h = engine._lib, engine._h
    f32p, i32p, f64p = Ct.POINTER(Ct.c_float), Ct.POINTER(Ct.c_int32), Ct.POINTER(Ct.c_double)
    ind = np.ascontiguousarray(wave["half"][:9])
    bins = np.ascontiguousarray(wave["bins"][:9])
    out, sh = np.empty((3, 256, 9), np.float32), np.empty((3, 256, 6), np.float32)
    bp, ip, op, sp = inv.ctypes.data_as(f64p), ind.ctypes.data_as(i32p), out.ctypes.data_as(f32p), sh.ctypes.data_as(f32p)
    binp = bins.ctypes.data_as(i32p)

    def refused(rc, word):
        msg = lib.psa_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    assert lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 1, op, out.nbytes) == 0
    assert lib.psa_lattice_spectra(h, bp, ip, 9, binp, 6, None, 0, 1, sp, sh.nbytes) == 0
    refused(lib.psa_lattice_spectra(h, None, ip, 9, None, 0, None, 0, 1, op, out.nbytes), "null")
    refused(lib.psa_lattice_spectra(h, bp, None, 9, None, 0, None, 0, 1, op, out.nbytes), "null")
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 1, None, out.nbytes), "null")
    refused(lib.psa_debug_lattice_project(h, bp, ip, 9, None, 0, 1, None), "null")
    refused(lib.psa_lattice_spectra(h, bp, ip, 0, None, 0, None, 0, 1, op, out.nbytes), "at least one")
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 1, op, out.nbytes - 4), "out_bytes")
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, binp, 6, None, 0, 1, op, out.nbytes), "out_bytes")     # the shell form is (3, L, n_bins)
    for bad_inv, word in ((np.full(9, np.nan), "finite"), (np.zeros(9), "singular"), (np.ones(9), "singular")):
        refused(lib.psa_lattice_spectra(h, bad_inv.ctypes.data_as(f64p), ip, 9, None, 0, None, 0, 1, op, out.nbytes), word)
    far = ind.copy()
    far[4, 1] = -_hip.LAT_MAX_INDEX - 1
    refused(lib.psa_lattice_spectra(h, bp, far.ctypes.data_as(i32p), 9, None, 0, None, 0, 1, op, out.nbytes), "is served")
    for bad_bin in (-1, 6):
        bb = bins.copy()
        bb[2] = bad_bin
        refused(lib.psa_lattice_spectra(h, bp, ip, 9, bb.ctypes.data_as(i32p), 6, None, 0, 1, sp, sh.nbytes), "outside")
    for bad_n in ((0, 0, 0), (0, -1, 2), (-1, 2, 2)):
        nn = ind.copy()
        nn[7] = bad_n
        refused(lib.psa_lattice_spectra(h, bp, nn.ctypes.data_as(i32p), 9, binp, 6, None, 0, 1, sp, sh.nbytes), "half-space")
        assert lib.psa_lattice_spectra(h, bp, nn.ctypes.data_as(i32p), 9, None, 0, None, 0, 1, op, out.nbytes) == 0   # per vector: allowed
    bad = np.array([3, 130], np.int32)
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, bad.ctypes.data_as(i32p), 2, 1, op, out.nbytes), "out of bounds")
    engine.set_atom_weights(np.ones(129, np.float32))
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 1, op, out.nbytes), "weights")
    engine.set_atom_weights(None)
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 * 8 * 256 - 1)
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 1, op, out.nbytes), "budget")
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
    engine.set_segments(Segments(512, 256, "hann"))
    big = np.empty((3, 512, 9), np.float32)
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 1, big.ctypes.data_as(f32p), big.nbytes), "segment length")
    engine.set_segments(None)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, np.ascontiguousarray(vel[:128]))
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 1, op, out.nbytes), "shape")
    engine.release(_hip.SLOT_VELOCITIES)
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 1, op, out.nbytes), "velocities")
    one = np.empty((1, 256, 9), np.float32)
    assert lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 0, one.ctypes.data_as(f32p), one.nbytes) == 0   # the density needs none
    engine.release(_hip.SLOT_POSITIONS)
    refused(lib.psa_lattice_spectra(h, bp, ip, 9, None, 0, None, 0, 0, one.ctypes.data_as(f32p), one.nbytes), "positions")


def test_no_trace_in_the_other_entry_points(engine, wave):
    """an ordinary `calculate` and a `calculate_dynamic_spectra` give the bits they gave before the lattice calls in between"""
    from psa_amd import Segments
    calc = _calculator(engine, wave["pos"], wave["vel"], wave["box"], cells=(4, 4, 4))
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    for _ in range(2):                      # (the first call uploads and projects at once, the next builds what is cached)
        calc.calculate(mags, vecs)
    k = dynamic_cases.k_list(9, seed=22)
    s = Segments(64, 32, "hann")
    before = calc.calculate(mags, vecs)
    dyn_before = calc.calculate_dynamic_spectra(np.linalg.norm(k, axis=1), k, segments=s, atom_weights=wave["w"])
    calc.calculate_powder_spectra(EDGES, segments=s, atom_weights=wave["w"])
    calc.calculate_lattice_spectra(wave["half"][:20], currents=False)
    after = calc.calculate(mags, vecs)
    dyn_after = calc.calculate_dynamic_spectra(np.linalg.norm(k, axis=1), k, segments=s, atom_weights=wave["w"])
    assert np.array_equal(before.sed.view(np.uint32), after.sed.view(np.uint32))
    for name in ("density", "longitudinal", "transverse"):
        assert np.array_equal(getattr(dyn_before, name).view(np.uint32), getattr(dyn_after, name).view(np.uint32)), name
    engine.timings()                                                       # (reset)
    calc.calculate_powder_spectra(EDGES)
    timings = engine.timings()
    assert timings["project"] > 0 and timings["fft"] > 0 and timings["epilogue"] > 0 and timings["d2h"] > 0
