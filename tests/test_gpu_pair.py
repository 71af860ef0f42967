"""The pair distributions on the GPU (psa_pair_histogram, psa_debug_pair_fractions and the two calculator methods) against
the brute-force float64 reference of tests/pair64.py inside the allowance of tests/pair_cases.py: the fractions per
element; the counts for one, two and three species at every edge of the atom tile, of the lags and of the origin step,
at 1, 64 and 1024 bins, at the served radius and at a tenth of it; exact totals and exact symmetry at lag 0; the input
families; permutations, work budgets and repeated calls bit for bit; a simple-cubic lattice's 6, 12, 8; the calculator
methods; every refusal (a context with a communicator among them); no trace in later calls.

Every counts test first asserts the reference's borderline share under the cap, then prints how many counts moved."""
import ctypes as Ct
import functools

import numpy as np
import pytest

import pair64 as R
import pair_cases as P
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = {"cubic": P.CUBIC, "triclinic": P.TRICLINIC}
TILE = P.TILE


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


def _served(box):
    from psa_amd import max_pair_radius
    return max_pair_radius(BOXES[box] if isinstance(box, str) else box)


@functools.lru_cache(maxsize=None)
def _walk(box, n_atoms, n_frames, seed=11):
    return P.walk(n_atoms, n_frames, seed, box=BOXES[box])


def _listing(kind, n_atoms, seed=3):
    """the species for the engine (None: all atoms as one)"""
    if kind == "one":
        return None
    if kind == "two":                                                      # the last 40 atoms (of few: the last third) and the rest
        cut = n_atoms - (40 if n_atoms > 100 else n_atoms // 3)
        return [np.arange(0, cut, dtype=np.int32), np.arange(cut, n_atoms, dtype=np.int32)]
    order = np.random.default_rng(seed).permutation(n_atoms).astype(np.int32)
    return [order[: n_atoms // 3], np.zeros(0, np.int32), order[n_atoms // 3: max(n_atoms - 2, n_atoms // 3)]]


def _groups(listing, n_atoms):
    return [np.arange(n_atoms)] if listing is None else listing


@functools.lru_cache(maxsize=None)
def _reference(box, family, n_atoms, n_frames, kind, lags, step, n_r, fraction=1.0):
    """(dr, counts, allowed, borderline, total), computed once per case and shared"""
    dr = fraction * _served(box) / n_r
    groups = _groups(_listing(kind, n_atoms), n_atoms)
    return (dr,) + P.reference(_walk(box, n_atoms, n_frames)[family], BOXES[box], groups, list(lags), step, dr, n_r)


def _check(got, ref, allowed, borderline, total, n_r, totals, what):
    assert borderline <= P.cap(n_r) * max(total, 1), what                   # the borderline condition, before anything else
    assert got.dtype == np.uint64 and got.shape == ref.shape
    got = got.astype(np.int64)
    print(f"{what}: {borderline} borderline of {total}, {int(np.abs(got - ref).sum())} counts moved")
    assert np.array_equal(got.sum(axis=3), totals), what                    # exact totals
    assert np.all(np.abs(got - ref) <= allowed), what


def _run(engine, box, family, n_atoms, n_frames, kind, lags, step=1, n_r=64, fraction=1.0):
    dr, ref, allowed, borderline, total = _reference(box, family, n_atoms, n_frames, kind, tuple(lags), step, n_r, fraction)
    listing = _listing(kind, n_atoms)
    _resident(engine, _walk(box, n_atoms, n_frames)[family])
    got = engine.pair_histogram(BOXES[box], lags, dr, n_r, listing, origin_step=step)
    totals = P.expected_totals(n_frames, _groups(listing, n_atoms), lags, step)
    _check(got, ref, allowed, borderline, total, n_r, totals, f"{box} {family} N {n_atoms} T {n_frames} {kind} step {step} n_r {n_r} x{fraction}")
    for j, lag in enumerate(lags):
        if lag == 0:
            assert np.array_equal(got[j], got[j].transpose(1, 0, 2))       # tau = 0: (a, b) = (b, a) bit for bit
    return got


# ---- the fractions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["wrapped", "shifted"])
@pytest.mark.parametrize("box", BOXES)
def test_fractions(engine, box, family):
    """|c - c64| <= 2^-26 (the float32 rounding of a value of at most 0.5) + 4 2^-53 sum_c |r_c| |Hinv_cj| (the float64
    chain's three roundings and the subtraction), compared modulo 1: c enters the pair kernel through e - rint(e) alone"""
    pos = _walk(box, 37, 20)[family]
    _resident(engine, pos)
    ref = R.fractions64(pos, BOXES[box])
    bound = 2.0 ** -26 + 4.0 * 2.0 ** -53 * (np.abs(pos.astype(np.float64)) @ np.abs(R.box64(BOXES[box])[1]))
    for idx in (None, np.random.default_rng(2).permutation(37)[:20].astype(np.int32)):
        c = engine.debug_pair_fractions(BOXES[box], idx)
        want, lim = (ref, bound) if idx is None else (ref[:, idx], bound[:, idx])
        assert c.dtype == np.float32 and c.shape == want.shape and np.all(np.abs(c) <= 0.5)
        d = c.astype(np.float64) - want
        d -= np.rint(d)
        print(f"fractions {box} {family}: worst fraction of the bound {np.max(np.abs(d) / lim):.3f}")
        assert np.all(np.abs(d) <= lim)


# ---- counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [1, 2, 37, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
@pytest.mark.parametrize("box", BOXES)
def test_counts_one_species(engine, box, n_atoms):
    n_frames, step = (6, 3) if n_atoms > 100 else (20, 1)                   # (the brute force stays quick)
    got = _run(engine, box, "wrapped", n_atoms, n_frames, "one", [0, 1, n_frames - 1], step=step)
    if n_atoms == 1:
        assert not got.any()                                               # one atom against itself: zeros


@pytest.mark.parametrize("box,n_atoms,kind", [("cubic", 37, "two"), ("triclinic", 37, "two"), ("cubic", 37, "three"), ("triclinic", 37, "three"),
                                              ("triclinic", TILE + 39, "two"), ("cubic", TILE + 41, "two"),
                                              ("triclinic", 2 * TILE + 43, "two"), ("cubic", 2 * TILE + 3, "three"),
                                              ("cubic", 2, "two"), ("triclinic", 2, "three")])
def test_counts_species(engine, box, n_atoms, kind):
    """two species: 40 atoms against TILE - 1, TILE + 1 and 2 TILE + 3; "three": an empty species between two shuffled ones,
    171 and 342 atoms at 2 TILE + 3"""
    n_frames, step = (6, 3) if n_atoms > 100 else (20, 1)
    got = _run(engine, box, "wrapped", n_atoms, n_frames, kind, [0, 1, n_frames - 1], step=step)
    if kind == "three":
        assert not got[:, 1].any() and not got[:, :, 1].any()
    if n_atoms > 2:
        assert not np.array_equal(got[1], got[1].transpose(1, 0, 2))       # tau > 0: the two orders differ


@pytest.mark.parametrize("step", [1, 3, 50])
def test_origin_steps(engine, step):
    _run(engine, "triclinic", "wrapped", 37, 40, "three", [0, 1, 39], step=step)


@pytest.mark.parametrize("fraction", [1.0, 0.1])
@pytest.mark.parametrize("n_r", [1, 64, 1024])
@pytest.mark.parametrize("box", BOXES)
def test_bins_and_radius(engine, box, n_r, fraction):
    _run(engine, box, "wrapped", 130, 10, "two", [0, 3], n_r=n_r, fraction=fraction)


@pytest.mark.parametrize("family", ["unwrapped", "shifted"])
@pytest.mark.parametrize("box", BOXES)
def test_families(engine, box, family):
    """every family against the reference of its own float32 positions; "shifted" is 1000 box vectors from the origin"""
    _run(engine, box, family, 130, 10, "two", [0, 3])


@pytest.mark.parametrize("box", BOXES)
def test_frozen(engine, box):
    n, T = 40, 7
    pos = P.frozen(n, T, seed=4, box=BOXES[box])
    groups = [np.arange(n)]
    dr = _served(box) / 64
    ref, allowed, borderline, total = P.reference(pos[:1], BOXES[box], groups, [0], 1, dr, 64)
    _resident(engine, pos)
    got = engine.pair_histogram(BOXES[box], [0, 2, 6], dr, 64)
    n_o = np.array([7, 5, 1])
    _check(got, ref * n_o[:, None, None, None], allowed * n_o[:, None, None, None], borderline, total, 64,
           P.expected_totals(T, groups, [0, 2, 6], 1), f"frozen {box}")
    assert np.array_equal(got[1] * 7, got[0] * 5)                           # every origin and lag: the same frame


@pytest.mark.parametrize("box", BOXES)
def test_wrapped_against_unwrapped_and_moved(engine, box):
    """the unwrapped trajectory, and the one moved by whole box vectors per atom, inside the allowance of the WRAPPED
    input's reference widened by what the float32 rounding of the other input's positions moves a pair distance by:
    two positions, 2^-24 of the largest coordinate per axis each"""
    n, T, lags, n_r = 130, 10, [0, 3], 64
    w = _walk(box, n, T)
    groups = _groups(_listing("two", n), n)
    dr = _served(box) / n_r
    for family in ("unwrapped", "moved"):
        extra = 2.0 * np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(w[family]).max())
        ref, allowed, borderline, total = P.reference(w["wrapped"], BOXES[box], groups, lags, 1, dr, n_r, extra=extra)
        _resident(engine, w[family])
        got = engine.pair_histogram(BOXES[box], lags, dr, n_r, _listing("two", n))
        _check(got, ref, allowed, borderline, total, n_r, P.expected_totals(T, groups, lags, 1), f"{family} against wrapped, {box}")


# ---- bit for bit ----------------------------------------------------------------------------------------------------------
def test_permutations_budgets_and_repeats(engine):
    from psa_amd import _hip
    n, T, lags = 2 * TILE + 3, 6, [0, 2]
    pos = _walk("triclinic", n, T)["wrapped"]
    _resident(engine, pos)
    listing = _listing("two", n)
    dr = _served("triclinic") / 64
    whole = engine.pair_histogram(P.TRICLINIC, lags, dr, 64, listing, origin_step=1)
    assert np.array_equal(whole, engine.pair_histogram(P.TRICLINIC, lags, dr, 64, listing))
    rng = np.random.default_rng(8)
    assert np.array_equal(whole, engine.pair_histogram(P.TRICLINIC, lags, dr, 64, [rng.permutation(g) for g in listing]))
    for origins in (1, 2, 4):                                              # origins per block
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * n * origins + 5)
        assert np.array_equal(whole, engine.pair_histogram(P.TRICLINIC, lags, dr, 64, listing))
    # one species of all atoms is the sum over the two
    reset(engine)
    one = engine.pair_histogram(P.TRICLINIC, lags, dr, 64)
    assert np.array_equal(one[:, 0, 0], whole.sum(axis=(1, 2)))


# ---- workgroups that loop: runs of beta-tiles, slabs of several origins ------------------------------------------------------
def test_runs_of_beta_tiles(engine):
    """128 tiles and 77 atoms: the host's table gives an item a run of 2 beta-tiles at lag 0 (upper triangle, the diagonal
    tile first in its run, the last run clipped) and of 4 at lag 1, and both origins of a lag to one workgroup.  No
    reference over N^2: exact totals, lag-0 symmetry, one species against the sum over two (another table: other runs,
    other tiles), two budgets and a permuted list bit for bit, and a sparse check of the first bins by brute force"""
    from psa_amd import _hip
    n, T, lags, n_r = 128 * TILE + 77, 2, [0, 1], 8
    assert _hip.Engine.debug_pair_plan([n], True, 2)["run"] == 2 and _hip.Engine.debug_pair_plan([n], False, 1)["run"] == 4
    sizes = [79 * TILE - 9, n - (79 * TILE - 9)]
    assert _hip.Engine.debug_pair_plan(sizes, True, 2)["run"] >= 2 and _hip.Engine.debug_pair_plan(sizes, True, 2)["slabs"] == 1
    pos = _walk("triclinic", n, T, seed=12)["wrapped"]
    _resident(engine, pos)
    dr = _served("triclinic") / n_r
    one = engine.pair_histogram(P.TRICLINIC, lags, dr, n_r).astype(np.int64)
    assert np.array_equal(one.sum(axis=3), P.expected_totals(T, [np.arange(n)], lags, 1))
    order = np.random.default_rng(5).permutation(n).astype(np.int32)
    listing = [order[: sizes[0]], order[sizes[0]:]]
    two = engine.pair_histogram(P.TRICLINIC, lags, dr, n_r, listing)
    assert np.array_equal(two.astype(np.int64).sum(axis=3), P.expected_totals(T, listing, lags, 1))
    assert np.array_equal(two[0], two[0].transpose(1, 0, 2)) and not np.array_equal(two[1], two[1].transpose(1, 0, 2))
    assert np.array_equal(two.astype(np.int64).sum(axis=(1, 2)), one[:, 0, 0])
    rng = np.random.default_rng(6)
    assert np.array_equal(two, engine.pair_histogram(P.TRICLINIC, lags, dr, n_r, [rng.permutation(g) for g in listing]))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * n + 3)             # one origin per block
    assert np.array_equal(two, engine.pair_histogram(P.TRICLINIC, lags, dr, n_r, listing))
    # the atoms within the first bin of 300 alpha-atoms spread over all tiles, by the brute force, against a call of those
    # 300 as one species and the rest as another (alpha-tiles of 256 and 44 against runs over every beta-tile)
    pick = np.sort(order[:300])
    rest = np.setdiff1d(np.arange(n), pick).astype(np.int32)
    got = engine.pair_histogram(P.TRICLINIC, [1], dr, n_r, [pick.astype(np.int32), rest]).astype(np.int64)
    reset(engine)
    ref, allowed, borderline, total = P.reference(pos, P.TRICLINIC, [pick, rest[::40]], [1], 1, dr, n_r)
    sub = engine.pair_histogram(P.TRICLINIC, [1], dr, n_r, [pick.astype(np.int32), rest[::40]]).astype(np.int64)
    assert borderline <= P.cap(n_r) * total and np.all(np.abs(sub - ref) <= allowed)
    assert np.array_equal(got[0, 0, 0], sub[0, 0, 0]) and np.all(got[0, 0, 1] >= sub[0, 0, 1])


@pytest.mark.parametrize("box", BOXES)
def test_slabs_of_several_origins(engine, box):
    """515 frozen atoms over 1000 frames: 6 tile pairs at lag 0 and 9 at the others, so the table cuts the origins into
    682 and 455 slabs and a workgroup takes two or three origins, a stride apart; against n_o times the one-frame
    reference, as test_frozen"""
    from psa_amd import _hip
    n, T, lags, n_r = 2 * TILE + 3, 1000, [0, 2, 600], 64
    assert _hip.Engine.debug_pair_plan([n], True, 1000)["slabs"] == 682 and _hip.Engine.debug_pair_plan([n], False, 998)["slabs"] == 455
    pos = P.frozen(n, T, seed=9, box=BOXES[box])
    groups = [np.arange(n)]
    dr = _served(box) / n_r
    ref, allowed, borderline, total = P.reference(pos[:1], BOXES[box], groups, [0], 1, dr, n_r)
    _resident(engine, pos)
    got = engine.pair_histogram(BOXES[box], lags, dr, n_r)
    n_o = np.array([1000, 998, 400])
    _check(got, ref * n_o[:, None, None, None], allowed * n_o[:, None, None, None], borderline, total, n_r,
           P.expected_totals(T, groups, lags, 1), f"slabs of several origins, {box}")
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * n * 300 + 1)       # blocks of 300 origins: 300 slabs where there were 682
    assert np.array_equal(got, engine.pair_histogram(BOXES[box], lags, dr, n_r))


# ---- a lattice ----# ---- a lattice ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", P.LATTICE_BOXES)
def test_simple_cubic_shells(engine, box):
    """4 x 4 x 4 simple cubic, a = 5.43: 6 neighbours at a, 12 at sqrt(2) a, 8 at sqrt(3) a; bins of 0.65 put the shells at
    x = 8.35, 11.81 and 14.47, away from every edge, and r_max = 10.4 below 2 a"""
    H = P.LATTICE_BOXES[box]
    pos, a = P.simple_cubic(5, box)
    n_r, dr = 16, 0.65
    assert n_r * dr <= _served(H) and n_r * dr < 2 * a
    _resident(engine, pos)
    got = engine.pair_histogram(H, [0, 2], dr, n_r).astype(np.int64)
    shells = {int(np.floor(a / dr)): 6, int(np.floor(np.sqrt(2.0) * a / dr)): 12, int(np.floor(np.sqrt(3.0) * a / dr)): 8}
    assert sorted(shells) == [8, 11, 14]
    for j, n_o in enumerate((5, 3)):
        per_atom = got[j, 0, 0, :n_r] / (64.0 * n_o)
        want = np.zeros(n_r)
        for k, z in shells.items():
            want[k] = z
        assert np.array_equal(per_atom, want)
        assert got[j, 0, 0, n_r] == 64 * n_o * (63 - 26)


# ---- the calculator -------------------------------------------------------------------------------------------------------
def _calculator(engine, pos, box, types=None, dt=0.002):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, 1, 1, 1).attach(engine=engine)


def test_calculator_methods_and_draws(engine):
    from psa_amd import RadialDistribution, VanHoveDistinct, draw_atoms, max_pair_radius
    n, T = 130, 10
    pos = _walk("triclinic", n, T)["wrapped"]
    types = (np.arange(n) % 3 + 1).astype(np.int32)
    calc = _calculator(engine, pos, P.TRICLINIC, types)
    want = [draw_atoms(np.flatnonzero(types == s), 30, 5) for s in (1, 3)]
    served = max_pair_radius(P.TRICLINIC)
    rd = calc.calculate_rdf(n_r=32, basis_atom_types=[1, 3], origin_step=2, max_atoms=30, seed=5)
    assert isinstance(rd, RadialDistribution) and all(np.array_equal(a, b) for a, b in zip(rd.groups, want))
    assert rd.counts.shape == (2, 2, 32) and rd.counts.dtype == np.uint64 and rd.origins == 5 and np.isclose(rd.r_edges[-1], served)
    assert np.array_equal(rd.group_sizes, [30, 30]) and np.array_equal(rd.samples, 5 * 30 * (30 - np.eye(2, dtype=np.int64)))
    assert np.array_equal(rd.counts.sum(axis=2) + rd.overflow, rd.samples.astype(np.uint64))
    dr = served / 32
    ref, allowed, borderline, total = P.reference(pos, P.TRICLINIC, want, [0], 2, dr, 32)
    assert borderline <= 1e-3 * total
    assert np.all(np.abs(rd.counts.astype(np.int64) - ref[0, :, :, :32]) <= allowed[0, :, :, :32])
    assert np.all(np.abs(rd.overflow.astype(np.int64) - ref[0, :, :, 32]) <= allowed[0, :, :, 32])
    assert np.isclose(rd.volume, abs(np.linalg.det(P.TRICLINIC.astype(np.float64))))
    assert np.allclose(rd.coordination[:, :, -1], rd.counts.sum(axis=2) / (5.0 * 30))
    assert calc.calculate_rdf().counts.shape == (1, 1, 200)
    vh = calc.calculate_distinct_van_hove([0, 1, 4], 8.0, 32, basis_atom_types=[1, 3], max_atoms=30, seed=5)
    assert isinstance(vh, VanHoveDistinct) and vh.counts.shape == (3, 2, 2, 32) and np.array_equal(vh.origins, [10, 9, 6])
    assert np.array_equal(vh.counts.sum(axis=3) + vh.overflow, vh.samples.astype(np.uint64))
    assert np.allclose(vh.times, 0.002 * np.array([0, 1, 4])) and np.array_equal(vh.lag_frames, [0, 1, 4])
    ref, allowed, borderline, total = P.reference(pos, P.TRICLINIC, want, [0, 1, 4], 1, 0.25, 32)
    assert borderline <= 1e-3 * total
    assert np.all(np.abs(vh.counts.astype(np.int64) - ref[..., :32]) <= allowed[..., :32])
    assert np.allclose((vh.radial_density * 0.25).sum(axis=3), vh.counts.sum(axis=3) / (vh.origins[:, None, None] * 30.0))


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    from psa_amd import _hip
    n, T = 37, 20
    _resident(engine, _walk("triclinic", n, T)["wrapped"])
    lib, h = engine._lib, engine._h
    f64p, f32p, i32p, i64p, u64p = (Ct.POINTER(t) for t in (Ct.c_double, Ct.c_float, Ct.c_int32, Ct.c_int64, Ct.c_uint64))
    H, inv = (np.ascontiguousarray(a) for a in R.box64(P.TRICLINIC))
    idx = np.arange(10, dtype=np.int32)
    start = np.array([0, 4, 10], np.int64)
    lags = np.array([0, 5], np.int64)
    cnt, frac = np.empty((2, 2, 2, 9), np.uint64), np.empty((T, 10, 3), np.float32)
    dr_ok = _served("triclinic") / 8

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)

    def refused(rc, word):
        msg = lib.psa_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def hist(box=H, binv=inv, ix=idx, st=start, G=2, lg=lags, n_vh=2, step=1, dr=dr_ok, n_r=8, o=cnt, nbytes=None):
        return lib.psa_pair_histogram(h, ptr(box, f64p), ptr(binv, f64p), ptr(ix, i32p), ptr(st, i64p), G, ptr(lg, i64p), n_vh, step, dr,
                                      n_r, ptr(o, u64p), cnt.nbytes if nbytes is None else nbytes)

    def dbg(binv=inv, ix=idx, n_g=10, o=frac):
        return lib.psa_debug_pair_fractions(h, ptr(binv, f64p), ptr(ix, i32p), n_g, ptr(o, f32p))

    assert hist() == 0 and dbg() == 0
    singular = H.copy()
    singular[2] = singular[0] + singular[1]
    refused(hist(box=None), "null")
    refused(hist(binv=None), "null")
    refused(hist(o=None), "null")
    refused(hist(lg=None), "null")
    refused(hist(st=None), "null")
    refused(hist(box=singular), "singular")
    refused(hist(binv=2.0 * inv), "not the inverse")
    refused(hist(box=H * np.nan), "finite")
    refused(hist(dr=dr_ok * 1.001), "served radius")                        # r_max above the served radius
    refused(hist(dr=100.0, n_r=1, nbytes=2 * 2 * 2 * 2 * 8), "served radius")
    for dr in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
        refused(hist(dr=dr), "bin width")
    refused(hist(n_r=0, nbytes=0), "number of bins")
    refused(hist(n_r=1025, dr=1e-3), "number of bins")
    refused(hist(n_vh=0), "number of lags")
    refused(hist(n_vh=65), "number of lags")
    refused(hist(lg=np.array([0, T], np.int64)), "outside [0, T - 1")
    refused(hist(lg=np.array([-1, 3], np.int64)), "outside [0, T - 1")
    refused(hist(step=0), "origin_step")
    refused(hist(G=0), "groups")
    refused(hist(G=9), "groups")
    refused(hist(st=np.array([1, 4, 10], np.int64)), "must be 0")
    refused(hist(st=np.array([0, 6, 4], np.int64)), "ascending")
    refused(hist(ix=None), "n_groups must be 1")
    refused(hist(nbytes=8), "out_bytes")
    for call in (hist, dbg):
        refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 37], np.int32)), "out of bounds")
        refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1], np.int32)), "out of bounds")
        refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 3], np.int32)), "twice")
    refused(dbg(binv=None), "null")
    refused(dbg(o=None), "null")
    refused(dbg(binv=np.ascontiguousarray(np.linalg.pinv(singular))), "singular")
    # one species of all atoms
    one = np.empty((2, 1, 1, 9), np.uint64)
    assert lib.psa_pair_histogram(h, ptr(H, f64p), ptr(inv, f64p), None, None, 1, ptr(lags, i64p), 2, 1, dr_ok, 8, ptr(one, u64p),
                                  one.nbytes) == 0
    # a budget below one origin names the bytes
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * 10 - 1)
    for call in (hist, dbg):
        refused(call(), f"need {24 * 10} bytes")
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * 10)
    again = np.empty_like(cnt)
    assert hist(o=again) == 0 and dbg() == 0 and np.array_equal(again, cnt)
    # no positions resident
    engine.release(_hip.SLOT_POSITIONS)
    engine.invalidate(_hip.SLOT_POSITIONS)
    for call in (hist, dbg):
        refused(call(), "positions slot holds no array")


def test_sharded_context_is_refused(engine):
    """a context that holds a communicator (one rank is enough) is refused by both entry points, and serves again once
    the communicator is gone"""
    n, T = 37, 20
    _resident(engine, _walk("triclinic", n, T)["wrapped"])
    lib, h = engine._lib, engine._h
    f64p, f32p, i64p, u64p = (Ct.POINTER(t) for t in (Ct.c_double, Ct.c_float, Ct.c_int64, Ct.c_uint64))
    H, inv = (np.ascontiguousarray(a) for a in R.box64(P.TRICLINIC))
    hp, ip = H.ctypes.data_as(f64p), inv.ctypes.data_as(f64p)
    lags = np.array([0, 5], np.int64)
    cnt, frac = np.empty((2, 1, 1, 9), np.uint64), np.empty((T, n, 3), np.float32)
    entries = {
        "psa_pair_histogram": lambda: lib.psa_pair_histogram(h, hp, ip, None, None, 1, lags.ctypes.data_as(i64p), 2, 1, 0.5, 8,
                                                             cnt.ctypes.data_as(u64p), cnt.nbytes),
        "psa_debug_pair_fractions": lambda: lib.psa_debug_pair_fractions(h, ip, None, 0, frac.ctypes.data_as(f32p)),
    }
    assert [call() for call in entries.values()] == [0, 0]
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        got = {name: (call(), lib.psa_last_error().decode()) for name, call in entries.items()}
    finally:
        engine.comm_destroy()
    for name, (rc, msg) in got.items():
        assert rc == -1 and "sharded context" in msg and name in msg, (name, rc, msg)
    assert [call() for call in entries.values()] == [0, 0]


# ---- no trace -----------------------------------------------------------------------------------------------------------
def test_no_trace_in_the_other_entry_points(engine):
    """`calculate`, `calculate_self_spectra` and `calculate_van_hove` give the bits they gave before the pair calls in
    between; atom weights and segments set on the context change nothing; the stage times are where the header says"""
    from psa_amd import Segments, commensurate_vectors
    pos = _walk("cubic", 37, 40)["wrapped"]
    calc = _calculator(engine, pos, P.CUBIC)
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    half = commensurate_vectors(P.CUBIC, 1.2, 0.1)[0][:12]
    for _ in range(2):
        calc.calculate(mags, vecs)
    weights = np.linspace(0.5, 2.0, 37).astype(np.float32)
    s = Segments(16, 8, "hann")

    def spectra():
        return (calc.calculate(mags, vecs).sed.view(np.uint32), calc.calculate_self_spectra(half, segments=s, atom_weights=weights).density.view(np.uint32),
                calc.calculate_van_hove([1, 9], 6.0, 48).counts)
    before = spectra()
    engine.timings()                                                       # (reset)
    rd = calc.calculate_rdf(n_r=48)
    t = engine.timings()
    assert t["gather"] > 0 and t["transpose"] > 0 and t["epilogue"] > 0 and t["d2h"] > 0 and t["fft"] == 0 and t["project"] == 0
    vh = calc.calculate_distinct_van_hove([1, 30], 6.0, 48)
    for a, b in zip(before, spectra()):
        assert np.array_equal(a, b)
    engine.set_atom_weights(weights)
    engine.set_segments(s)
    assert np.array_equal(calc.calculate_rdf(n_r=48).counts, rd.counts)
    assert np.array_equal(calc.calculate_distinct_van_hove([1, 30], 6.0, 48).counts, vh.counts)
