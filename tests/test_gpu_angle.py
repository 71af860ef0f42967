"""Bond angles and coordination on the GPU (psa_angle_histogram, psa_debug_neighbour_lists and the calculator method)
against the brute-force float64 reference of tests/angle64.py inside the allowance of tests/angle_cases.py: random walks
at every edge of the centre tile, one, two and three species, a scalar cut-off and a matrix with a zero entry, 1 to 1024
bins, the origin steps; every identity of the definition exact; the neighbour counts against psa_pair_histogram bit for
bit; the neighbour lists against the reference's sets; lattices whose angles are known; the capacity; coincident
neighbours; workgroups that loop; budgets, permutations and repeated calls bit for bit; the calculator; every refusal (a
context with a communicator among them); no trace in later calls.

Every counts test first asserts the reference's borderline share under the cap, then prints how many counts moved."""
import ctypes as Ct
import functools

import numpy as np
import pytest

import angle64 as A
import angle_cases as Q
import pair64 as R
import pair_cases as P
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = Q.BOXES
TILE = 256
PER_ORIGIN = 1040                                                          # work bytes per atom and origin


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


@functools.lru_cache(maxsize=None)
def _walk(box, n_atoms, n_frames, seed=11):
    return P.walk(n_atoms, n_frames, seed, box=BOXES[box])["wrapped"]


def _shape(n_atoms):
    """(frames, r_cut) of a walk of that many atoms: about a dozen neighbours where the atoms allow it"""
    if n_atoms <= 37:
        return 12, 8.0
    return (4, 5.0) if n_atoms <= 300 else (3, 4.1)


def _groups(kind, n_atoms):
    return {"one": lambda n: [np.arange(n)], "two": Q.two_species, "three": Q.three_species}[kind](n_atoms)


def _listing(kind, groups):
    return None if kind == "one" else [np.asarray(g, np.int32) for g in groups]


@functools.lru_cache(maxsize=None)
def _reference(box, n_atoms, n_frames, kind, matrix, r_cut, step, n_theta):
    groups = _groups(kind, n_atoms)
    rc = Q.matrix_cutoff(r_cut, len(groups)) if matrix else r_cut
    return groups, rc, Q.reference(_walk(box, n_atoms, n_frames), BOXES[box], groups, rc, step, n_theta)


def _cross_from_lists(engine, box, rc, listing, groups, frames):
    """(S, P) the sum over the centres with at most 64 neighbours of n_beta n_gamma (n (n - 1) / 2 on the diagonal), from the
    debug entry's lists"""
    S = len(groups)
    _, spec = A.species_of(groups)
    out = np.zeros((S, S * (S + 1) // 2), np.int64)
    for f in frames:
        count, lst = engine.debug_neighbour_lists(box, rc, int(f), listing)
        for a in np.flatnonzero(count <= Q.CAPACITY):
            n = np.bincount(spec[lst[a, :count[a]]], minlength=S)
            for be in range(S):
                out[spec[a], A.pair_row(be, be, S)] += n[be] * (n[be] - 1) // 2
                for ga in range(be + 1, S):
                    out[spec[a], A.pair_row(be, ga, S)] += n[be] * n[ga]
    return out


def _run(engine, box, n_atoms, kind="one", matrix=False, step=1, n_theta=45, lists=True):
    n_frames, r_cut = _shape(n_atoms)
    what = f"{box} N {n_atoms} T {n_frames} {kind} matrix {matrix} step {step} n_theta {n_theta}"
    groups, rc, ref = _reference(box, n_atoms, n_frames, kind, matrix, r_cut, step, n_theta)
    assert ref["borderline"] <= Q.cap(n_theta) * max(ref["triplets"], 1), what       # the borderline condition, before anything else
    pos, H, listing = _walk(box, n_atoms, n_frames), BOXES[box], _listing(kind, groups)
    _resident(engine, pos)
    got = engine.angle_histogram(H, rc, n_theta, listing, origin_step=step)
    S, n_o = len(groups), A.n_origins(n_frames, step)
    assert all(g.dtype == np.uint64 for g in got)
    assert got[0].shape == (S, S * (S + 1) // 2, n_theta + 1) and got[1].shape == (S, S, 65) and got[2].shape == (S,)
    assert Q.check(got, ref, what)
    assert Q.identities(got, [len(g) for g in groups], n_o), what
    origins = range(0, n_frames, step)
    assert np.array_equal(got[0].astype(np.int64).sum(axis=2), _cross_from_lists(engine, H, rc, listing, groups, origins)), what
    if not matrix and not got[2].any():                                    # the neighbours are the pair histogram's bin 0, bit for bit
        pairs = engine.pair_histogram(H, [0], r_cut, 1, listing, origin_step=step)[0, :, :, 0].astype(np.int64)
        assert np.array_equal((got[1].astype(np.int64) * np.arange(65)).sum(axis=2), pairs), what
    if lists:
        _, spec = A.species_of(groups)
        for j, f in enumerate(origins):
            count, lst = engine.debug_neighbour_lists(H, rc, f, listing)
            for a, (sure, edge) in enumerate(ref["lists"][j]):
                mine = lst[a, :min(count[a], 64)]
                assert np.all(np.diff(mine) > 0) and np.all(lst[a, count[a]:] == -1)
                assert np.all(np.isin(sure, mine)) and np.all(np.isin(mine, np.concatenate([sure, edge]))), (what, f, a)
    return got


# ---- random walks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [1, 2, 3, 37, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
@pytest.mark.parametrize("box", BOXES)
def test_counts_one_species(engine, box, n_atoms):
    got = _run(engine, box, n_atoms)
    if n_atoms == 1:
        assert not got[0].any() and got[1][0, 0, 0] == 12


@pytest.mark.parametrize("box,n_atoms,kind,matrix", [("cubic", 37, "two", True), ("triclinic", 37, "three", False), ("triclinic", 37, "three", True),
                                                     ("cubic", 3, "two", False), ("triclinic", 2, "three", True),
                                                     ("triclinic", TILE + 1, "two", True), ("cubic", TILE + 1, "three", True),
                                                     ("cubic", 2 * TILE + 3, "two", False), ("triclinic", 2 * TILE + 3, "three", True)])
def test_counts_species(engine, box, n_atoms, kind, matrix):
    """two species: 40 atoms against the rest; "three": an empty species between two shuffled ones; the matrix has two
    different cut-offs and a zero: the last species does not bond to itself"""
    got = _run(engine, box, n_atoms, kind, matrix)
    S = got[1].shape[0]
    if kind == "three":
        assert not got[0][1].any() and not got[1][1].any() and not got[1][:, 1, 1:].any()
    if matrix and S > 1:
        assert not got[0][S - 1, A.pair_row(S - 1, S - 1, S)].any() and not got[1][S - 1, S - 1, 1:].any()


@pytest.mark.parametrize("step", [1, 3, 50])
def test_origin_steps(engine, step):
    _run(engine, "triclinic", 37, "three", True, step=step)


@pytest.mark.parametrize("n_theta", [1, 180, 1024])
@pytest.mark.parametrize("box", BOXES)
def test_bins(engine, box, n_theta):
    _run(engine, box, TILE + 1, "two", False, n_theta=n_theta, lists=False)


# ---- lattices, exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", P.LATTICE_BOXES)
def test_simple_cubic(engine, box):
    """4 x 4 x 4 simple cubic, r_cut = 1.2 a: 6 neighbours, 12 angles of 90 degrees (bin 22 of 45: 88..92) and 3 of 180 (the
    last bin) per atom and origin, nothing elsewhere"""
    H = P.LATTICE_BOXES[box]
    pos, a = P.simple_cubic(5, box)
    _resident(engine, pos)
    for step, n_o in ((1, 5), (2, 3)):
        angles, coord, trunc = engine.angle_histogram(H, 1.2 * a, 45, origin_step=step)
        want = np.zeros(46, np.int64)
        want[22], want[44] = 12 * 64 * n_o, 3 * 64 * n_o
        assert np.array_equal(angles[0, 0], want) and not trunc.any()
        assert coord[0, 0, 6] == 64 * n_o and coord.sum() == 64 * n_o


def test_diamond_as_zincblende(engine):
    """512 atoms of diamond as two species, r_cut = 2.8 above the bond of 2.35 and below the second shell of 3.84: four
    neighbours of the other species, six angles of 109.47 degrees (bin 27 of 45: 108..112) per centre"""
    pos, groups = Q.diamond(3)
    _resident(engine, pos)
    listing = [np.asarray(g, np.int32) for g in groups]
    angles, coord, trunc = engine.angle_histogram(Q.CUBIC, 2.8, 45, listing)
    assert coord[0, 1, 4] == 3 * 256 and coord[1, 0, 4] == 3 * 256 and coord[0, 0, 0] == 3 * 256 and coord[1, 1, 0] == 3 * 256
    assert coord.sum() == 4 * 3 * 256 and not trunc.any()
    want = np.zeros(46, np.int64)
    want[27] = 6 * 3 * 256
    assert np.array_equal(angles[0, A.pair_row(1, 1, 2)], want) and np.array_equal(angles[1, A.pair_row(0, 0, 2)], want)
    assert angles.sum() == 2 * want.sum()                                  # zeros in (0; 0,0), (0; 0,1) and their mirror


# ---- capacity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_on", [64, 65])
def test_sphere_of_64_and_65(engine, n_on):
    """a centre with exactly 64 and with 65 atoms on a sphere of radius 3 around it, r_cut = 3.5: the centre is counted with
    64 and left out with 65, all or nothing; the atoms on the sphere see the centre and a few of each other either way"""
    pos = Q.sphere(n_on, 3.0)
    groups = [np.arange(1), np.arange(1, n_on + 1)]
    listing = [np.asarray(g, np.int32) for g in groups]
    ref = Q.reference(pos, Q.CUBIC, groups, 3.5, 1, 45)
    assert ref["borderline"] <= Q.cap(45) * ref["triplets"] and ref["leg_borderline"] == 0
    _resident(engine, pos)
    got = engine.angle_histogram(Q.CUBIC, 3.5, 45, listing)
    assert Q.check(got, ref, f"sphere of {n_on}") and Q.identities(got, [1, n_on], 1)
    count, lst = engine.debug_neighbour_lists(Q.CUBIC, 3.5, 0, listing)
    assert count[0] == n_on and np.array_equal(lst[0], np.arange(1, 65))
    if n_on == 64:
        assert got[2][0] == 0 and got[1][0, 1, 64] == 1 and got[0][0, A.pair_row(1, 1, 2)].sum() == 64 * 63 // 2
    else:
        assert got[2][0] == 1 and not got[1][0].any() and not got[0][0].any()
    assert got[2][1] == 0 and got[1][1, 0, 1] == n_on


def test_ball_all_truncated(engine):
    """100 atoms inside a ball of radius r_cut / 2: 99 neighbours each, all truncated, all histograms zero"""
    pos = Q.ball(100, 3, 6.0)
    _resident(engine, pos)
    angles, coord, trunc = engine.angle_histogram(Q.CUBIC, 6.0, 45)
    assert trunc[0] == 300 and not angles.any() and not coord.any()
    count, lst = engine.debug_neighbour_lists(Q.CUBIC, 6.0, 2)
    assert np.all(count == 99) and np.all(lst >= 0)
    calc = _calculator(engine, pos, Q.CUBIC)
    with pytest.raises(ValueError, match="species 0: 300.*smaller r_cut"):
        calc.calculate_bond_angles(6.0, 45)


# ---- degenerate -----------------------------------------------------------------------------------------------------------
def test_coincident_neighbours(engine):
    """two atoms at one place: each is the other's neighbour at distance 0, and every angle with that leg is undefined; the
    totals stay exact"""
    pos = _walk("cubic", 37, 12).copy()
    pos[:, 5] = pos[:, 9]
    groups = [np.arange(37)]
    ref = Q.reference(pos, Q.CUBIC, groups, 8.0, 1, 45)
    assert ref["borderline"] <= Q.cap(45) * ref["triplets"] and ref["angles"][0, 0, 45] > 0
    _resident(engine, pos)
    got = engine.angle_histogram(Q.CUBIC, 8.0, 45)
    assert Q.check(got, ref, "coincident") and Q.identities(got, [37], 12)
    assert got[0][0, 0, 45] == ref["angles"][0, 0, 45]                     # a distance of exactly 0 is no rounding matter


# ---- bit for bit ----------------------------------------------------------------------------------------------------------
def _equal(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def test_permutations_budgets_and_repeats(engine):
    from psa_amd import _hip
    n, T = 2 * TILE + 3, 6
    pos = _walk("triclinic", n, T)
    _resident(engine, pos)
    groups = Q.two_species(n)
    listing = _listing("two", groups)
    rc = Q.matrix_cutoff(4.1, 2)
    whole = engine.angle_histogram(Q.TRICLINIC, rc, 180, listing)
    assert whole[0].any() and _equal(whole, engine.angle_histogram(Q.TRICLINIC, rc, 180, listing))
    rng = np.random.default_rng(8)
    assert _equal(whole, engine.angle_histogram(Q.TRICLINIC, rc, 180, [rng.permutation(g) for g in listing]))
    for origins in (1, 2, 4):                                              # origins per block
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n * origins + 5)
        assert _equal(whole, engine.angle_histogram(Q.TRICLINIC, rc, 180, listing))
    # one species of all atoms is the sum over the two, with one cut-off
    reset(engine)
    two = engine.angle_histogram(Q.TRICLINIC, 4.1, 180, listing)
    one = engine.angle_histogram(Q.TRICLINIC, 4.1, 180)
    assert np.array_equal(one[0][0, 0], two[0].sum(axis=(0, 1))) and one[2][0] == two[2].sum() == 0


def test_walk_case_is_the_twin_exactly(engine):
    """`angle_cases.walk_case`, every branch of the centre walk: its five origins in blocks of 2, 2 and 1, and the five frames
    280 times over in one block -- 3 items x 1400 origins are more than the 4096 workgroups a launch aims at, so a slab holds
    two origins and a wavefront walks on from one into the next.  Every count is the twin's (angle_cases.model), exactly"""
    from psa_amd import _hip
    pos, box, groups, rc = Q.walk_case()
    listing = [np.asarray(g, np.int32) for g in groups]
    want = Q.model(pos, box, groups, rc, 1, 1024)
    assert want[2].tolist() == [2, 0] and want[0][..., 1024].sum() == 4 and want[1][0, 0, 64] == 3
    _resident(engine, pos)
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * 70 * 2 + 5)
    got = engine.angle_histogram(box, rc, 1024, listing)
    assert all(np.array_equal(g.astype(np.int64), w) for g, w in zip(got, want))
    reset(engine)
    reps = 280
    _resident(engine, np.tile(pos, (reps, 1, 1)))
    got = engine.angle_histogram(box, rc, 1024, listing)
    assert all(np.array_equal(g.astype(np.int64), reps * w) for g, w in zip(got, want))


def test_species_pairs_in_chunks(engine):
    """eight species at 1024 bins: 36 species pairs, 11 of which fit a workgroup's histograms, so the angle pass runs four
    chunks of pairs; the sum over all is the one-species histogram"""
    n, T = 2 * TILE + 3, 3
    _resident(engine, _walk("cubic", n, T))
    order = np.random.default_rng(4).permutation(n).astype(np.int32)
    listing = np.array_split(order, 8)
    many = engine.angle_histogram(Q.CUBIC, 4.1, 1024, listing)
    one = engine.angle_histogram(Q.CUBIC, 4.1, 1024)
    assert Q.identities(many, [len(g) for g in listing], T) and Q.identities(one, [n], T)
    assert np.array_equal(one[0][0, 0], many[0].sum(axis=(0, 1))) and (many[0].sum(axis=(0, 2)) > 0).all()


# ---- workgroups that loop ---------------------------------------------------------------------------------------------------
def test_many_tiles(engine):
    """32 845 atoms x 2 frames, r_cut for about 12 neighbours: 129 centre tiles that each walk 129 beta-tiles.  No reference
    over N^2: the identities, one species against the sum over two, a permuted list and a one-origin budget bit for bit,
    and the lists of 300 centres against the brute force over a thinned set of partners"""
    from psa_amd import _hip
    n, T = 128 * TILE + 77, 2
    pos = P.walk(n, T, 12, box=Q.TRICLINIC)["wrapped"]
    _resident(engine, pos)
    volume = abs(np.linalg.det(Q.TRICLINIC.astype(np.float64)))
    r_cut = float((12.0 / n * volume * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0))
    one = engine.angle_histogram(Q.TRICLINIC, r_cut, 45)
    assert Q.identities(one, [n], T) and one[2][0] == 0
    mean = float((one[1][0, 0] * np.arange(65)).sum()) / (n * T)
    assert 10.0 < mean < 14.0
    order = np.random.default_rng(5).permutation(n).astype(np.int32)
    sizes = [79 * TILE - 9, n - (79 * TILE - 9)]
    listing = [order[: sizes[0]], order[sizes[0]:]]
    two = engine.angle_histogram(Q.TRICLINIC, r_cut, 45, listing)
    assert Q.identities(two, sizes, T)
    assert np.array_equal(two[0].sum(axis=(0, 1)), one[0][0, 0])
    rng = np.random.default_rng(6)
    assert _equal(two, engine.angle_histogram(Q.TRICLINIC, r_cut, 45, [rng.permutation(g) for g in listing]))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n + 3)     # one origin per block
    assert _equal(two, engine.angle_histogram(Q.TRICLINIC, r_cut, 45, listing))
    reset(engine)
    # 300 centres spread over all tiles against every 8th of the rest: the reference's sets, and the same pairs in the full call
    pick = np.sort(order[:300])
    rest = np.setdiff1d(np.arange(n), pick).astype(np.int32)
    wide = 1.3 * r_cut
    rc = np.array([[wide, wide], [wide, 0.0]])
    sets = A.neighbour_sets(pos[1], Q.TRICLINIC, [pick, rest[::8]], rc, centres=np.arange(300))
    count, lst = engine.debug_neighbour_lists(Q.TRICLINIC, rc, 1, [pick.astype(np.int32), rest[::8]])
    full_count, full = engine.debug_neighbour_lists(Q.TRICLINIC, rc, 1, [pick.astype(np.int32), rest])
    assert count[:300].max() <= 64 and full_count[:300].max() <= 64 and count[:300].sum() > 500
    thinned = np.concatenate([np.arange(300), 300 + np.arange(rest.size)[::8]])   # list positions of the thinned set in the full list
    for a in range(300):
        mine = lst[a, :count[a]]
        assert np.array_equal(mine, sets[a]), a                            # (no leg within rounding of the cut-off: asserted by equality)
        assert np.array_equal(thinned[mine], np.intersect1d(full[a, :full_count[a]], thinned)), a


# ---- the calculator -------------------------------------------------------------------------------------------------------
def _calculator(engine, pos, box, types=None, dt=0.002):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, 1, 1, 1).attach(engine=engine)


def test_calculator(engine):
    from psa_amd import BondAngleDistribution
    n, T = TILE + 1, 4
    pos = _walk("triclinic", n, T)
    types = np.ones(n, np.int32)
    types[Q.two_species(n)[1]] = 2
    calc = _calculator(engine, pos, Q.TRICLINIC, types)
    groups, rc, ref = _reference("triclinic", n, T, "two", True, 5.0, 1, 45)
    res = calc.calculate_bond_angles(rc, 45, basis_atom_types=[1, 2])
    assert isinstance(res, BondAngleDistribution) and all(np.array_equal(a, b) for a, b in zip(res.groups, groups))
    got = (np.concatenate([res.counts, res.undefined[:, :, None]], axis=2), res.coordination_counts, res.truncated)
    assert Q.check(got, ref, "calculator") and Q.identities(got, [len(g) for g in groups], T)
    assert res.origins == T and np.array_equal(res.samples, [T * len(groups[0]), T * len(groups[1])])
    assert np.allclose(res.coordination_fraction.sum(axis=2), 1.0) and np.allclose((res.density * 4.0).sum(axis=2)[res.counts.sum(axis=2) > 0], 1.0)
    assert np.array_equal(res.triplet(0, 1, 0), res.counts[0, 1])
    half = calc.calculate_bond_angles(5.0, origin_step=2)
    assert half.counts.shape == (1, 1, 180) and half.origins == 2


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    from psa_amd import _hip, max_pair_radius
    n, T = 37, 12
    _resident(engine, _walk("triclinic", n, T))
    lib, h = engine._lib, engine._h
    f64p, i32p, i64p, u64p = (Ct.POINTER(t) for t in (Ct.c_double, Ct.c_int32, Ct.c_int64, Ct.c_uint64))
    H, inv = (np.ascontiguousarray(a) for a in R.box64(Q.TRICLINIC))
    idx = np.arange(10, dtype=np.int32)
    start = np.array([0, 4, 10], np.int64)
    rc = np.array([[5.0, 4.0], [4.0, 0.0]])
    ang, crd, trn = np.empty((2, 3, 46), np.uint64), np.empty((2, 2, 65), np.uint64), np.empty(2, np.uint64)
    cnt, lst = np.empty(10, np.int32), np.empty((10, 64), np.int32)
    served = max_pair_radius(Q.TRICLINIC)

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)

    def refused(rc_, word):
        msg = lib.psa_last_error().decode()
        assert rc_ == -1 and word in msg, (rc_, msg)

    def hist(box=H, binv=inv, ix=idx, st=start, G=2, r=rc, step=1, n_theta=45, a=ang, c=crd, t=trn, abytes=None, cbytes=None):
        return lib.psa_angle_histogram(h, ptr(box, f64p), ptr(binv, f64p), ptr(ix, i32p), ptr(st, i64p), G, ptr(r, f64p), step, n_theta,
                                       ptr(a, u64p), ang.nbytes if abytes is None else abytes, ptr(c, u64p),
                                       crd.nbytes if cbytes is None else cbytes, ptr(t, u64p))

    def dbg(box=H, binv=inv, ix=idx, st=start, G=2, r=rc, frame=0, c=cnt, o=lst):
        return lib.psa_debug_neighbour_lists(h, ptr(box, f64p), ptr(binv, f64p), ptr(ix, i32p), ptr(st, i64p), G, ptr(r, f64p), frame,
                                             ptr(c, i32p), ptr(o, i32p))

    assert hist() == 0 and dbg() == 0
    singular = H.copy()
    singular[2] = singular[0] + singular[1]
    for call in (hist, dbg):
        refused(call(box=None), "null")
        refused(call(binv=None), "null")
        refused(call(r=None), "null")
        refused(call(st=None), "null")
        refused(call(box=singular), "singular")
        refused(call(binv=2.0 * inv), "not the inverse")
        refused(call(box=H * np.nan), "finite")
        refused(call(r=np.array([[5.0, 4.0], [4.5, 0.0]])), "not symmetric")
        refused(call(r=np.array([[5.0, -4.0], [-4.0, 0.0]])), "not negative")
        refused(call(r=np.array([[np.nan, 4.0], [4.0, 0.0]])), "finite")
        refused(call(r=np.array([[np.inf, 4.0], [4.0, 0.0]])), "finite")
        refused(call(r=np.array([[served * 1.001, 4.0], [4.0, 0.0]])), "served radius")
        refused(call(G=0), "groups")
        refused(call(G=9), "groups")
        refused(call(st=np.array([1, 4, 10], np.int64)), "must be 0")
        refused(call(st=np.array([0, 6, 4], np.int64)), "ascending")
        refused(call(ix=None), "n_groups must be 1")
        refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 37], np.int32)), "out of bounds")
        refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1], np.int32)), "out of bounds")
        refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 3], np.int32)), "twice")
    assert hist(r=np.array([[served, 4.0], [4.0, 0.0]])) == 0               # the served radius itself
    refused(hist(a=None), "null")
    refused(hist(c=None), "null")
    refused(hist(t=None), "null")
    refused(hist(n_theta=0, abytes=2 * 3 * 8), "number of bins")
    refused(hist(n_theta=1025, abytes=2 * 3 * 1026 * 8), "number of bins")
    refused(hist(step=0), "origin_step")
    refused(hist(abytes=8), "angles_bytes")
    refused(hist(cbytes=8), "coord_bytes")
    refused(dbg(c=None), "null")
    refused(dbg(o=None), "null")
    refused(dbg(frame=-1), "outside [0, T - 1")
    refused(dbg(frame=T), "outside [0, T - 1")
    assert dbg(frame=T - 1) == 0
    # one species of all atoms
    one_a, one_c, one_t, one_r = np.empty((1, 1, 46), np.uint64), np.empty((1, 1, 65), np.uint64), np.empty(1, np.uint64), np.array([5.0])
    assert lib.psa_angle_histogram(h, ptr(H, f64p), ptr(inv, f64p), None, None, 1, ptr(one_r, f64p), 1, 45, ptr(one_a, u64p), one_a.nbytes,
                                   ptr(one_c, u64p), one_c.nbytes, ptr(one_t, u64p)) == 0
    # a budget below one origin names the bytes
    assert hist() == 0
    keep = ang.copy()
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * 10 - 1)
    for call in (hist, dbg):
        refused(call(), f"need {PER_ORIGIN * 10} bytes")
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * 10)
    assert hist() == 0 and dbg() == 0 and np.array_equal(ang, keep)
    # no positions resident
    engine.release(_hip.SLOT_POSITIONS)
    engine.invalidate(_hip.SLOT_POSITIONS)
    for call in (hist, dbg):
        refused(call(), "positions slot holds no array")


def test_sharded_context_is_refused(engine):
    """a context that holds a communicator (one rank is enough) is refused by both entry points, and serves again once
    the communicator is gone; the calculator refuses a sharded run before it"""
    n, T = 37, 12
    _resident(engine, _walk("triclinic", n, T))
    lib, h = engine._lib, engine._h
    f64p, i32p, u64p = (Ct.POINTER(t) for t in (Ct.c_double, Ct.c_int32, Ct.c_uint64))
    H, inv = (np.ascontiguousarray(a) for a in R.box64(Q.TRICLINIC))
    hp, ip = H.ctypes.data_as(f64p), inv.ctypes.data_as(f64p)
    rc = np.array([5.0])
    ang, crd, trn = np.empty((1, 1, 46), np.uint64), np.empty((1, 1, 65), np.uint64), np.empty(1, np.uint64)
    cnt, lst = np.empty(n, np.int32), np.empty((n, 64), np.int32)
    entries = {
        "psa_angle_histogram": lambda: lib.psa_angle_histogram(h, hp, ip, None, None, 1, rc.ctypes.data_as(f64p), 1, 45, ang.ctypes.data_as(u64p),
                                                               ang.nbytes, crd.ctypes.data_as(u64p), crd.nbytes, trn.ctypes.data_as(u64p)),
        "psa_debug_neighbour_lists": lambda: lib.psa_debug_neighbour_lists(h, hp, ip, None, None, 1, rc.ctypes.data_as(f64p), 0,
                                                                           cnt.ctypes.data_as(i32p), lst.ctypes.data_as(i32p)),
    }
    assert [call() for call in entries.values()] == [0, 0]
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        got = {name: (call(), lib.psa_last_error().decode()) for name, call in entries.items()}
    finally:
        engine.comm_destroy()
    for name, (rc_, msg) in got.items():
        assert rc_ == -1 and "sharded context" in msg and name in msg, (name, rc_, msg)
    assert [call() for call in entries.values()] == [0, 0]


# ---- no trace -----------------------------------------------------------------------------------------------------------
def test_no_trace_in_the_other_entry_points(engine):
    """`calculate`, `calculate_rdf` and `calculate_van_hove` give the bits they gave before the angle calls in between; atom
    weights and segments set on the context change nothing; the stage times are where the header says"""
    from psa_amd import Segments
    pos = _walk("cubic", 37, 12)
    calc = _calculator(engine, pos, Q.CUBIC)
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    for _ in range(2):
        calc.calculate(mags, vecs)

    def others():
        return (calc.calculate(mags, vecs).sed.view(np.uint32), calc.calculate_rdf(n_r=48).counts, calc.calculate_van_hove([1, 9], 6.0, 48).counts)
    before = others()
    engine.timings()                                                       # (reset)
    res = calc.calculate_bond_angles(8.0, 45)
    t = engine.timings()
    assert t["gather"] > 0 and t["transpose"] > 0 and t["phase"] > 0 and t["epilogue"] > 0 and t["d2h"] > 0
    assert t["fft"] == 0 and t["project"] == 0
    engine.debug_neighbour_lists(Q.CUBIC, 8.0, 3)
    for a, b in zip(before, others()):
        assert np.array_equal(a, b)
    engine.set_atom_weights(np.linspace(0.5, 2.0, 37).astype(np.float32))
    engine.set_segments(Segments(8, 4, "hann"))
    assert np.array_equal(calc.calculate_bond_angles(8.0, 45).counts, res.counts)
