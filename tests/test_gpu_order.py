"""The Steinhardt order parameters on the GPU (psa_bond_order, Engine.bond_order and the calculator method): the per-atom X
against the spherical-harmonic float64 reference of tests/order64.py inside the allowance of tests/order_cases.py -- random
walks with one, two and three species, a scalar cut-off and a matrix with a zero entry, one, two and eight orders, the origin
steps --; the edges of the centre tile and of the item; centres with 0 to 65 neighbours; a coincident pair; lattices whose q_l
are known; the histogram against the integer bin rule applied to the returned X, exactly; every identity; the neighbour counts
against psa_debug_neighbour_lists and psa_pair_histogram bit for bit; budgets, blocks, permutations and repeated calls bit
for bit; the calculator; every refusal (a context with a communicator among them); no trace in later calls.

Every comparison first asserts the excluded share under the cap, then prints the largest |dX| as a share of its allowance."""
import ctypes as Ct
import functools

import numpy as np
import pytest

import angle64 as A
import angle_cases as Q
import order64 as O
import order_cases as C
import pair64 as R
import pair_cases as P
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = Q.BOXES
PER_ORIGIN = 1040                                                          # work bytes per atom and origin, without x
EIGHT = (1, 2, 3, 5, 7, 8, 10, 12)


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


def _groups(kind, n_atoms):
    return {"one": lambda n: [np.arange(n)], "two": Q.two_species, "three": Q.three_species}[kind](n_atoms)


def _listing(kind, groups):
    return None if kind == "one" else [np.asarray(g, np.int32) for g in groups]


@functools.lru_cache(maxsize=None)
def _walk(box, n_atoms, n_frames, seed=11):
    return P.walk(n_atoms, n_frames, seed, box=BOXES[box])["wrapped"]


def _held(engine, pos, box, groups, listing, rc, step, ls, n_q, what, ref=None):
    """one call with per-atom output held to the reference, the bin rule and the identities; returns what the engine gave"""
    ref = C.reference(pos, box, groups, rc, step, list(ls)) if ref is None else ref
    assert C.excluded_share(ref) <= C.EXCLUDED_CAP, what                  # the excluded share, before anything else
    _resident(engine, pos)
    got = engine.bond_order(box, rc, ls, n_q, listing, origin_step=step, per_atom=True)
    hist, trunc, iso, undef, x, n = got
    S, n_o, n_a = len(groups), A.n_origins(pos.shape[0], step), sum(len(g) for g in groups)
    assert all(g.dtype == np.uint64 for g in got[:4]) and x.dtype == np.int64 and n.dtype == np.int32
    assert hist.shape == (S, len(ls), n_q) and trunc.shape == iso.shape == undef.shape == (S,)
    assert x.shape == (n_o, n_a, len(ls)) and n.shape == (n_o, n_a)
    assert C.check(x, n, ref, what), what
    sizes = [len(g) for g in groups]
    want, out = C.histogram_of(x, n, sizes, n_q)
    assert np.array_equal(hist.astype(np.int64), want), what                # the integer bin rule, exactly
    left = (trunc + iso + undef).astype(np.int64)
    assert np.array_equal(left, out) and np.all(want.sum(axis=2) + left[:, None] == n_o * np.array(sizes)[:, None]), what
    full = n.astype(np.int64)[..., None] ** 2 * C.ONE
    assert np.all((x >= 0) <= (x <= full)) and np.all(x >= -1)
    return got


# ---- random walks against the reference -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family_reference(name, kind, matrix, step, ls):
    pos, box, r_cut = C.family(name)
    groups = _groups(kind, pos.shape[1])
    rc = Q.matrix_cutoff(r_cut, len(groups)) if matrix else r_cut
    return pos, box, groups, rc, C.reference(pos, box, groups, rc, step, list(ls))


@pytest.mark.parametrize("name,kind,matrix,step,ls", [
    ("cubic130", "one", False, 1, (4, 6)), ("triclinic130", "one", False, 1, (4, 6)), ("cubic37", "one", False, 1, (4, 6)),
    ("triclinic257", "one", False, 1, (4, 6)), ("cubic130", "two", True, 3, (1,)), ("triclinic130", "three", False, 1, (12,)),
    ("cubic37", "three", True, 3, EIGHT), ("triclinic257", "two", False, 1, (4, 6)), ("cubic37", "two", True, 1, EIGHT)])
def test_per_atom_against_the_reference(engine, name, kind, matrix, step, ls):
    pos, box, groups, rc, ref = _family_reference(name, kind, matrix, step, ls)
    if kind == "one":
        assert not ref["excluded"].any()                                    # no leg-borderline neighbour at all
    got = _held(engine, pos, box, groups, _listing(kind, groups), rc, step, ls, 200, f"{name} {kind} matrix {matrix} step {step} ls {ls}",
                ref)
    if kind == "three":
        assert not got[0][1].any() and got[1][1] == got[2][1] == got[3][1] == 0      # the empty species


# ---- the edges of the tile, the item and the list --------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [63, 64, 65, 255, 256, 257])
def test_tile_and_item_edges(engine, n_atoms):
    pos = _walk("triclinic", n_atoms, 2)
    groups = [np.arange(n_atoms)]
    _held(engine, pos, Q.TRICLINIC, groups, None, 5.0 if n_atoms > 100 else 8.0, 1, (4, 6), 7, f"{n_atoms} centres")


@pytest.mark.parametrize("n_on", [0, 1, 2, 3, 63, 64])
def test_neighbour_counts_of_a_centre(engine, n_on):
    """a centre with exactly n_on atoms on a sphere around it; the atoms on the sphere bond to the centre alone, so each has
    one leg and q_l = 1, X = 2^24, the last bin.  64 legs: every lane holds one, 32 rounds, the last one counted once"""
    pos = Q.sphere(max(n_on, 1), 3.0)
    groups = [np.arange(1), np.arange(1, pos.shape[1])]
    listing = [np.asarray(g, np.int32) for g in groups]
    rc = np.array([[0.0, 3.5 if n_on else 0.0], [3.5 if n_on else 0.0, 0.0]])
    ref = C.reference(pos, Q.CUBIC, groups, rc, 1, [2, 4, 6])
    hist, trunc, iso, undef, x, n = _held(engine, pos, Q.CUBIC, groups, listing, rc, 1, (2, 4, 6), 1024, f"sphere of {n_on}", ref)
    assert n[0, 0] == n_on and not trunc.any() and not undef.any()
    if n_on == 0:
        assert np.array_equal(iso, [1, 1]) and np.all(x == -1) and not hist.any()
        return
    assert not iso.any() and np.all(n[0, 1:] == 1) and np.all(x[0, 1:] == C.ONE) and np.all(hist[1, :, 1023] == n_on)
    legs = pos[0, 1:].astype(np.float64) - pos[0, 0].astype(np.float64)
    known = n_on ** 2 * O.theorem(legs, [2, 4, 6])                          # the known sum, n + 2 sum P_l: what X was held to above
    assert np.abs(ref["xq"][0, 0] - known).max() <= 1e-9 * n_on ** 2
    if n_on == 1:
        assert np.all(x[0, 0] == C.ONE)


def test_sixty_five_neighbours_all_truncated(engine):
    pos = Q.ball(66, 2, 6.0)
    _resident(engine, pos)
    hist, trunc, iso, undef, x, n = engine.bond_order(Q.CUBIC, 6.0, (4, 6), 50, per_atom=True)
    assert trunc[0] == 2 * 66 and not hist.any() and not iso.any() and not undef.any() and np.all(x == -1) and np.all(n == 65)
    calc = _calculator(engine, pos, Q.CUBIC)
    with pytest.raises(ValueError, match="species 0: 132.*smaller r_cut"):
        calc.calculate_bond_order(6.0)


def test_coincident_pair(engine):
    """two atoms at one place: each has a leg of length 0, so every pair with that leg has no cosine and the two centres are
    undefined at every origin; every other centre is what the reference says (the two coincide as its neighbours: cos = 1)"""
    pos = _walk("cubic", 37, 12).copy()
    pos[:, 5] = pos[:, 9]
    groups = [np.arange(37)]
    ref = C.reference(pos, Q.CUBIC, groups, 8.0, 1, [4, 6])
    assert np.all(ref["why"][:, [5, 9]] == 3) and (ref["why"] == 3).sum() == 24
    hist, trunc, iso, undef, x, n = _held(engine, pos, Q.CUBIC, groups, None, 8.0, 1, (4, 6), 200, "coincident", ref)
    assert undef[0] == 24 and np.all(x[:, [5, 9]] == -1) and trunc[0] == 0


# ---- known structures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diamond", "fcc", "bcc8", "bcc14"])
def test_known_structures(engine, name):
    """every atom of a perfect lattice has the shell's q_l: X inside the allowance of the float64 value, the histogram one
    spike in the bin of the known q"""
    pos, rc, n_nb, known = {"diamond": (Q.diamond(2)[0], 2.8, 4, {3: 0.74536, 4: 0.50918, 6: 0.62854}),
                            "fcc": (C.fcc_block(), 4.6, 12, {3: 0.0, 4: 0.19094, 6: 0.57452, 8: 0.40391}),
                            "bcc8": (C.bcc_block(), 5.0, 8, {4: 0.50918, 6: 0.62854}),
                            "bcc14": (C.bcc_block(), 6.0, 14, {4: 0.03637, 6: 0.51069})}[name]
    ls, n_atoms = tuple(known), pos.shape[1]
    hist, trunc, iso, undef, x, n = _held(engine, pos, Q.CUBIC, [np.arange(n_atoms)], None, rc, 1, ls, 200, name)
    assert np.all(n == n_nb) and not (trunc.any() or iso.any() or undef.any())
    for j, l in enumerate(ls):
        spike = np.zeros(200, np.int64)
        spike[int(known[l] * 200)] = 2 * n_atoms
        assert np.array_equal(hist[0, j].astype(np.int64), spike), (name, l)


# ---- the histogram, the identities, the neighbours ----------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 7, 200, 1024])
def test_histogram_is_the_bin_rule(engine, n_q):
    pos, box, groups, rc, ref = _family_reference("triclinic130", "three", False, 1, (12,))
    _held(engine, pos, box, groups, _listing("three", groups), rc, 1, (12,), n_q, f"n_q {n_q}", ref)


def test_neighbour_counts_are_the_other_entries(engine):
    pos, box, r_cut = C.family("triclinic130")
    groups = Q.two_species(130)
    listing = _listing("two", groups)
    _resident(engine, pos)
    for rc in (r_cut, Q.matrix_cutoff(r_cut, 2)):
        n = engine.bond_order(box, rc, (6,), 10, listing, per_atom=True)[5]
        for f in range(pos.shape[0]):
            assert np.array_equal(n[f], engine.debug_neighbour_lists(box, rc, f, listing)[0])
    pairs = engine.pair_histogram(box, [0], r_cut, 1, listing)[0, :, :, 0].astype(np.int64)
    n = engine.bond_order(box, r_cut, (6,), 10, listing, per_atom=True)[5]
    assert n.sum() == pairs.sum() and n[:, :90].sum() == pairs[0].sum()


# ---- bit for bit ----------------------------------------------------------------------------------------------------------
def _equal(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def test_budgets_blocks_permutations_and_repeats(engine):
    from psa_amd import _hip
    pos, box, r_cut = C.family("cubic37")                                  # 40 frames
    n, T = pos.shape[1], pos.shape[0]
    groups = Q.two_species(n)
    listing = _listing("two", groups)
    rc = Q.matrix_cutoff(r_cut, 2)
    _resident(engine, pos)
    whole = engine.bond_order(box, rc, EIGHT, 200, listing, per_atom=True)
    assert whole[0].any() and _equal(whole, engine.bond_order(box, rc, EIGHT, 200, listing, per_atom=True))
    bare = engine.bond_order(box, rc, EIGHT, 200, listing)
    assert bare[4] is None and bare[5] is None and _equal(whole[:4], bare[:4])    # per_atom on and off: the same counts
    for origins in (1, 7, 39):                                             # origins per block: 40, 6 and 2 blocks
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, (PER_ORIGIN + 8 * len(EIGHT)) * n * origins + 5)
        assert _equal(whole, engine.bond_order(box, rc, EIGHT, 200, listing, per_atom=True)), origins
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n * origins + 5)
        assert _equal(whole[:4], engine.bond_order(box, rc, EIGHT, 200, listing)[:4]), origins
    reset(engine)
    rng = np.random.default_rng(8)
    perms = [rng.permutation(len(g)) for g in listing]
    moved = engine.bond_order(box, rc, EIGHT, 200, [g[p] for g, p in zip(listing, perms)], per_atom=True)
    assert _equal(whole[:4], moved[:4])
    at = np.concatenate([np.argsort(p) + s for p, s in zip(perms, (0, len(listing[0])))])   # undo: column of atom i after the shuffle
    assert np.array_equal(moved[4][:, at], whole[4]) and np.array_equal(moved[5][:, at], whole[5])
    # one species of all atoms is the sum over the two, with one cut-off
    two = engine.bond_order(box, r_cut, (4, 6), 200, listing)
    one = engine.bond_order(box, r_cut, (4, 6), 200)
    assert np.array_equal(one[0][0], two[0].sum(axis=0)) and one[2][0] == two[2].sum()
    assert whole[0].shape == (2, 8, 200) and T == 40


def test_walk_case_is_the_twin_exactly(engine):
    """`angle_cases.walk_case`, every branch of the centre walk: its five origins in blocks of 2, 2 and 1, and the five frames
    150 times over in one block -- 3 items x 750 origins are more workgroups than the 2047 that rows of 8 x 1024 + 3 words
    leave the partials, so a slab holds two origins and a wavefront walks on from one into the next.  The histogram, the
    centres left out and n are the twin's (order_cases.model), exactly; X is held to the float64 reference and the bin rule
    as everywhere else, and is the same bits in every blocking.

    X is not compared with the twin bit for bit: the twin rounds the square root under the cosine once, the kernel's comes
    from v_sqrt_f32 (within one ulp), and on this input 2577 of the 2800 X differ from the twin's, the first twenty by 10 to
    268 units of 2^-24 on X near 10^9"""
    from psa_amd import _hip
    pos, box, groups, rc = Q.walk_case()
    listing = [np.asarray(g, np.int32) for g in groups]
    want = C.model(pos, box, groups, rc, 1, EIGHT, 1024)
    assert Q.walk_counts(want[5]) and want[1].tolist() == [2, 0] and want[2].sum() == 10 and want[3].tolist() == [0, 4]
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, (PER_ORIGIN + 8 * len(EIGHT)) * 70 * 2 + 5)
    first = _held(engine, pos, box, groups, listing, rc, 1, EIGHT, 1024, "walk case, blocks of 2, 2 and 1")
    assert all(np.array_equal(first[i].astype(np.int64), want[i]) for i in (0, 1, 2, 3, 5))
    reset(engine)
    reps = 150
    _resident(engine, np.tile(pos, (reps, 1, 1)))
    got = engine.bond_order(box, rc, EIGHT, 1024, listing, per_atom=True)
    assert all(np.array_equal(g.astype(np.int64), reps * w) for g, w in zip(got[:4], want[:4]))
    assert np.array_equal(got[4], np.tile(first[4], (reps, 1, 1))) and np.array_equal(got[5], np.tile(want[5], (reps, 1)))


# ---- the calculator -------------------------------------------------------------------------------------------------------
def _calculator(engine, pos, box, types=None, dt=0.002):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, 1, 1, 1).attach(engine=engine)


def test_calculator(engine):
    from psa_amd import BondOrder
    pos, box, groups, rc, ref = _family_reference("cubic130", "two", True, 3, (1,))
    types = np.ones(130, np.int32)
    types[groups[1]] = 2
    calc = _calculator(engine, pos, box, types)
    res = calc.calculate_bond_order(rc, (1,), 50, basis_atom_types=[1, 2], origin_step=3, per_atom=True)
    assert isinstance(res, BondOrder) and all(np.array_equal(a, b) for a, b in zip(res.groups, groups))
    raw = engine.bond_order(box, rc, (1,), 50, _listing("two", groups), origin_step=3, per_atom=True)
    assert np.array_equal(res.counts, raw[0]) and np.array_equal(res.neighbours, raw[5]) and res.origins == 4
    kept = raw[4][..., 0] >= 0
    assert np.array_equal(np.isnan(res.q_atoms[..., 0]), ~kept) and C.check(raw[4], raw[5], ref, "calculator")
    assert np.array_equal(res.q_atoms[kept], np.sqrt(raw[4][kept] / (raw[5][kept][:, None].astype(np.float64) ** 2 * C.ONE)))
    assert np.array_equal(res.samples, [4 * 90, 4 * 40]) and np.array_equal(res.atoms, np.concatenate(groups))
    assert np.allclose(res.mean[0], res.q_atoms[:, :90][kept[:, :90]].mean(axis=0)) and res.mean.shape == (2, 1)
    assert np.allclose((res.density * 0.02).sum(axis=2)[res.counts.sum(axis=2) > 0], 1.0)
    plain = calc.calculate_bond_order(6.0)
    assert plain.counts.shape == (1, 2, 200) and np.array_equal(plain.ls, [4, 6]) and plain.q_atoms is None and plain.mean is None
    assert plain.order(6) == 1 and plain.origins == 12


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _raw_call(engine):
    """(call(**changes) -> return code, refused(rc, word)) on ten atoms in two species of the triclinic walk"""
    lib, h = engine._lib, engine._h
    f64p, i32p, i64p, u64p = (Ct.POINTER(t) for t in (Ct.c_double, Ct.c_int32, Ct.c_int64, Ct.c_uint64))
    H, inv = (np.ascontiguousarray(a) for a in R.box64(Q.TRICLINIC))
    idx = np.arange(10, dtype=np.int32)
    start = np.array([0, 4, 10], np.int64)
    rc = np.array([[5.0, 4.0], [4.0, 0.0]])
    orders = np.array([4, 6], np.int32)
    hist, out = np.empty((2, 2, 45), np.uint64), [np.empty(2, np.uint64) for _ in range(3)]
    x, n = np.empty((12, 10, 2), np.int64), np.empty((12, 10), np.int32)

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)

    def call(box=H, binv=inv, ix=idx, st=start, G=2, r=rc, step=1, ls=orders, n_ls=2, n_q=45, hi=hist, hbytes=None, t=out[0], i=out[1],
             u=out[2], xs=x, ns=n):
        return lib.psa_bond_order(h, ptr(box, f64p), ptr(binv, f64p), ptr(ix, i32p), ptr(st, i64p), G, ptr(r, f64p), step, ptr(ls, i32p),
                                  n_ls, n_q, ptr(hi, u64p), hist.nbytes if hbytes is None else hbytes, ptr(t, u64p), ptr(i, u64p),
                                  ptr(u, u64p), ptr(xs, i64p), ptr(ns, i32p))

    def refused(rc_, word):
        msg = lib.psa_last_error().decode()
        assert rc_ == -1 and word in msg, (rc_, msg)
    return call, refused, H, inv, hist


def test_refusals(engine):
    from psa_amd import _hip, max_pair_radius
    _resident(engine, _walk("triclinic", 37, 12))
    call, refused, H, inv, hist = _raw_call(engine)
    served = max_pair_radius(Q.TRICLINIC)
    assert call() == 0 and call(xs=None) == 0 and call(ns=None) == 0 and call(xs=None, ns=None) == 0
    singular = H.copy()
    singular[2] = singular[0] + singular[1]
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
    refused(call(r=np.array([[served * 1.001, 4.0], [4.0, 0.0]])), "served radius")
    refused(call(G=0), "groups")
    refused(call(G=9), "groups")
    refused(call(st=np.array([0, 6, 4], np.int64)), "ascending")
    refused(call(ix=None), "n_groups must be 1")
    refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 37], np.int32)), "out of bounds")
    refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 3], np.int32)), "twice")
    refused(call(step=0), "origin_step")
    for what in ("hi", "t", "i", "u"):
        refused(call(**{what: None}), "null output")
    refused(call(ls=None), "null ls")
    refused(call(n_ls=0), "number of orders")
    refused(call(ls=np.arange(1, 10, dtype=np.int32), n_ls=9), "number of orders")
    refused(call(ls=np.array([0, 6], np.int32)), "outside [1, 12]")
    refused(call(ls=np.array([4, 13], np.int32)), "outside [1, 12]")
    refused(call(ls=np.array([4, 4], np.int32)), "strictly ascending")
    refused(call(ls=np.array([6, 4], np.int32)), "strictly ascending")
    refused(call(n_q=0, hbytes=0), "number of bins")
    refused(call(n_q=1025, hbytes=2 * 2 * 1025 * 8), "number of bins")
    refused(call(hbytes=hist.nbytes - 8), "hist_bytes")
    refused(call(n_ls=1), "hist_bytes")
    # a budget below one origin names the bytes: 1040 per atom, and 8 per order more with x
    assert call() == 0
    keep = hist.copy()
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, (PER_ORIGIN + 16) * 10 - 1)
    refused(call(), f"need {(PER_ORIGIN + 16) * 10} bytes")
    assert call(xs=None) == 0 and np.array_equal(hist, keep)
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * 10 - 1)
    refused(call(xs=None), f"need {PER_ORIGIN * 10} bytes")
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, (PER_ORIGIN + 16) * 10)
    assert call() == 0 and np.array_equal(hist, keep)
    with pytest.raises(_hip.PsaHipError, match="strictly ascending"):
        engine.bond_order(Q.TRICLINIC, 5.0, (6, 4), 45)
    engine.release(_hip.SLOT_POSITIONS)
    engine.invalidate(_hip.SLOT_POSITIONS)
    refused(call(), "positions slot holds no array")


def test_sharded_context_is_refused(engine):
    """a context that holds a communicator (one rank is enough) is refused, and serves again once the communicator is gone"""
    _resident(engine, _walk("triclinic", 37, 12))
    call, refused, *_ = _raw_call(engine)
    assert call() == 0
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        got = (call(), engine._lib.psa_last_error().decode())
    finally:
        engine.comm_destroy()
    assert got[0] == -1 and "sharded context" in got[1] and "psa_bond_order" in got[1], got
    assert call() == 0


# ---- no trace -----------------------------------------------------------------------------------------------------------
def test_no_trace_in_the_other_entry_points(engine):
    """`angle_histogram` and `pair_histogram` give the bits they gave before the order calls in between (they share the work
    buffer, the item table, the partials and the accumulator); atom weights and segments set on the context change nothing;
    the stage times are where the header says"""
    from psa_amd import Segments
    pos, box, r_cut = C.family("cubic37")
    _resident(engine, pos)

    def others():
        return (*engine.angle_histogram(box, r_cut, 45), engine.pair_histogram(box, [0, 3], 0.25, 40))
    before = others()
    engine.timings()                                                       # (reset)
    first = engine.bond_order(box, r_cut, EIGHT, 1024, per_atom=True)
    t = engine.timings()
    assert t["gather"] > 0 and t["transpose"] > 0 and t["phase"] > 0 and t["epilogue"] > 0 and t["d2h"] > 0
    assert t["fft"] == 0 and t["project"] == 0
    for a, b in zip(before, others()):
        assert np.array_equal(a, b)
    engine.set_atom_weights(np.linspace(0.5, 2.0, 37).astype(np.float32))
    engine.set_segments(Segments(8, 4, "hann"))
    assert _equal(first, engine.bond_order(box, r_cut, EIGHT, 1024, per_atom=True))
