"""The self-overlap on the GPU (psa_self_overlap, Engine.self_overlap, SEDCalculator.calculate_overlap) through the C ABI
against the float64 reference of tests/overlap64.py inside the allowance of tests/overlap_cases.py: every element of the
per-origin table, the sums as exact sums of that table, the identity with psa_van_hove_self, the edges of the origin
tiles and of the origin step, the exact families (lattice walk, cooperative motion, frozen atoms), the far family,
blockings and repeats, 256 lags, no trace in later calls, poisoned scratch, the calculator path, every refusal."""
import ctypes as Ct
import functools
from fractions import Fraction

import numpy as np
import pytest

import msd64 as R
import msd_cases as M
import overlap64 as O
import overlap_cases as OC
import scratch_cases
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = {"cubic": M.CUBIC, "triclinic": M.TRICLINIC}
T = 250
LAGS = [0, 1, 7, 33, T - 1]
CUTOFFS = (1.0, 4.0, 12.0)
STEPS = (1, 3, 7, 249, 400)


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


def _calculator(engine, pos, box, types=None, dt=0.002):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, 1, 1, 1).attach(engine=engine)


@functools.lru_cache(maxsize=None)
def _walk(box, n_atoms, n_frames=T, seed=21):
    wrapped, unwrapped, _, _ = M.random_walk(n_atoms, n_frames, seed=seed, box=BOXES[box])
    assert M.tie_free(wrapped, BOXES[box])
    u, n, S = R.unwrap64(wrapped, BOXES[box])
    return dict(pos=wrapped, unwrapped=unwrapped, u=u, n=n, S=S, box=BOXES[box])


def _listing(kind, n_atoms, seed=3):
    """(groups for the engine, or None: all atoms)"""
    if kind == "all":
        return None
    order = np.random.default_rng(seed).permutation(n_atoms).astype(np.int32)
    if kind == "shuffled":
        return [order[: n_atoms - 5]]
    return [order[: n_atoms // 3], np.zeros(0, np.int32), order[n_atoms // 3: n_atoms - 2]]


def _groups(listing, n_atoms):
    return [np.arange(n_atoms)] if listing is None else listing


def _held(engine, w, listing, lags, cutoff, step, what, van_hove=True, **kw):
    """one call with the table: every element within its allowance, the sums exactly those of the table, the same sums
    without the table, S1 the van Hove count.  Returns (sums, table, borderline, total)"""
    groups = _groups(listing, w["u"].shape[1])
    Q, S1, S2 = O.overlap64(w["u"], groups, lags, step, cutoff)
    allowed, borderline, total = OC.allowance(w["u"], w["S"], groups, lags, step, cutoff)
    sums, table = engine.self_overlap(w["box"], lags, cutoff, listing, step, per_origin=True, **kw)
    assert sums.dtype == np.uint64 and sums.shape == (len(lags), len(groups), 2)
    assert table.dtype == np.uint32 and table.shape == Q.shape
    moved = int(np.abs(table.astype(np.int64) - Q).sum())
    print(f"{what}: {borderline} borderline of {total}, {moved} moved")
    assert OC.inside(table, Q, allowed), what
    t = table.astype(np.uint64)
    assert np.array_equal(sums[:, :, 0], t.sum(axis=2)) and np.array_equal(sums[:, :, 1], (t * t).sum(axis=2)), what
    for j, lag in enumerate(lags):
        assert not table[j, :, R.n_origins(w["u"].shape[0], int(lag), step):].any(), what
    plain, none = engine.self_overlap(w["box"], lags, cutoff, listing, step, **kw)
    assert none is None and np.array_equal(plain, sums), what
    if van_hove:
        for j0 in range(0, len(lags), 64):
            vh = engine.van_hove_self(w["box"], lags[j0:j0 + 64], cutoff, 1, listing, step, **kw)
            assert np.array_equal(vh[:, :, 0], sums[j0:j0 + 64, :, 0]), what
    return sums, table, borderline, total


# ---- the random walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all", "shuffled", "three"])
@pytest.mark.parametrize("n_atoms", [37, 130])
@pytest.mark.parametrize("box", BOXES)
def test_random_walk(engine, box, n_atoms, kind):
    w = _walk(box, n_atoms)
    _resident(engine, w["pos"])
    listing = _listing(kind, n_atoms)
    borderline = total = 0
    for cutoff in CUTOFFS:
        for step in STEPS:
            sums, table, b, t = _held(engine, w, listing, LAGS, cutoff, step, f"walk {box} {n_atoms} {kind} a {cutoff} step {step}")
            borderline, total = borderline + b, total + t
            if kind == "three":
                assert not sums[:, 1].any() and not table[:, 1].any()
    assert borderline <= 1e-3 * total                                         # the reference alone


def test_random_walk_is_not_degenerate(engine):
    """at a = 4.0 q runs from 1 to 0 over the lags and chi4(7) is of order 0.2"""
    w = _walk("cubic", 130)
    calc = _calculator(engine, w["pos"], w["box"])
    r = calc.calculate_overlap(LAGS, 4.0)
    q, chi = r.q[:, 0], r.chi4[:, 0]
    print("q", q, "chi4", chi)
    assert q[0] == 1.0 and q[1] > 0.99 and 0.3 < q[2] < 0.5 and q[3] < 0.1 and q[4] < 0.05
    assert 0.1 < chi[2] < 0.4 and chi[0] == 0.0 and r.peak()[0][0] == r.times[int(np.argmax(chi))]


# ---- tile edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2, 5])
def test_tile_edges(engine, step):
    """T = 1500 crosses the origin tiles (1024, 513 and 205 origins at steps 1, 2, 5) and the 256-origin pieces of a tile;
    the lags 255 / 256 / 257 end inside different pieces, lag 1499 has one origin"""
    w = _walk("triclinic", 20, 1500)
    _resident(engine, w["pos"])
    listing = [np.arange(0, 20, 2, dtype=np.int32), np.arange(1, 20, 2, dtype=np.int32)]
    _held(engine, w, listing, [0, 255, 256, 257, 1499], 4.0, step, f"tile edges step {step}")
    _held(engine, w, listing, [257, 1499], 4.0, step, f"tile edges step {step}, n_o_max of lag 257")


# ---- exact families -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unwrap", [True, False])
@pytest.mark.parametrize("cutoff", [0.6, 0.5])
def test_lattice_walk_is_exact(engine, cutoff, unwrap):
    """steps of 0.25 on a lattice: no rounding anywhere (tests/overlap_cases.py); at a = 0.5, |D| = 0.5 exactly is not counted"""
    pos = OC.lattice_walk(23, T, seed=8)
    _resident(engine, pos)
    u = R.unwrap64(pos, M.CUBIC)[0]
    listing = [np.arange(0, 23, 2, dtype=np.int32), np.arange(1, 23, 2, dtype=np.int32)]
    lags = [0, 1, 2, 5, 40]
    for step in (1, 3):
        Q, S1, S2 = O.overlap64(u, listing, lags, step, cutoff)
        sums, table = engine.self_overlap(M.CUBIC, lags, cutoff, listing, step, unwrap=unwrap, per_origin=True)
        assert np.array_equal(table, Q) and np.array_equal(sums[:, :, 0], S1) and np.array_equal(sums[:, :, 1], S2)
        assert np.array_equal(engine.van_hove_self(M.CUBIC, lags, cutoff, 1, listing, step, unwrap=unwrap)[:, :, 0], S1)
    D = R.displacements(u, np.arange(23), 2)
    assert ((D * D).sum(axis=2) == 0.25).sum() > 100


def test_cooperative_motion(engine):
    """all atoms share one walk: Q is 0 or N_g at every origin, so chi4 = N_g q (1 - q) as rationals"""
    pos = OC.lattice_walk(24, T, seed=9, cooperative=True)
    calc = _calculator(engine, pos, M.CUBIC)
    groups = [np.arange(0, 10), np.arange(10, 24)]
    r = calc.calculate_overlap([1, 2, 3, 9], 0.5, basis_atom_indices=[list(g) for g in groups], per_origin=True)
    for g, members in enumerate(groups):
        assert set(np.unique(r.q_origins[:, g])) <= {0, members.size}
        for j in range(4):
            n_o, n_g = int(r.origins[j]), members.size
            q = Fraction(int(r.sum[j, g]), n_o * n_g)
            assert O.chi4_fraction(r.sum[j, g], r.sum_squares[j, g], n_o, n_g) == n_g * q * (1 - q)
            assert r.chi4[j, g] == float(n_g * q * (1 - q)) and r.q[j, g] == float(q)
    assert 0 < r.q[1, 0] < 1                                                  # neither all nor nothing


@pytest.mark.parametrize("box", BOXES)
def test_frozen_atoms(engine, box):
    pos = M.frozen(9, T, seed=6, box=BOXES[box])
    calc = _calculator(engine, pos, BOXES[box])
    for cutoff in (0.3, 1e-30):
        r = calc.calculate_overlap([0, 7, T - 1], cutoff, origin_step=3, per_origin=True)
        for j, n_o in enumerate(r.origins):
            assert np.all(r.q_origins[j, 0, :n_o] == 9) and not r.q_origins[j, 0, n_o:].any()
        assert np.array_equal(r.sum[:, 0], 9 * r.origins) and np.array_equal(r.sum_squares[:, 0], 81 * r.origins)
        assert np.all(r.q == 1.0) and not r.chi4.any()


# ---- the far family -----------------------------------------------------------------------------------------------------
def test_far_family(engine):
    """|u| reaches 1e3 where a lag-1 displacement is 0.03: one atom per group and two origins (0 and T - 16) show single
    samples, where float32 storage of u or the wrong tile origin would leave the allowance (tests/test_overlap_host.py)"""
    n_t, n_atoms = 40000, 8
    pos = M.far(n_atoms, n_t, seed=4)
    u, n, S = R.unwrap64(pos, M.CUBIC)
    assert not n.any() and np.abs(u[-1]).max() > 500.0
    _resident(engine, pos)
    w = dict(u=u, S=S, box=M.CUBIC)
    groups = [np.array([a], np.int32) for a in range(n_atoms)]
    lags = list(range(1, 16))
    for cutoff in (0.1, 0.2):
        sums, table, _, _ = _held(engine, w, groups, lags, cutoff, n_t - 16, f"far a {cutoff}")
        assert 0.1 < table.sum() / (8 * 2 * 15) < 0.9
        same, _ = engine.self_overlap(M.CUBIC, lags, cutoff, groups, n_t - 16, unwrap=False)
        assert np.array_equal(same, sums)


# ---- input forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", BOXES)
def test_wrapped_and_unwrapped_input(engine, box):
    """the unwrapped twin of the wrapped walk: within the allowance of its own reference, with and without the image
    search, which finds nothing there and so gives the same bits"""
    w = _walk(box, 37)
    uu, nu, Su = R.unwrap64(w["unwrapped"], w["box"])
    assert not nu.any() and np.abs(w["n"]).max() >= 1
    _resident(engine, w["unwrapped"])
    twin = dict(u=uu, S=Su, box=w["box"])
    a, _, _, _ = _held(engine, twin, None, LAGS, 4.0, 3, f"unwrapped twin {box}")
    b, _, _, _ = _held(engine, twin, None, LAGS, 4.0, 3, f"unwrapped twin {box}, unwrap=0", unwrap=False)
    assert np.array_equal(a, b)


# ---- blockings, repeats, many lags ---------------------------------------------------------------------------------------
def test_budgets_and_repeats(engine):
    from psa_amd import _hip
    w = _walk("triclinic", 37)
    _resident(engine, w["pos"])
    listing = _listing("three", 37)
    whole = engine.self_overlap(w["box"], LAGS, 4.0, listing, 3, per_origin=True)
    again = engine.self_overlap(w["box"], LAGS, 4.0, listing, 3, per_origin=True)
    assert np.array_equal(whole[0], again[0]) and np.array_equal(whole[1], again[1])
    table_bytes = whole[1].nbytes
    for atoms in (1, 5, 11):
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, table_bytes + 24 * T * atoms + 7)
        cut = engine.self_overlap(w["box"], LAGS, 4.0, listing, 3, per_origin=True)
        assert np.array_equal(cut[0], whole[0]) and np.array_equal(cut[1], whole[1]), atoms
        for g, members in enumerate(listing):                                 # group by group the one-group calls
            one = engine.self_overlap(w["box"], LAGS, 4.0, [members], 3)[0]
            assert np.array_equal(one[:, 0], whole[0][:, g]), (atoms, g)


def test_256_lags_in_one_call(engine):
    from psa_amd import _hip
    assert _hip.OVERLAP_MAX_LAGS == 256
    w = _walk("cubic", 37)
    _resident(engine, w["pos"])
    lags = [int(t) for t in (np.arange(256) * 7) % T]                         # every order, duplicates among them
    assert len(set(lags)) < 256 and min(lags) == 0
    _held(engine, w, _listing("three", 37), lags, 4.0, 2, "256 lags")


# ---- no trace, poisoned scratch -------------------------------------------------------------------------------------------
def test_no_disturbance_of_the_other_entry_points(engine):
    """`calculate_msd`, `calculate_van_hove` and `calculate_self_spectra` give the bits they gave before the overlap calls
    in between; the stage times are where the header says"""
    from psa_amd import commensurate_vectors
    w = _walk("cubic", 37)
    calc = _calculator(engine, w["pos"], w["box"])
    half = commensurate_vectors(w["box"], 1.2, 0.1)[0][:12]

    def others():
        return (calc.calculate_msd(lags=60).msd, calc.calculate_van_hove([1, 30], 6.0, 48).counts,
                calc.calculate_self_spectra(half).density)
    before = others()
    engine.timings()                                                          # (reset)
    r = calc.calculate_overlap(LAGS, 4.0, per_origin=True)
    t = engine.timings()
    assert t["gather"] > 0 and t["transpose"] > 0 and t["epilogue"] > 0 and t["d2h"] > 0 and t["fft"] == 0 and t["project"] == 0
    calc.calculate_overlap([5], 1.0, origin_step=4)
    for a, b in zip(before, others()):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    again = calc.calculate_overlap(LAGS, 4.0, per_origin=True)
    assert np.array_equal(again.sum, r.sum) and np.array_equal(again.sum_squares, r.sum_squares)
    assert np.array_equal(again.q_origins, r.q_origins)


def test_scratch_history(engine):
    """no result depends on what the scratch memory held: a table that is not zeroed, or a partial read beyond a lag's
    origins, fails here"""
    def call(engine, loud=False):
        from psa_amd import _hip
        scratch_cases.prepare(engine)
        engine.ensure_resident(_hip.SLOT_POSITIONS, scratch_cases.walk(loud))
        groups = scratch_cases.species_of(loud)
        return scratch_cases._copy(engine.self_overlap(scratch_cases.BOX, [0, 3, 50] if loud else [0, 5, 99], 3.0, groups, 2, True,
                                                       per_origin=True))
    r0 = call(engine)
    assert r0[0].any() and r0[1].any()
    scratch_cases.compare("self_overlap", "repeated", r0, call(engine))
    scratch_cases.check_poisoned(engine, "self_overlap", call, r0)
    call(engine, loud=True)                                                   # a larger call of the same entry before
    scratch_cases.compare("self_overlap", "after a loud call", r0, call(engine))
    for name, other in (("van_hove_self", scratch_cases.CASES["van_hove_self"][1]),
                        ("displacement_moments unwrap", scratch_cases.CASES["displacement_moments unwrap"][1])):
        v0 = other(engine)
        call(engine, loud=True)
        scratch_cases.compare(name, "after a loud self_overlap", v0, other(engine))


# ---- the calculator path --------------------------------------------------------------------------------------------------
def test_calculator_path_and_draws(engine):
    from psa_amd import DynamicOverlap, draw_atoms
    w = _walk("triclinic", 130)
    types = (np.arange(130) % 3 + 1).astype(np.int32)
    calc = _calculator(engine, w["pos"], w["box"], types)
    r = calc.calculate_overlap([1, 20, 7], 4.0, basis_atom_types=[1, 3], origin_step=2, max_atoms=10, seed=5, per_origin=True)
    want = [draw_atoms(np.flatnonzero(types == s), 10, 5) for s in (1, 3)]
    assert isinstance(r, DynamicOverlap) and all(np.array_equal(a, b) for a, b in zip(r.groups, want))
    assert np.array_equal(r.counts, [10, 10]) and np.array_equal(r.origins, (T - 1 - np.array([1, 20, 7])) // 2 + 1)
    assert np.array_equal(r.lag_frames, [1, 20, 7]) and np.allclose(r.times, 0.002 * np.array([1, 20, 7])) and r.cutoff == 4.0
    sums, table = engine.self_overlap(np.asarray(w["box"], np.float32).astype(np.float64), [1, 20, 7], 4.0, want, 2, per_origin=True)
    assert np.array_equal(r.sum, sums[:, :, 0]) and np.array_equal(r.sum_squares, sums[:, :, 1]) and np.array_equal(r.q_origins, table)
    Q = O.overlap64(w["u"], want, [1, 20, 7], 2, 4.0)[0]
    allowed = OC.allowance(w["u"], w["S"], want, [1, 20, 7], 2, 4.0)[0]
    assert OC.inside(r.q_origins, Q, allowed)
    for j in range(3):
        for g in range(2):
            assert r.chi4[j, g] == float(O.chi4_fraction(r.sum[j, g], r.sum_squares[j, g], r.origins[j], 10))
    assert r.relaxation_time().shape == (2,) and r.peak()[0].shape == (2,)
    v = calc.calculate_van_hove([1, 20, 7], 4.0, 1, basis_atom_types=[1, 3], origin_step=2, max_atoms=10, seed=5)
    assert np.array_equal(v.counts[:, :, 0], r.sum)
    assert calc.calculate_overlap([3], 4.0).q_origins is None


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    from psa_amd import _hip
    w = _walk("triclinic", 37)
    _resident(engine, w["pos"])
    lib, h = engine._lib, engine._h
    f64p, i32p, i64p = Ct.POINTER(Ct.c_double), Ct.POINTER(Ct.c_int32), Ct.POINTER(Ct.c_int64)
    u64p, u32p = Ct.POINTER(Ct.c_uint64), Ct.POINTER(Ct.c_uint32)
    H, inv = R.box64(w["box"])
    H, inv = np.ascontiguousarray(H), np.ascontiguousarray(inv)
    idx = np.arange(10, dtype=np.int32)
    start = np.array([0, 4, 10], np.int64)
    lags = np.array([5, 0], np.int64)
    out, tab = np.empty((2, 2, 2), np.uint64), np.empty((2, 2, T), np.uint32)

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)

    def refused(rc, word):
        msg = lib.psa_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def ov(box=H, binv=inv, ix=idx, st=start, G=2, lg=lags, n=2, step=1, unwrap=1, a=0.5, o=out, nbytes=None, t=tab, tbytes=None):
        return lib.psa_self_overlap(h, ptr(box, f64p), ptr(binv, f64p), ptr(ix, i32p), ptr(st, i64p), G, ptr(lg, i64p), n, step, unwrap,
                                    a, ptr(o, u64p), out.nbytes if nbytes is None else nbytes, ptr(t, u32p),
                                    (0 if t is None else tab.nbytes) if tbytes is None else tbytes)

    assert ov() == 0 and ov(t=None) == 0
    singular = H.copy()
    singular[2] = singular[0] + singular[1]
    refused(ov(box=None), "null")
    refused(ov(binv=None), "null")
    refused(ov(o=None), "null")
    refused(ov(lg=None), "null")
    refused(ov(box=singular), "singular")
    refused(ov(binv=2.0 * inv), "not the inverse")
    refused(ov(box=H * np.nan), "finite")
    refused(ov(unwrap=2), "unwrap")
    refused(ov(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 37], np.int32)), "out of bounds")
    refused(ov(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1], np.int32)), "out of bounds")
    refused(ov(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 3], np.int32)), "twice")
    refused(ov(G=0), "groups")
    refused(ov(G=9), "groups")
    refused(ov(st=None), "null")
    refused(ov(st=np.array([1, 4, 10], np.int64)), "must be 0")
    refused(ov(st=np.array([0, 6, 4], np.int64)), "ascending")
    refused(ov(ix=None), "n_groups must be 1")
    refused(ov(step=0), "origin_step")
    refused(ov(nbytes=8), "out_bytes")
    refused(ov(tbytes=8), "origins_bytes")
    refused(ov(t=None, tbytes=8), "origins_bytes")
    refused(ov(n=0), "number of lags")
    refused(ov(n=257), "number of lags")
    refused(ov(lg=np.array([0, T], np.int64)), "outside [0, T - 1")
    refused(ov(lg=np.array([-1, 3], np.int64)), "outside [0, T - 1")
    for a in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
        refused(ov(a=a), "cut-off")
    # the table's size follows the smallest lag
    assert ov(lg=np.array([5, 9], np.int64), tbytes=2 * 2 * (T - 5) * 4) == 0
    refused(ov(lg=np.array([5, 9], np.int64)), "origins_bytes")
    # a budget that cannot hold the table beside one atom says what to change
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, tab.nbytes + 24 * T - 1)
    refused(ov(), "a larger origin_step or fewer lags")
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, tab.nbytes + 24 * T)
    assert ov() == 0
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * T - 1)
    refused(ov(), f"need {24 * T} bytes")
    engine.reset_options()
    # every group empty: zeros
    out[:], tab[:] = 7, 7
    assert ov(st=np.array([0, 0, 0], np.int64)) == 0 and not out.any() and not tab.any()
    # no positions resident
    engine.release(_hip.SLOT_POSITIONS)
    engine.invalidate(_hip.SLOT_POSITIONS)
    refused(ov(), "positions slot holds no array")


def test_sharded_context_is_refused(engine):
    """a context that holds a communicator (one rank is enough) is refused, and serves again once it is gone"""
    w = _walk("triclinic", 37)
    _resident(engine, w["pos"])

    def call():
        return engine.self_overlap(w["box"], [0, 5], 4.0)[0]
    first = call()
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        with pytest.raises(Exception, match="sharded context") as e:
            call()
    finally:
        engine.comm_destroy()
    assert "psa_self_overlap" in str(e.value)
    assert np.array_equal(call(), first)
