"""The bond persistence on the GPU (psa_bond_persistence, Engine.bond_persistence and the calculator method).  Every comparison
is of integers: the counts against the float64 reference of tests/persist64.py inside the allowance of tests/persist_cases.py
on the families of angle_cases (one, two and three species, the matrix of cut-offs with its zero entry, with and without
hysteresis, origin steps 1, 3 and above T, sample steps 1 and 2, continuous on and off) and on angle_cases.walk_case; closed
forms that need no reference (a frozen trajectory, a dimer that leaves and returns, a dimer that oscillates between r_cut and
r_break, the diamond lattice); the exact identities of the definition on every case, the agreement of lag 0 with
psa_angle_histogram and of every mask bit with psa_debug_neighbour_lists; the same bits for any budget, for repeated calls and
for a permutation of the atoms; poisoned scratch; every refusal; no trace in later calls; the calculator."""
import functools

import numpy as np
import pytest

import angle_cases as Q
import pair_cases as P
import persist_cases as C
import scratch_cases as S
from engine_state import reset

pytestmark = pytest.mark.gpu

PER_ORIGIN = 1040 + 288                                                    # work bytes per atom and origin
# (the matrix of cut-offs?, r_break / r_cut, origin_step -- None: above T --, sample_step, continuous)
CONFIGS = [(False, 1.0, 1, 1, True), (True, C.HYSTERESIS, 1, 1, True), (False, C.HYSTERESIS, 3, 2, True), (True, 1.0, None, 1, False),
           (False, C.HYSTERESIS, 1, 2, False)]


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


def _listing(groups):
    return [np.asarray(g, np.int32) for g in groups]


def _call(engine, box, r_cut, lags, listing, step=1, r_break=None, ss=1, cont=True, per_atom=True):
    return engine.bond_persistence(box, r_cut, lags, listing, step, r_break=r_break, sample_step=ss, continuous=cont, per_atom=per_atom)


def _popcount(masks):
    m = np.ascontiguousarray(masks, np.uint64)
    return np.unpackbits(m.view(np.uint8).reshape(m.shape + (8,)), axis=-1).sum(axis=-1, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _frames(name, kind):
    pos, box, rc = Q.family(name)
    groups = C.species(kind, pos.shape[1])
    return pos, box, rc, groups, C.Frames(pos, box, groups)


@functools.lru_cache(maxsize=None)
def _case(name, kind, config):
    """the inputs of a configuration of a family and their reference, computed once"""
    matrix, factor, step, ss, cont = config
    pos, box, rc, groups, frames = _frames(name, kind)
    T = pos.shape[0]
    r_cut = C.cutoffs(kind, rc, matrix)
    r_break = C.breaks(r_cut, factor)
    step = T + 1 if step is None else step
    lags = C.lags_of(T, ss)
    return pos, box, groups, r_cut, r_break, lags, step, ss, cont, C.reference(pos, box, groups, r_cut, r_break, lags, step, ss, cont, frames)


def _exact(engine, got, box, r_cut, listing, sizes, T, lags, step, cont, what):
    """the exact identities on a result with per-atom masks: those of the counts, lag 0 against psa_angle_histogram, the masks'
    popcounts against the counts"""
    assert C.identities(got, sizes, T, lags, step, cont), what
    for k in C.KEYS:
        assert got[k].dtype == np.uint64
    if 0 in lags:
        _, coord, trunc = engine.angle_histogram(box, r_cut, 1, listing, step)
        j = list(lags).index(0)
        assert np.array_equal((coord * np.arange(65, dtype=np.uint64)).sum(axis=2, dtype=np.uint64), got["bonds"][j]), what
        assert np.array_equal(trunc, got["truncated"][j]), what
    start = np.concatenate([[0], np.cumsum(sizes)])
    n_o0 = (T - 1) // step + 1
    assert got["alive_masks"].shape == got["unbroken_masks"].shape == (len(lags), n_o0, start[-1])
    for key, masks in (("alive", got["alive_masks"]), ("unbroken", got["unbroken_masks"])):
        pop = _popcount(masks)
        for a in range(len(sizes)):
            assert np.array_equal(pop[:, :, start[a]:start[a + 1]].sum(axis=(1, 2)), got[key][:, a].sum(axis=1).astype(np.int64)), (what, key)
    assert not (got["unbroken_masks"] & ~got["alive_masks"]).any() or not cont
    for j, lag in enumerate(lags):                                         # an origin outside O_tau: 0
        assert not got["alive_masks"][j, (T - 1 - lag) // step + 1:].any(), what


# ---- 1. against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("kind", ["one", "two", "three"])
@pytest.mark.parametrize("name", list(Q.FAMILIES))
def test_against_the_reference(engine, name, kind, config):
    pos, box, groups, r_cut, r_break, lags, step, ss, cont, ref = _case(name, kind, config)
    assert ref["borderline"] <= C.BORDERLINE_CAP * max(ref["events"], 1) and ref["bonds"].sum() > 100 and ref["most"] <= C.CAPACITY
    assert (ref["alive"] < ref["bonds"]).any() or max(lags) == 0          # something breaks: before the GPU is touched
    _resident(engine, pos)
    listing = _listing(groups)
    what = f"{name} {kind} {config}"
    got = _call(engine, box, r_cut, lags, listing, step, r_break, ss, cont)
    assert C.check(got, ref, what)
    _exact(engine, got, box, r_cut, listing, [len(g) for g in groups], pos.shape[0], lags, step, cont, what)
    if not cont:
        assert not got["unbroken"].any() and not got["unbroken_masks"].any()
    else:                                                                  # continuous=False leaves alive and lost the same bits
        bare = _call(engine, box, r_cut, lags, listing, step, r_break, ss, False, per_atom=False)
        assert all(np.array_equal(bare[k], got[k]) for k in ("bonds", "alive", "lost", "truncated")) and bare["alive_masks"] is None


@pytest.mark.parametrize("name,kind", [("cubic37", "two"), ("triclinic130", "three")])
def test_mask_bits_pair_with_the_neighbour_lists(engine, name, kind):
    """bit i of a mask is the i-th entry of psa_debug_neighbour_lists at the origin: every bit against the float64 distance of
    that very pair at the later frame (no event of these inputs is borderline)"""
    config = (True, C.HYSTERESIS, 3, 1, True)
    pos, box, groups, r_cut, r_break, lags, step, ss, cont, ref = _case(name, kind, config)
    assert ref["borderline"] == 0
    _, _, _, _, frames = _frames(name, kind)
    _resident(engine, pos)
    listing = _listing(groups)
    got = _call(engine, box, r_cut, lags, listing, step, r_break, ss, cont)
    brk = np.asarray(r_break)[frames.spec[:, None], frames.spec[None, :]]
    rows = np.arange(frames.n)[:, None]
    seen = 0
    for k, o in enumerate(range(0, pos.shape[0], step)):
        count, lists = engine.debug_neighbour_lists(box, r_cut, o, listing)
        held = np.arange(64)[None, :] < count[:, None]
        col = np.where(held, lists, 0)
        for j, lag in enumerate(lags):
            if o + lag > pos.shape[0] - 1:
                continue
            up = held & (frames.r[o + lag][rows, col] < brk[rows, col])
            whole = held.copy()
            for v in range(ss, lag + 1, ss):
                whole &= frames.r[o + v][rows, col] < brk[rows, col]
            bits = (got["alive_masks"][j, k][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
            assert np.array_equal(bits.astype(bool), up), (o, lag)
            bits = (got["unbroken_masks"][j, k][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
            assert np.array_equal(bits.astype(bool), whole), (o, lag)
            seen += int(up.sum())
    assert seen > 100


# ---- 2. the walk case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("factor,cont", [(1.0, True), (C.HYSTERESIS, True), (C.HYSTERESIS, False)])
def test_walk_case(engine, split, factor, cont):
    """items of 64, 3 and 3 centres; 0, 1, 2, 64 and 65 neighbours; a centre truncated at the origins 0 and 3 alone; a coincident
    pair.  truncated[j] follows the origins of lag j"""
    pos, box, groups, r_cut = C.walk_split() if split else Q.walk_case()
    lags, r_break = [0, 1, 2, 4], C.breaks(r_cut, factor)
    ref = C.reference(pos, box, groups, r_cut, r_break, lags, 1, 1, cont)
    assert ref["truncated"][:, 0].tolist() == [2, 2, 1, 1] and not ref["truncated"][:, 1].any() and not ref["truncated_allowed"].any()
    _resident(engine, pos)
    listing = _listing(groups)
    n = np.stack([engine.debug_neighbour_lists(box, r_cut, f, listing)[0] for f in range(5)])
    if not split:
        assert Q.walk_counts(n)
    got = _call(engine, box, r_cut, lags, listing, 1, r_break, 1, cont)
    assert C.check(got, ref, f"walk case split {split} r_break x {factor} continuous {cont}")
    assert got["truncated"][:, 0].tolist() == [2, 2, 1, 1]
    _exact(engine, got, box, r_cut, listing, [len(g) for g in groups], 5, lags, 1, cont, "walk case")
    assert not got["alive_masks"][:, [0, 3], 0].any() and got["alive_masks"][0, 1, 0] == np.uint64(2 ** 64 - 1)   # truncated: 0; 64 neighbours: all bits
    if split:                                                              # the truncated centre's bonds are missing on one side alone
        assert got["bonds"][0, 0, 1] + 2 * 65 == got["bonds"][0, 1, 0]


# ---- 3. closed forms, independent of the reference ---------------------------------------------------------------------------
def test_frozen_trajectory(engine):
    pos = P.frozen(90, 7, 4)
    groups = _listing(Q.two_species(90)[::-1])
    _resident(engine, pos)
    for cont in (True, False):
        got = _call(engine, Q.CUBIC, 7.0, [0, 1, 3, 6], groups, 2, 1.1 * 7.0, 1, cont)
        assert got["bonds"][0].sum() > 200 and np.array_equal(got["alive"], got["bonds"])
        assert np.array_equal(got["unbroken"], got["bonds"] if cont else np.zeros_like(got["bonds"]))
        assert not got["lost"][:, :, 1:].any() and not got["truncated"].any()
        n_o = np.array([4, 3, 2, 1], np.uint64)                            # origins 0, 2, 4, 6 with o + lag <= 6
        assert np.array_equal(got["bonds"], got["bonds"][3][None] * n_o[:, None, None])
        assert np.array_equal(got["lost"][:, :, 0], n_o[:, None] * np.array([len(g) for g in groups], np.uint64)[None, :])


def test_dimer_that_leaves_and_returns(engine):
    """apart at the frames 3 and 4, back at frame 5: at lag 5 the bond is alive and was broken"""
    pos = C.dimer([1.0, 1.0, 1.0, 3.0, 3.0, 1.0])
    _resident(engine, pos)
    got = _call(engine, Q.CUBIC, 2.0, [0, 2, 3, 5], None)
    assert got["bonds"][:, 0, 0].tolist() == [2 * 4, 2 * 3, 2 * 3, 2]     # listed at the origins 0, 1, 2, 5
    assert got["alive"][:, 0, 0].tolist() == [8, 2, 2, 2] and got["unbroken"][:, 0, 0].tolist() == [8, 2, 0, 0]
    assert got["alive"][3, 0, 0] == got["bonds"][3, 0, 0] and got["unbroken"][3, 0, 0] == 0          # intermittent 1, continuous 0
    assert got["lost"][3, 0].tolist()[:2] == [2, 0] and got["lost"][2, 0].tolist()[:2] == [2, 4]
    assert got["alive_masks"][3, 0].tolist() == [1, 1] and got["unbroken_masks"][3, 0].tolist() == [0, 0]
    coarse = _call(engine, Q.CUBIC, 2.0, [0, 5], None, ss=5)               # sampled every fifth frame, the excursion is not seen
    assert coarse["unbroken"][:, 0, 0].tolist() == [8, 2]


def test_dimer_between_r_cut_and_r_break(engine):
    """1.9 and 2.2 apart in turn, r_cut 2: alive all along with r_break 2.4, broken at every odd lag without"""
    pos = C.dimer([1.9, 2.2] * 4)
    _resident(engine, pos)
    lags = [0, 1, 2, 3]
    held = _call(engine, Q.CUBIC, 2.0, lags, None, 1, 2.4)
    n_o = [2 * 4, 2 * 4, 2 * 3, 2 * 3]                                     # the even origins list the bond: 0, 2, 4, 6 with o + lag <= 7
    assert held["bonds"][:, 0, 0].tolist() == n_o and np.array_equal(held["alive"], held["bonds"]) and np.array_equal(held["unbroken"], held["bonds"])
    bare = _call(engine, Q.CUBIC, 2.0, lags, None, 1)
    assert bare["bonds"][:, 0, 0].tolist() == n_o and bare["alive"][:, 0, 0].tolist() == [8, 0, 6, 0]
    assert bare["unbroken"][:, 0, 0].tolist() == [8, 0, 0, 0]
    assert bare["lost"][1, 0].tolist()[:2] == [6, 8] and held["lost"][1, 0].tolist()[:2] == [14, 0]   # (an origin that lists nothing: centres that lost 0)


def test_diamond(engine):
    pos, groups = Q.diamond(4)
    _resident(engine, pos)
    lags = [0, 1, 3]
    got = _call(engine, Q.CUBIC, 2.8, lags, _listing(groups), 1, 3.0)
    n_o = np.array([4, 3, 1], np.uint64)
    assert np.array_equal(got["bonds"], n_o[:, None, None] * np.array([[0, 4 * 256], [4 * 256, 0]], np.uint64)[None])
    assert np.array_equal(got["alive"], got["bonds"]) and np.array_equal(got["unbroken"], got["bonds"])
    assert np.array_equal(got["lost"][:, :, 0], np.broadcast_to(256 * n_o[:, None], (3, 2))) and not got["lost"][:, :, 1:].any()
    assert np.all(got["alive_masks"][0] == 15) and not got["alive_masks"][2, 1:].any() and np.all(got["unbroken_masks"][2, 0] == 15)


# ---- 4. the same bits ------------------------------------------------------------------------------------------------------
def _equal(x, y, keys=None):
    return all((x[k] is None and y[k] is None) or np.array_equal(x[k], y[k]) for k in (keys or x))


def test_budgets_blocks_and_repeats(engine):
    from psa_amd import _hip
    pos, box, groups, r_cut, r_break, lags, step, ss, cont, ref = _case("cubic37", "two", (True, C.HYSTERESIS, 3, 1, True))
    n = pos.shape[1]
    listing = _listing(groups)
    _resident(engine, pos)
    whole = _call(engine, box, r_cut, lags, listing, step, r_break, ss, cont)
    assert C.check(whole, ref, "cubic37 whole") and _equal(whole, _call(engine, box, r_cut, lags, listing, step, r_break, ss, cont))
    bare = _call(engine, box, r_cut, lags, listing, step, r_break, ss, cont, per_atom=False)
    assert bare["alive_masks"] is None and bare["unbroken_masks"] is None and _equal(whole, bare, C.KEYS)
    for origins in (1, 3, 14):                                             # origins per block: 14, 5 and 1 block
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n * origins + 5)
        assert _equal(whole, _call(engine, box, r_cut, lags, listing, step, r_break, ss, cont)), origins
        assert _equal(whole, _call(engine, box, r_cut, lags, listing, step, r_break, ss, False), ("bonds", "alive", "lost", "truncated", "alive_masks"))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n - 1)
    with pytest.raises(_hip.PsaHipError, match=f"need {PER_ORIGIN * n} bytes"):
        _call(engine, box, r_cut, lags, listing, step, r_break, ss, cont)


def _bonds_of(masks, lists, atoms):
    """the set of (lag, origin, centre atom, neighbour atom) of the bits set"""
    out = set()
    for j, k, a in zip(*np.nonzero(masks)):
        for i in range(64):
            if int(masks[j, k, a]) >> i & 1:
                out.add((int(j), int(k), int(atoms[a]), int(atoms[lists[k][a, i]])))
    return out


def test_permutation_of_the_atoms(engine):
    """integer adds over the same pairs: the same counts for any order of the atoms inside a species, the masks the same sets of
    bonds once their bits are mapped to atoms through the lists of either order"""
    pos, box, groups, r_cut, r_break, lags, step, ss, cont, _ = _case("triclinic130", "two", (True, C.HYSTERESIS, 3, 1, True))
    listing = _listing(groups)
    _resident(engine, pos)
    whole = _call(engine, box, r_cut, lags, listing, step, r_break, ss, cont)
    rng = np.random.default_rng(8)
    shuffled = [g[rng.permutation(len(g))] for g in listing]
    moved = _call(engine, box, r_cut, lags, shuffled, step, r_break, ss, cont)
    assert _equal(whole, moved, C.KEYS) and not np.array_equal(whole["alive_masks"], moved["alive_masks"])
    origins = range(0, pos.shape[0], step)
    for key in ("alive_masks", "unbroken_masks"):
        sets = [_bonds_of(res[key], [engine.debug_neighbour_lists(box, r_cut, o, order)[1] for o in origins], np.concatenate(order))
                for res, order in ((whole, listing), (moved, shuffled))]
        assert sets[0] == sets[1] and len(sets[0]) == int(whole[key[:-6]].sum())


# ---- 5. scratch, no trace ------------------------------------------------------------------------------------------------
def _calculator(engine, pos, box, types=None, dt=0.002, vel=None):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos) if vel is None else vel, np.ones(n, np.int32) if types is None else types,
                    np.arange(n_t, dtype=np.float32), box, np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, 1, 1, 1).attach(engine=engine)


def test_poisoned_scratch_and_no_trace(engine):
    pos, box, rc = Q.family("cubic37")
    vel = np.random.default_rng(3).standard_normal(pos.shape).astype(np.float32)
    calc = _calculator(engine, pos, box, vel=vel)
    mags, vecs = calc.get_k_path("100", 1.0, 8)

    def others():
        ang = calc.calculate_bond_angles(rc, 45)
        clu = calc.calculate_solid_clusters(rc, 6, 0.35, 3, per_atom=True)
        sed = calc.calculate(mags, vecs)
        return [np.asarray(ang.counts), np.asarray(ang.coordination_counts), np.asarray(clu.size_counts), np.asarray(clu.labels),
                np.asarray(clu.largest), np.asarray(sed.intensity if sed.is_complex else sed.sed)]

    def call(eng, loud=False):
        got = _call(eng, box, Q.matrix_cutoff(rc, 2), [0, 1, 2, 7, 39], _listing(Q.two_species(37)), 3, C.breaks(Q.matrix_cutoff(rc, 2), 1.2))
        return [np.asarray(v).copy() for v in got.values()]
    before = others()
    engine.timings()                                                       # (reset)
    r0 = call(engine)
    t = engine.timings()
    assert all(t[k] > 0 for k in ("gather", "transpose", "phase", "d2h"))
    try:
        S.check_poisoned(engine, "bond_persistence per atom", call, r0)
    finally:
        engine.scratch_fill(-1)
    for a, b in zip(before, others()):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 6. the calculator -----------------------------------------------------------------------------------------------------
def test_calculator(engine):
    from psa_amd import BondPersistence
    pos, box, groups, r_cut, r_break, lags, step, ss, cont, _ = _case("triclinic130", "two", (True, C.HYSTERESIS, 3, 1, True))
    types = np.ones(130, np.int32)
    types[groups[1]] = 2
    calc = _calculator(engine, pos, box, types)
    res = calc.calculate_bond_persistence(r_cut, lags, basis_atom_types=[1, 2], r_break=r_break, origin_step=3, per_atom=True)
    raw = _call(engine, box, r_cut, lags, _listing(groups), 3, r_break)
    assert isinstance(res, BondPersistence) and all(np.array_equal(getattr(res, k), raw[k]) for k in C.KEYS + ("alive_masks", "unbroken_masks"))
    assert np.array_equal(res.lags, lags) and np.allclose(res.times, 0.002 * np.asarray(lags)) and res.atoms.shape == (130,)
    assert np.array_equal(res.origins, [(12 - 1 - t) // 3 + 1 for t in lags])
    assert np.all(res.intermittent[0][raw["bonds"][0] > 0] == 1.0) and np.isnan(res.intermittent[:, 1, 1]).all()   # r_cut[1][1] = 0
    assert np.all(res.continuous[raw["bonds"] > 0] <= res.intermittent[raw["bonds"] > 0]) and np.all(res.cage(1)[0] == 1.0)
    assert np.array_equal(res.pair(0, 1)["alive"], raw["alive"][:, 0, 1]) and res.lifetime().shape == (2, 2)
    plain = calc.calculate_bond_persistence(r_cut, [0, 2], basis_atom_types=[1, 2], continuous=False)
    assert plain.unbroken is None and plain.continuous is None and plain.alive_masks is None
    same = _call(engine, box, r_cut, [0, 2], _listing(groups), 1, None, 1, False, False)
    assert np.array_equal(plain.alive, same["alive"]) and np.array_equal(plain.lost, same["lost"])
    with pytest.raises(ValueError, match="continuous correlation was not computed"):
        plain.lifetime()
    ball = Q.ball(70, 3, 6.0)
    with pytest.raises(ValueError, match="more than 64 neighbours"):
        _calculator(engine, ball, Q.CUBIC).calculate_bond_persistence(6.0, [0, 1])


def test_sharded_calculator_refuses(engine):
    pos, box, rc = Q.family("cubic37")
    calc = _calculator(engine, pos, box)

    class Sharded:
        nranks = 2
    calc._shard = Sharded()
    with pytest.raises(NotImplementedError, match="sharded calculator"):
        calc.calculate_bond_persistence(rc, [0, 1])


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    import ctypes as ct

    from psa_amd import _hip, max_pair_radius
    pos, box, rc = Q.family("cubic37")                                     # 40 frames
    _resident(engine, pos)
    two = _listing(Q.two_species(37))

    def refused(word, r_cut=rc, lags=(0, 1), groups=None, step=1, **kw):
        with pytest.raises(_hip.PsaHipError, match=word):
            engine.bond_persistence(box, r_cut, list(lags), groups, step, **kw)
    refused("r_break.* must be finite and at least r_cut", r_break=0.9 * rc)
    refused("r_break.* must be finite", r_break=float("inf"))
    refused("r_break.* must be finite", r_break=float("nan"))
    refused("r_break is not symmetric", groups=two, r_break=[[9.0, 9.0], [9.5, 9.0]])
    refused("r_break.*beyond the served radius", r_break=1.01 * max_pair_radius(box))
    refused("one is 0", r_cut=Q.matrix_cutoff(rc, 2), groups=two, r_break=np.full((2, 2), 9.0))
    refused("must be finite and at least r_cut", r_cut=rc, groups=two, r_break=[[9.0, 9.0], [9.0, 0.0]])
    refused("lags must be strictly ascending", lags=(0, 2, 2))
    refused("lags must be strictly ascending", lags=(3, 1))
    refused(r"lag 40 is outside \[0, T - 1 = 39\]", lags=(0, 40))
    refused("lag -1 is outside", lags=(-1, 0))
    refused("lag 3 is no multiple of sample_step = 2", lags=(0, 2, 3), sample_step=2)
    refused(r"number of lags is in \[1, 1024\], got 0", lags=())
    refused("sample_step must be at least 1, got 0", sample_step=0)
    refused("origin_step must be at least 1, got 0", step=0)
    refused("r_cut.*beyond the served radius", r_cut=1.01 * max_pair_radius(box), r_break=1.02 * max_pair_radius(box))
    refused("r_cut is not symmetric", r_cut=[[3.0, 2.0], [2.5, 3.0]], groups=two, r_break=np.full((2, 2), 4.0))
    refused("listed twice", groups=[np.array([0, 1], np.int32), np.array([1, 2], np.int32)])
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * 37 - 1)
    refused(f"need {PER_ORIGIN * 37} bytes")
    reset(engine)
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        refused("sharded context.*psa_bond_persistence|psa_bond_persistence.*sharded context")
    finally:
        engine.comm_destroy()
    # what the Engine method cannot get wrong: 1025 lags, continuous = 2, byte counts that are not exact
    a = engine._shell_args(box, None, None, rc, 1)
    lag = np.arange(1025, dtype=np.int64)
    u64 = lambda x: x.ctypes.data_as(ct.POINTER(ct.c_uint64))             # noqa: E731
    pair, lost, trunc, masks = np.zeros((2, 1, 1), np.uint64), np.zeros((2, 1, 65), np.uint64), np.zeros((2, 1), np.uint64), np.zeros((2, 40, 37), np.uint64)

    def raw(word, n_lags=2, continuous=1, pair_bytes=16, lost_bytes=2 * 65 * 8, trunc_bytes=16, with_masks=False, masks_bytes=0):
        rc_ = engine._lib.psa_bond_persistence(*a.head, a.alive[4].ctypes.data_as(ct.POINTER(ct.c_double)), 1,
                                               lag.ctypes.data_as(ct.POINTER(ct.c_int64)), n_lags, 1, continuous, u64(pair), u64(pair.copy()),
                                               u64(pair.copy()), pair_bytes, u64(lost), lost_bytes, u64(trunc), trunc_bytes,
                                               u64(masks) if with_masks else None, None, masks_bytes)
        assert rc_ != 0 and word in engine._lib.psa_last_error().decode(), engine._lib.psa_last_error()
    raw("number of lags is in [1, 1024], got 1025", n_lags=1025)
    raw("continuous is 0 or 1, got 2", continuous=2)
    raw("pair_bytes is 15", pair_bytes=15)
    raw("lost_bytes is 1048", lost_bytes=1048)
    raw("truncated_bytes is 8", trunc_bytes=8)
    raw("masks_bytes is 8", with_masks=True, masks_bytes=8)
    empty = engine.bond_persistence(box, rc, [0, 1], [np.zeros(0, np.int32)], per_atom=True)
    assert not any(empty[k].any() for k in C.KEYS) and empty["alive_masks"].shape == (2, 40, 0)
    assert engine.bond_persistence(box, rc, [0, 1])["bonds"].all()
