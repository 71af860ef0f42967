"""The common-neighbour analysis on the GPU (psa_common_neighbours, Engine.common_neighbours and the calculator method).  Every
comparison is of integers and exact: against the float64 reference of tests/cna64.py by cna_cases.check on the families of
angle_cases (one, two and three species, the matrix of cut-offs with its zero entry, origin steps 1, 3 and above T); against
the pure-integer route over the engine's own neighbour lists on every family and on angle_cases.walk_case and its
split-species variant; closed forms that need no reference (fcc, bcc, hcp, the icosahedron, diamond); the exact identities of
the definition on every case; the same bits for any budget, for repeated calls, with and without the per-atom outputs and for
a permutation of the atoms; poisoned scratch; no trace in later calls; the calculator; every refusal."""
import functools

import numpy as np
import pytest

import angle_cases as Q
import cna_cases as C
import scratch_cases as S
from engine_state import reset

pytestmark = pytest.mark.gpu

PER_ORIGIN = 1040 + 8                                                      # work bytes per atom and origin; with the per-bond output:
PER_ORIGIN_BONDS = PER_ORIGIN + 256
CONFIGS = [(False, 1), (True, 1), (False, 3), (True, None)]               # (the matrix of cut-offs?, origin_step -- None: above T)


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


@functools.lru_cache(maxsize=None)
def _case(name, kind, matrix):
    """the inputs of a family and their reference over every frame, computed once"""
    pos, box, rc = Q.family(name)
    groups = C.species(kind, pos.shape[1])
    r_cut = C.cutoffs(kind, rc, matrix)
    return pos, box, groups, r_cut, C.Reference(pos, box, groups, r_cut)


def _exact(engine, got, box, r_cut, listing, step, what):
    """the exact identities: the bonds against sum_n n coord of psa_angle_histogram, the census against N_alpha, the dtypes"""
    assert all(got[k].dtype == np.uint64 for k in C.COUNTS), what
    _, coord, trunc = engine.angle_histogram(box, r_cut, 1, listing, step)
    bonds = (coord * np.arange(65, dtype=np.uint64)).sum(axis=(1, 2), dtype=np.uint64)
    S_ = len(listing)
    assert np.array_equal(got["signature_counts"].reshape(S_, -1).sum(axis=1, dtype=np.uint64) + got["signature_outside"], bonds), what
    assert np.array_equal(got["truncated"], trunc), what
    sizes = np.array([len(g) for g in listing], np.uint64)
    start = np.concatenate([[0], np.cumsum([len(g) for g in listing])])
    if got["types"] is not None:
        assert got["types"].dtype == np.int32 and got["n"].dtype == np.int32 and got["bond_signatures"].dtype == np.uint32
        cut = np.stack([(got["types"][:, start[a]:start[a + 1]] < 0).sum(axis=1) for a in range(S_)], axis=1).astype(np.uint64)
        assert np.array_equal(cut, np.stack([(got["n"][:, start[a]:start[a + 1]] > 64).sum(axis=1) for a in range(S_)], axis=1)), what
        assert np.array_equal(got["type_counts"].sum(axis=2, dtype=np.uint64) + cut, np.broadcast_to(sizes[None, :], cut.shape)), what
        assert np.array_equal(cut.sum(axis=0, dtype=np.uint64), got["truncated"]), what
    else:
        assert np.array_equal(got["type_counts"].sum(axis=(0, 2), dtype=np.uint64) + got["truncated"], sizes * np.uint64(got["type_counts"].shape[0])), what


def _equal(x, y, keys=None):
    return all((x[k] is None and y[k] is None) or np.array_equal(x[k], y[k]) for k in (keys or x))


def _from_lists(engine, box, r_cut, listing, frames):
    """the expected dict of a call over the origins `frames`, by the integer route over psa_debug_neighbour_lists"""
    rows = []
    for f in frames:
        count, lists = engine.debug_neighbour_lists(box, r_cut, f, listing)
        rows.append((count,) + C.from_lists(count, lists))
    return C.with_groups(C.result_of(rows, listing), listing)


# ---- 1. against the reference, 2. against the engine's own lists, 4. the identities -------------------------------------------
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("kind", ["one", "two", "three"])
@pytest.mark.parametrize("name", list(Q.FAMILIES))
def test_against_the_reference(engine, name, kind, config):
    matrix, step = config
    pos, box, groups, r_cut, ref = _case(name, kind, matrix)
    step = pos.shape[0] + 1 if step is None else step
    want, out = ref.result(step), ref.excluded(step)
    whole = _case(name, "one", False)[4]                                   # what the family holds: before the GPU is touched
    assert ref.excluded().mean() <= C.EXCLUDED_CAP and whole.bonds > 100 and C.distinct_signatures(whole.result()) >= 50
    assert whole.branching > 0 and whole.result()["signature_outside"].sum() > 0 and ref.bonds > 100
    _resident(engine, pos)
    listing = _listing(groups)
    what = f"{name} {kind} {config}"
    got = engine.common_neighbours(box, r_cut, listing, step, per_atom=True)
    assert C.check(got, want, out, what)
    _exact(engine, got, box, r_cut, listing, step, what)
    assert C.check(got, _from_lists(engine, box, r_cut, listing, range(0, pos.shape[0], step)), None, what + " (lists)")
    bare = engine.common_neighbours(box, r_cut, listing, step)
    assert bare["types"] is None and bare["n"] is None and bare["bond_signatures"] is None and _equal(got, bare, C.COUNTS)
    _exact(engine, bare, box, r_cut, listing, step, what)


@pytest.mark.parametrize("split", [False, True])
def test_walk_case(engine, split):
    """items of 64, 3 and 3 centres; 0, 1, 2, an odd number, 64 and 65 neighbours; a centre truncated at the origins 0 and 3 alone,
    which stays a neighbour of 65 centres; a coincident pair"""
    pos, box, groups, r_cut = C.walk_split() if split else Q.walk_case()
    _resident(engine, pos)
    listing = _listing(groups)
    got = engine.common_neighbours(box, r_cut, listing, 1, per_atom=True)
    if not split:
        assert Q.walk_counts(got["n"])
    assert got["types"][[0, 3], 0].tolist() == [-1, -1] and (got["types"] == -1).sum() == 2 and got["n"][[1, 2, 4], 0].tolist() == [64, 64, 64]
    assert np.all(got["bond_signatures"][[0, 3], 0] == C.NO_BOND) and np.all(got["bond_signatures"][[1, 2, 4], 0] != C.NO_BOND)
    assert got["truncated"].tolist() == [2, 0]
    assert C.check(got, _from_lists(engine, box, r_cut, listing, range(5)), None, f"walk case split {split}")
    _exact(engine, got, box, r_cut, listing, 1, "walk case")
    # the coincident pair (67, 68) is bonded; with the third atom in reach (frames 0, 3, 4 -- frame 3: apart) each bond has it in common
    col = {False: (67, 68, 69), True: (2, 3, 4)}[split]
    assert got["bond_signatures"][1, col[0], 0] == 0 and got["bond_signatures"][0, col[0], 0] == 1 | 0 << 8


# ---- 3. closed forms, independent of any reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc", "bcc", "hcp", "ico", "diamond"])
def test_closed_forms(engine, name):
    pos, box, groups, r_cut = C.closed_inputs(name)
    _resident(engine, pos)
    listing = _listing(groups)
    got = engine.common_neighbours(box, r_cut, listing, 1, per_atom=True)
    assert C.closed_form_holds(name, got), name
    _exact(engine, got, box, r_cut, listing, 1, name)


# ---- 5. the same bits ------------------------------------------------------------------------------------------------------------
def test_budgets_blocks_and_repeats(engine):
    from psa_amd import _hip
    pos, box, groups, r_cut, ref = _case("cubic37", "two", True)
    n, step = pos.shape[1], 3
    listing = _listing(groups)
    _resident(engine, pos)
    whole = engine.common_neighbours(box, r_cut, listing, step, per_atom=True)
    assert C.check(whole, ref.result(step), ref.excluded(step), "cubic37 whole")
    assert _equal(whole, engine.common_neighbours(box, r_cut, listing, step, per_atom=True))
    for origins in (1, 3, 14):                                             # origins per block: 14, 5 and 1 block
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN_BONDS * n * origins + 5)
        assert _equal(whole, engine.common_neighbours(box, r_cut, listing, step, per_atom=True)), origins
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n * origins + 5)
        assert _equal(whole, engine.common_neighbours(box, r_cut, listing, step), C.COUNTS), origins
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN_BONDS * n - 1)
    with pytest.raises(_hip.PsaHipError, match=f"need {PER_ORIGIN_BONDS * n} bytes"):
        engine.common_neighbours(box, r_cut, listing, step, per_atom=True)
    assert _equal(whole, engine.common_neighbours(box, r_cut, listing, step), C.COUNTS)   # without the per-bond output it fits
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n - 1)
    with pytest.raises(_hip.PsaHipError, match=f"need {PER_ORIGIN * n} bytes"):
        engine.common_neighbours(box, r_cut, listing, step)


def _bonds_of(res, lists, atoms):
    """the multiset, as a sorted list, of (origin, centre atom, neighbour atom, word) of the bonds of a result"""
    out = []
    for k, a, i in zip(*np.nonzero(res["bond_signatures"] != C.NO_BOND)):
        out.append((int(k), int(atoms[a]), int(atoms[lists[k][a, i]]), int(res["bond_signatures"][k, a, i])))
    return sorted(out)


def test_permutation_of_the_atoms(engine):
    """integer adds over the same bonds: the same counts for any order of the atoms inside a species, the same signature on every
    bond once the words are mapped to atoms through the lists of either order"""
    pos, box, groups, r_cut, _ = _case("triclinic130", "two", True)
    listing, step = _listing(groups), 3
    _resident(engine, pos)
    whole = engine.common_neighbours(box, r_cut, listing, step, per_atom=True)
    rng = np.random.default_rng(8)
    shuffled = [g[rng.permutation(len(g))] for g in listing]
    moved = engine.common_neighbours(box, r_cut, shuffled, step, per_atom=True)
    assert _equal(whole, moved, C.COUNTS) and not np.array_equal(whole["bond_signatures"], moved["bond_signatures"])
    origins = range(0, pos.shape[0], step)
    sets = [_bonds_of(res, [engine.debug_neighbour_lists(box, r_cut, o, order)[1] for o in origins], np.concatenate(order))
            for res, order in ((whole, listing), (moved, shuffled))]
    assert sets[0] == sets[1] and len(sets[0]) == int(whole["signature_counts"].sum() + whole["signature_outside"].sum())
    back = [np.argsort(np.concatenate(order), kind="stable") for order in (listing, shuffled)]
    assert np.array_equal(whole["types"][:, back[0]], moved["types"][:, back[1]]) and np.array_equal(whole["n"][:, back[0]], moved["n"][:, back[1]])


# ---- 6. scratch, no trace, the calculator, refusals --------------------------------------------------------------------------
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
        got = eng.common_neighbours(box, Q.matrix_cutoff(rc, 2), _listing(Q.two_species(37)), 3, per_atom=True)
        return [np.asarray(v).copy() for v in got.values()]
    before = others()
    engine.timings()                                                       # (reset)
    r0 = call(engine)
    t = engine.timings()
    assert all(t[k] > 0 for k in ("gather", "transpose", "phase", "project", "epilogue", "d2h")) and t["project"] <= t["phase"]
    try:
        S.check_poisoned(engine, "common_neighbours per atom", call, r0)
    finally:
        engine.scratch_fill(-1)
    for a, b in zip(before, others()):
        assert np.array_equal(a, b, equal_nan=True)


def test_calculator(engine):
    from psa_amd import CommonNeighbours
    pos, box, groups, r_cut, ref = _case("triclinic130", "two", True)
    types = np.ones(130, np.int32)
    types[groups[1]] = 2
    calc = _calculator(engine, pos, box, types)
    res = calc.calculate_common_neighbours(r_cut, basis_atom_types=[1, 2], origin_step=3, per_atom=True)
    raw = engine.common_neighbours(box, r_cut, _listing(groups), 3, per_atom=True)
    assert isinstance(res, CommonNeighbours) and all(np.array_equal(getattr(res, k), raw[k]) for k in C.COUNTS + ("types", "bond_signatures"))
    assert np.array_equal(res.neighbours, raw["n"]) and res.atoms.shape == (130,) and res.origins == 4 and res.sizes.tolist() == [90, 40]
    assert res.structure_names == ("other", "fcc", "hcp", "bcc", "ico") and np.allclose(sum(res.fraction(t) for t in res.structure_names), 1.0)
    assert np.array_equal(res.signature(2, 1, 1), raw["signature_counts"][:, 2, 1, 1]) and 0.0 < res.share(2, 1, 1) < 1.0
    assert np.array_equal(res.atoms_of(1, "other"), res.atoms[raw["types"][1] == 0])
    plain = calc.calculate_common_neighbours(r_cut, basis_atom_types=[1, 2])
    assert plain.types is None and plain.bond_signatures is None and plain.type_counts.shape == (12, 2, 5)
    assert np.array_equal(plain.type_counts[::3], res.type_counts)
    fcc = _calculator(engine, *C.closed_inputs("fcc")[:2]).calculate_common_neighbours(4.64, per_atom=True)
    assert np.all(fcc.fraction("fcc") == 1.0) and fcc.share(4, 2, 1) == 1.0 and fcc.atoms_of(0, "fcc").size == 256
    with pytest.raises(ValueError, match="more than 64 neighbours"):
        _calculator(engine, Q.ball(70, 3, 6.0), Q.CUBIC).calculate_common_neighbours(6.0)
    with pytest.raises(TypeError, match="per_atom must be a bool"):
        calc.calculate_common_neighbours(r_cut, per_atom=1)


def test_sharded_calculator_refuses(engine):
    pos, box, rc = Q.family("cubic37")
    calc = _calculator(engine, pos, box)

    class Sharded:
        nranks = 2
    calc._shard = Sharded()
    with pytest.raises(NotImplementedError, match="sharded calculator"):
        calc.calculate_common_neighbours(rc)


def test_refusals_and_empty_species(engine):
    import ctypes as ct

    from psa_amd import _hip, max_pair_radius
    pos, box, rc = Q.family("cubic37")                                     # 40 frames
    _resident(engine, pos)
    two = _listing(Q.two_species(37))

    def refused(word, r_cut=rc, groups=None, step=1, **kw):
        with pytest.raises(_hip.PsaHipError, match=word):
            engine.common_neighbours(box, r_cut, groups, step, **kw)
    refused("origin_step must be at least 1, got 0", step=0)
    refused("r_cut.*beyond the served radius", r_cut=1.01 * max_pair_radius(box))
    refused("r_cut is not symmetric", r_cut=[[3.0, 2.0], [2.5, 3.0]], groups=two)
    refused("must be finite and not negative", r_cut=-1.0)
    refused("must be finite and not negative", r_cut=float("nan"))
    refused("listed twice", groups=[np.array([0, 1], np.int32), np.array([1, 2], np.int32)])
    with pytest.raises(ValueError, match="out of bounds"):                # (the reference's exception type for this one)
        engine.common_neighbours(box, rc, [np.array([0, 37], np.int32)])
    refused(r"number of atom groups is in \[1, 8\], got 9", groups=[np.array([i], np.int32) for i in range(9)])
    with pytest.raises(_hip.PsaHipError, match="not the inverse of box"):
        engine.common_neighbours(box, rc, box_inverse=2.0 * np.linalg.inv(np.asarray(box, np.float64)))
    with pytest.raises(_hip.PsaHipError, match="must be finite"):
        engine.common_neighbours(box, rc, box_inverse=np.full((3, 3), np.nan))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * 37 - 1)
    refused(f"need {PER_ORIGIN * 37} bytes")
    reset(engine)
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        refused("sharded context.*psa_common_neighbours|psa_common_neighbours.*sharded context")
    finally:
        engine.comm_destroy()
    # what the Engine method cannot get wrong: byte counts that are not exact, null outputs
    a = engine._shell_args(box, None, None, rc, 1)
    u64 = lambda x: x.ctypes.data_as(ct.POINTER(ct.c_uint64))             # noqa: E731
    i32 = lambda x: x.ctypes.data_as(ct.POINTER(ct.c_int32))              # noqa: E731
    table, one, census = np.zeros((1, 8, 16, 16), np.uint64), np.zeros(1, np.uint64), np.zeros((40, 1, 5), np.uint64)
    atoms, bonds = np.zeros((40, 37), np.int32), np.zeros((40, 37, 64), np.uint32)

    def raw(word, table_bytes=table.nbytes, census_bytes=census.nbytes, types=False, n=False, atom_bytes=0, sigs=False, bond_bytes=0,
            no_table=False):
        rc_ = engine._lib.psa_common_neighbours(*a.head, 1, None if no_table else u64(table), table_bytes, u64(one), u64(census), census_bytes,
                                                u64(one.copy()), i32(atoms) if types else None, i32(atoms.copy()) if n else None, atom_bytes,
                                                bonds.ctypes.data_as(ct.POINTER(ct.c_uint32)) if sigs else None, bond_bytes)
        assert rc_ != 0 and word in engine._lib.psa_last_error().decode(), engine._lib.psa_last_error()
    raw("signature_bytes is 16383", table_bytes=table.nbytes - 1)
    raw("type_bytes is 1608", census_bytes=census.nbytes + 8)
    raw("atom_bytes is 0", types=True)
    raw("atom_bytes is 5924", n=True, atom_bytes=atoms.nbytes + 4)
    raw("bond_bytes is 378879", sigs=True, bond_bytes=bonds.nbytes - 1)
    raw("null output", no_table=True)
    ok = engine._lib.psa_common_neighbours(*a.head, 1, u64(table), table.nbytes, u64(one), u64(census), census.nbytes, u64(one.copy()), None,
                                           i32(atoms), atoms.nbytes, None, 12345)   # byte counts of outputs not asked for are not read
    assert ok == 0 and atoms.any()
    # empty species: all of them, and one among others
    empty = engine.common_neighbours(box, rc, [np.zeros(0, np.int32)], per_atom=True)
    assert not any(empty[k].any() for k in C.COUNTS) and empty["types"].shape == (40, 0) and empty["bond_signatures"].shape == (40, 0, 64)
    three = _listing(Q.three_species(37))
    got = engine.common_neighbours(box, rc, three, 5, per_atom=True)
    assert not got["signature_counts"][1].any() and not got["type_counts"][:, 1].any() and got["signature_counts"][[0, 2]].any()
    assert engine.common_neighbours(box, rc)["signature_counts"].any()
