"""The adaptive common-neighbour analysis on the GPU (psa_adaptive_common_neighbours, Engine.adaptive_common_neighbours and the
calculator method): against the float64 reference of tests/acna64.py by acna_cases.check on the four inputs of acna_cases (one
and two species, for the gas the matrix of cut-offs with its zero entry, origin steps 1, 3 and above T, with and without the
per-atom outputs); closed forms that need no reference (fcc, bcc, hcp, the icosahedron, diamond); the point of the feature (a
scaled crystal, an exact factor of two); angle_cases.walk_case and its split-species variant; the exact identities of the
definition on every case; the same bits for any budget, for repeated calls and for a permutation of the atoms; poisoned scratch;
no trace in later calls; the calculator; every refusal."""
import functools

import numpy as np
import pytest

import acna_cases as C
import angle64 as A
import angle_cases as Q
import order_cases
import pair_cases as P
import scratch_cases as S
from engine_state import reset

pytestmark = pytest.mark.gpu

PER_ORIGIN = 1040 + 12                                                     # work bytes per atom and origin; with the per-bond output:
PER_ORIGIN_BONDS = PER_ORIGIN + 112
# (case, species, the matrix of cut-offs?)
CONFIGS = [(name, kind, False) for name in C.CASES for kind in ("one", "two")] + [("gas", "two", True)]


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
def _case(name, kind="one", matrix=False):
    """the inputs of a case and their reference over every frame, computed once"""
    pos, box, rc = C.case(name)
    groups = C.species(kind, pos.shape[1])
    r_cut = C.cutoffs(kind, rc, matrix)
    return pos, box, groups, r_cut, C.Reference(pos, box, groups, r_cut)


def _equal(x, y, keys=None):
    return all((x[k] is None and y[k] is None) or np.array_equal(x[k], y[k], equal_nan=True) for k in (keys or x))


def _exact(engine, got, pos, box, r_cut, listing, step, what):
    """the exact identities of the definition, the dtypes, and `n` and `nearest` against the engine's own neighbour lists"""
    assert all(got[k].dtype == np.uint64 for k in C.COUNTS), what
    S_ = len(listing)
    sizes = np.array([len(g) for g in listing], np.uint64)
    start = np.concatenate([[0], np.cumsum([len(g) for g in listing])])
    n_o = got["type_counts"].shape[0]
    _, _, trunc = engine.angle_histogram(box, r_cut, 1, listing, step)
    assert np.array_equal(got["truncated"], trunc), what
    bonds = got["signature_counts"].reshape(S_, -1).sum(axis=1, dtype=np.uint64) + got["signature_outside"]
    if got["types"] is None:
        assert np.array_equal(got["type_counts"].sum(axis=(0, 2), dtype=np.uint64) + got["truncated"], sizes * np.uint64(n_o)), what
        return
    t, n, near, w, cut = got["types"], got["n"], got["nearest"], got["bond_signatures"], got["cutoffs"]
    assert t.dtype == np.int32 and n.dtype == np.int32 and near.dtype == np.int32 and w.dtype == np.uint32 and cut.dtype == np.float32
    per = lambda x: np.stack([x[:, start[a]:start[a + 1]].sum(axis=1) for a in range(S_)], axis=1).astype(np.uint64)   # noqa: E731
    assert np.array_equal(got["type_counts"].sum(axis=2, dtype=np.uint64) + per(t < 0), np.broadcast_to(sizes[None, :], (n_o, S_))), what
    assert np.array_equal(per(t < 0).sum(axis=0), got["truncated"]) and np.array_equal(t < 0, n > 64), what
    assert np.array_equal(per(n < 12).sum(axis=0), got["short"]), what
    members = (near >= 0).sum(axis=2)
    assert np.all(np.isin(members, (0, 12, 14))) and np.array_equal(members, (w != C.NO_BOND).sum(axis=2)), what
    assert np.array_equal(members > 0, (n >= 12) & (n <= 64)) and np.array_equal(np.isnan(cut), members == 0), what
    assert np.all((near >= 0) == (np.arange(14)[None, None, :] < members[:, :, None])), what   # by rank: no hole
    assert np.all(t[members == 14] % 3 == 0) and np.all(members[(t == 1) | (t == 2) | (t == 4)] == 12), what   # B: bcc or other
    assert np.array_equal(bonds, (12 * per(members == 12) + 14 * per(members == 14)).sum(axis=0)), what
    atoms = np.concatenate(listing).astype(np.int64)
    e64 = P.sigma_error(pos, box)
    for o, frame in enumerate(range(0, pos.shape[0], step)):
        count, lists = engine.debug_neighbour_lists(box, r_cut, frame, listing)
        assert np.array_equal(n[o], count), what
        e, d, r = A.frame_pairs(pos[frame], box, atoms)
        tol = P.tolerance(e.reshape(-1, 3), d.reshape(-1, 3), r.ravel(), box, 1.0, e64).reshape(r.shape)
        for a in np.flatnonzero(members[o]):
            m = near[o, a, :members[o, a]]
            assert len(set(m.tolist())) == m.size and set(m.tolist()) <= set(lists[a, :count[a]].tolist()), (what, o, a)
            assert np.all(np.diff(r[a, m]) >= -(tol[a, m][1:] + tol[a, m][:-1])), (what, o, a)   # non-descending distance


# ---- 1. against the reference, 5. the identities -----------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
def test_against_the_reference(engine, config):
    pos, box, groups, r_cut, ref = _case(*config)
    assert ref.excluded().mean() <= C.EXCLUDED_CAP                         # (before the GPU is touched)
    _resident(engine, pos)
    listing = _listing(groups)
    for step in (1, 3, pos.shape[0] + 1):
        what = f"{config} step {step}"
        got = engine.adaptive_common_neighbours(box, r_cut, listing, step, per_atom=True)
        assert C.check(got, ref.result(step), ref.excluded(step), ref.cut_tolerance(step), what)
        _exact(engine, got, pos, box, r_cut, listing, step, what)
        bare = engine.adaptive_common_neighbours(box, r_cut, listing, step)
        assert all(bare[k] is None for k in C.ROWS + ("cutoffs",)) and _equal(got, bare, C.COUNTS), what
        _exact(engine, bare, pos, box, r_cut, listing, step, what)


# ---- 2. closed forms, independent of any reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fcc", "bcc", "hcp", "ico", "diamond"])
def test_closed_forms(engine, name):
    """perfect fcc with 42 candidates, bcc with 26 (rho_11 = rho_12: test A's members are the tie rule's, it cannot come out fcc,
    hcp or ico, and test B decides), hcp, the icosahedron (the vertices short), diamond (all short)"""
    pos, box, groups, r_cut = C.closed_inputs(name)
    _resident(engine, pos)
    listing = _listing(groups)
    got = engine.adaptive_common_neighbours(box, r_cut, listing, 1, per_atom=True)
    assert C.closed_form_holds(name, got), name
    _exact(engine, got, pos, box, r_cut, listing, 1, name)
    if name == "fcc":                                                      # K a / sqrt 2, within 4 ulp
        want = np.float32(C.R.K * float(np.float32(21.72)) / 4.0 / np.sqrt(2.0))
        assert np.all(np.abs(got["cutoffs"] - want) <= 4 * np.spacing(want))
    if name == "diamond":
        assert np.all(got["types"] == 0) and np.all(got["n"] == 4) and got["short"].tolist() == [512, 512]


# ---- 3. the point of the feature ------------------------------------------------------------------------------------------------
def test_a_scaled_crystal_needs_no_new_radius(engine):
    """the fcc block with positions and box multiplied by 1.25: the plain analysis at the radius tuned for the unscaled crystal
    calls every atom other, the adaptive one with candidates up to the third shell calls every atom fcc"""
    pos = (order_cases.fcc_block().astype(np.float64) * 1.25).astype(np.float32)
    box = (np.asarray(Q.CUBIC, np.float64) * 1.25).astype(np.float32)
    _resident(engine, pos)
    plain = engine.common_neighbours(box, 4.64, None, 1, per_atom=True)
    assert np.all(plain["types"] == 0)
    got = engine.adaptive_common_neighbours(box, 8.0, None, 1, per_atom=True)
    assert np.all(got["types"] == 1) and np.all(got["n"] == 18) and int(got["signature_counts"][0, 4, 2, 1]) == 2 * 256 * 12


def test_an_exact_factor_of_two(engine):
    """positions, box and r_cut of the thermal fcc case multiplied by 2, exactly: every integer output the same bits, the
    cut-offs exactly doubled (the fractions are the same bits: the inverse of 2 H is half the inverse of H, exactly)"""
    pos, box, groups, r_cut, _ = _case("fcc")
    _resident(engine, pos)
    one = engine.adaptive_common_neighbours(box, r_cut, None, 1, per_atom=True)
    _resident(engine, pos * np.float32(2.0))
    two = engine.adaptive_common_neighbours(np.asarray(box, np.float32) * np.float32(2.0), 2.0 * r_cut, None, 1, per_atom=True)
    assert _equal(one, two, C.COUNTS + C.ROWS) and np.array_equal(two["cutoffs"], np.float32(2.0) * one["cutoffs"])


# ---- 4. the walk case ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_walk_case(engine, split):
    """items of 64, 3 and 3 centres; 0, 1, 2, an odd number, 64 and 65 candidates; a centre truncated at the origins 0 and 3 alone;
    a coincident pair"""
    pos, box, groups, r_cut = C.walk_split() if split else Q.walk_case()
    _resident(engine, pos)
    listing = _listing(groups)
    got = engine.adaptive_common_neighbours(box, r_cut, listing, 1, per_atom=True)
    if not split:
        assert Q.walk_counts(got["n"])
    assert got["types"][[0, 3], 0].tolist() == [-1, -1] and (got["types"] == -1).sum() == 2 and got["n"][[1, 2, 4], 0].tolist() == [64, 64, 64]
    assert np.all(got["bond_signatures"][[0, 3], 0] == C.NO_BOND) and np.all(got["nearest"][[0, 3], 0] == -1)
    assert np.all(np.isnan(got["cutoffs"][[0, 3], 0])) and got["truncated"].tolist() == [2, 0]
    # the centres with 64 candidates are served: 12 or 14 members, all on the sphere of radius 3.0 -- r_A = K x 3.0 up to the
    # noise, r_B = K x 3.0 x (8 x 2 / sqrt 3 + 6) / 14 = K x 3.0 x 1.088
    assert np.all((got["nearest"][[1, 2, 4], 0] >= 0).sum(axis=1) >= 12) and np.all(got["types"][[1, 2, 4], 0] >= 0)
    ratio = got["cutoffs"][[1, 2, 4], 0] / (C.R.K * 3.0)
    assert np.all((ratio > 0.95) & (ratio < 1.12))
    # the centres with 0, 1 and 2 candidates (the far atom, the coincident pair and the third atom) are short, and other
    col = {False: [66, 67, 68, 69], True: [1, 2, 3, 4]}[split]
    assert np.all(got["n"][:, col] <= 2) and np.all(got["types"][:, col] == 0) and np.all(got["nearest"][:, col] == -1)
    assert int(got["short"].sum()) == int((got["n"] < 12).sum()) and int(got["short"].sum()) >= 5 * 4
    _exact(engine, got, pos, box, r_cut, listing, 1, f"walk case split {split}")


# ---- 6. the same bits ------------------------------------------------------------------------------------------------------------
def test_budgets_blocks_and_repeats(engine):
    from psa_amd import _hip
    pos, box, groups, r_cut, ref = _case("hcp", "two", False)
    n, step = pos.shape[1], 1                                              # 6 origins
    listing = _listing(groups)
    _resident(engine, pos)
    whole = engine.adaptive_common_neighbours(box, r_cut, listing, step, per_atom=True)
    assert C.check(whole, ref.result(step), ref.excluded(step), ref.cut_tolerance(step), "hcp whole")
    assert _equal(whole, engine.adaptive_common_neighbours(box, r_cut, listing, step, per_atom=True))
    for origins in (1, 3, 6):                                              # origins per block: 6, 2 and 1 block
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN_BONDS * n * origins + 5)
        assert _equal(whole, engine.adaptive_common_neighbours(box, r_cut, listing, step, per_atom=True)), origins
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n * origins + 5)
        assert _equal(whole, engine.adaptive_common_neighbours(box, r_cut, listing, step), C.COUNTS), origins
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN_BONDS * n - 1)
    with pytest.raises(_hip.PsaHipError, match=f"need {PER_ORIGIN_BONDS * n} bytes"):
        engine.adaptive_common_neighbours(box, r_cut, listing, step, per_atom=True)
    assert _equal(whole, engine.adaptive_common_neighbours(box, r_cut, listing, step), C.COUNTS)   # without the per-bond output it fits
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n - 1)
    with pytest.raises(_hip.PsaHipError, match=f"need {PER_ORIGIN * n} bytes"):
        engine.adaptive_common_neighbours(box, r_cut, listing, step)


def _bonds_of(res, atoms):
    """the set of (origin, centre atom, member atom, word) of the bonds of a result, through `nearest`"""
    out = set()
    for k, a, i in zip(*np.nonzero(res["bond_signatures"] != C.NO_BOND)):
        out.add((int(k), int(atoms[a]), int(atoms[res["nearest"][k, a, i]]), int(res["bond_signatures"][k, a, i])))
    return out


def test_permutation_of_the_atoms(engine):
    """the same counts for any order of the atoms inside a species, the same types once mapped back, and the same (origin, centre
    atom, member atom, word) as sets: the rank labels of exactly tied r2 may swap"""
    pos, box, groups, r_cut, _ = _case("gas", "two", True)
    listing, step = _listing(groups), 3
    _resident(engine, pos)
    whole = engine.adaptive_common_neighbours(box, r_cut, listing, step, per_atom=True)
    rng = np.random.default_rng(8)
    shuffled = [g[rng.permutation(len(g))] for g in listing]
    moved = engine.adaptive_common_neighbours(box, r_cut, shuffled, step, per_atom=True)
    assert _equal(whole, moved, C.COUNTS) and not np.array_equal(whole["bond_signatures"], moved["bond_signatures"])
    sets = [_bonds_of(res, np.concatenate(order)) for res, order in ((whole, listing), (moved, shuffled))]
    assert sets[0] == sets[1] and len(sets[0]) == int(whole["signature_counts"].sum() + whole["signature_outside"].sum())
    back = [np.argsort(np.concatenate(order), kind="stable") for order in (listing, shuffled)]
    for k in ("types", "n", "cutoffs"):
        assert np.array_equal(whole[k][:, back[0]], moved[k][:, back[1]], equal_nan=True), k


# ---- 7. scratch, no trace, the calculator, refusals --------------------------------------------------------------------------
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
        cn = calc.calculate_common_neighbours(rc, per_atom=True)
        sed = calc.calculate(mags, vecs)
        return [np.asarray(ang.counts), np.asarray(ang.coordination_counts), np.asarray(cn.signature_counts), np.asarray(cn.types),
                np.asarray(cn.bond_signatures), np.asarray(sed.intensity if sed.is_complex else sed.sed)]

    def call(eng, loud=False):
        got = eng.adaptive_common_neighbours(box, Q.matrix_cutoff(1.3 * rc, 2), _listing(Q.two_species(37)), 3, per_atom=True)
        return [np.asarray(v).copy() for v in got.values()]
    before = others()
    engine.timings()                                                       # (reset)
    r0 = call(engine)
    assert (r0[5] >= 0).any() and (r0[5] == 0).any()                       # centres that are served and short ones
    t = engine.timings()
    assert all(t[k] > 0 for k in ("gather", "transpose", "phase", "project", "epilogue", "d2h")) and t["project"] <= t["phase"]
    try:
        S.check_poisoned(engine, "adaptive_common_neighbours per atom", call, r0)
    finally:
        engine.scratch_fill(-1)
    for a, b in zip(before, others()):
        assert np.array_equal(a, b, equal_nan=True)


def test_calculator(engine):
    from psa_amd import AdaptiveCommonNeighbours
    pos, box, groups, r_cut, ref = _case("hcp", "two", False)
    types = np.ones(64, np.int32)
    types[groups[1]] = 2
    calc = _calculator(engine, pos, box, types)
    res = calc.calculate_adaptive_common_neighbours(r_cut, basis_atom_types=[1, 2], origin_step=3, per_atom=True)
    raw = engine.adaptive_common_neighbours(box, r_cut, _listing(groups), 3, per_atom=True)
    assert isinstance(res, AdaptiveCommonNeighbours)
    assert all(np.array_equal(getattr(res, k), raw[k], equal_nan=True) for k in C.COUNTS + ("types", "bond_signatures", "cutoffs", "nearest"))
    assert np.array_equal(res.neighbours, raw["n"]) and res.atoms.shape == (64,) and res.origins == 2 and res.sizes.tolist() == [43, 21]
    assert res.structure_names == ("other", "fcc", "hcp", "bcc", "ico") and np.allclose(sum(res.fraction(t) for t in res.structure_names), 1.0)
    assert np.array_equal(res.signature(4, 2, 1), raw["signature_counts"][:, 4, 2, 1]) and 0.0 < res.share(4, 2, 1) < 1.0
    assert np.array_equal(res.atoms_of(1, "hcp"), res.atoms[raw["types"][1] == 2]) and res.atoms_of(1, "hcp").size > 0
    plain = calc.calculate_adaptive_common_neighbours(r_cut, basis_atom_types=[1, 2])
    assert plain.types is None and plain.nearest is None and plain.cutoffs is None and plain.type_counts.shape == (6, 2, 5)
    assert np.array_equal(plain.type_counts[::3], res.type_counts)
    fcc_pos, fcc_box = C.closed_inputs("fcc")[:2]
    fcc = _calculator(engine, fcc_pos, fcc_box).calculate_adaptive_common_neighbours(7.0, per_atom=True)
    assert np.all(fcc.fraction("fcc") == 1.0) and fcc.share(4, 2, 1) == 1.0 and fcc.atoms_of(0, "fcc").size == 256 and not fcc.short.any()
    with pytest.raises(ValueError, match="more than 64 neighbours"):
        _calculator(engine, Q.ball(70, 3, 6.0), Q.CUBIC).calculate_adaptive_common_neighbours(6.0)
    with pytest.raises(TypeError, match="per_atom must be a bool"):
        calc.calculate_adaptive_common_neighbours(r_cut, per_atom=1)


def test_sharded_calculator_refuses(engine):
    pos, box, rc = Q.family("cubic37")
    calc = _calculator(engine, pos, box)

    class Sharded:
        nranks = 2
    calc._shard = Sharded()
    with pytest.raises(NotImplementedError, match="sharded calculator"):
        calc.calculate_adaptive_common_neighbours(rc)


def test_refusals_and_empty_species(engine):
    import ctypes as ct

    from psa_amd import _hip, max_pair_radius
    pos, box, rc = Q.family("cubic37")                                     # 40 frames
    _resident(engine, pos)
    two = _listing(Q.two_species(37))

    def refused(word, r_cut=rc, groups=None, step=1, **kw):
        with pytest.raises(_hip.PsaHipError, match=word):
            engine.adaptive_common_neighbours(box, r_cut, groups, step, **kw)
    refused("origin_step must be at least 1, got 0", step=0)
    refused("r_cut.*beyond the served radius", r_cut=1.01 * max_pair_radius(box))
    refused("r_cut is not symmetric", r_cut=[[3.0, 2.0], [2.5, 3.0]], groups=two)
    refused("must be finite and not negative", r_cut=-1.0)
    refused("must be finite and not negative", r_cut=float("nan"))
    refused("listed twice", groups=[np.array([0, 1], np.int32), np.array([1, 2], np.int32)])
    with pytest.raises(ValueError, match="out of bounds"):                # (the reference's exception type for this one)
        engine.adaptive_common_neighbours(box, rc, [np.array([0, 37], np.int32)])
    refused(r"number of atom groups is in \[1, 8\], got 9", groups=[np.array([i], np.int32) for i in range(9)])
    with pytest.raises(_hip.PsaHipError, match="not the inverse of box"):
        engine.adaptive_common_neighbours(box, rc, box_inverse=2.0 * np.linalg.inv(np.asarray(box, np.float64)))
    with pytest.raises(_hip.PsaHipError, match="must be finite"):
        engine.adaptive_common_neighbours(box, rc, box_inverse=np.full((3, 3), np.nan))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * 37 - 1)
    refused(f"need {PER_ORIGIN * 37} bytes")
    reset(engine)
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        refused("sharded context.*psa_adaptive_common_neighbours|psa_adaptive_common_neighbours.*sharded context")
    finally:
        engine.comm_destroy()
    # what the Engine method cannot get wrong: byte counts that are not exact, null outputs
    a = engine._shell_args(box, None, None, rc, 1)
    u64 = lambda x: x.ctypes.data_as(ct.POINTER(ct.c_uint64))             # noqa: E731
    i32 = lambda x: x.ctypes.data_as(ct.POINTER(ct.c_int32))              # noqa: E731
    u32 = lambda x: x.ctypes.data_as(ct.POINTER(ct.c_uint32))             # noqa: E731
    f32 = lambda x: x.ctypes.data_as(ct.POINTER(ct.c_float))              # noqa: E731
    table, one, census = np.zeros((1, 8, 16, 16), np.uint64), np.zeros(1, np.uint64), np.zeros((40, 1, 5), np.uint64)
    atoms, cuts = np.zeros((40, 37), np.int32), np.zeros((40, 37), np.float32)
    near, bonds = np.zeros((40, 37, 14), np.int32), np.zeros((40, 37, 14), np.uint32)

    def raw(word, table_bytes=table.nbytes, census_bytes=census.nbytes, types=False, n=False, cut=False, atom_bytes=0, nearest=False,
            sigs=False, bond_bytes=0, no_table=False, no_short=False):
        rc_ = engine._lib.psa_adaptive_common_neighbours(
            *a.head, 1, None if no_table else u64(table), table_bytes, u64(one), u64(census), census_bytes, u64(one.copy()),
            None if no_short else u64(one.copy()), i32(atoms) if types else None, i32(atoms.copy()) if n else None,
            f32(cuts) if cut else None, atom_bytes, i32(near) if nearest else None, u32(bonds) if sigs else None, bond_bytes)
        assert rc_ != 0 and word in engine._lib.psa_last_error().decode(), engine._lib.psa_last_error()
    raw("signature_bytes is 16383", table_bytes=table.nbytes - 1)
    raw("type_bytes is 1608", census_bytes=census.nbytes + 8)
    raw("atom_bytes is 0", types=True)
    raw("atom_bytes is 5924", n=True, atom_bytes=atoms.nbytes + 4)
    raw("atom_bytes is 5916", cut=True, atom_bytes=atoms.nbytes - 4)
    raw("bond_bytes is 82879", sigs=True, bond_bytes=bonds.nbytes - 1)
    raw("bond_bytes is 0", nearest=True)
    raw("null output", no_table=True)
    raw("null output", no_short=True)
    ok = engine._lib.psa_adaptive_common_neighbours(*a.head, 1, u64(table), table.nbytes, u64(one), u64(census), census.nbytes, u64(one.copy()),
                                                    u64(one.copy()), None, i32(atoms), None, atoms.nbytes, None, None, 12345)
    assert ok == 0 and atoms.any()                                         # byte counts of outputs not asked for are not read
    ok = engine._lib.psa_adaptive_common_neighbours(*a.head, 1, u64(table), table.nbytes, u64(one), u64(census), census.nbytes, u64(one.copy()),
                                                    u64(one.copy()), None, None, None, 777, i32(near), None, near.nbytes)
    assert ok == 0 and (near != 0).any()                                   # nearest alone
    # empty species: all of them, and one among others
    empty = engine.adaptive_common_neighbours(box, rc, [np.zeros(0, np.int32)], per_atom=True)
    assert not any(empty[k].any() for k in C.COUNTS) and empty["types"].shape == (40, 0) and empty["bond_signatures"].shape == (40, 0, 14)
    assert empty["nearest"].shape == (40, 0, 14) and empty["cutoffs"].shape == (40, 0)
    three = _listing(Q.three_species(37))
    got = engine.adaptive_common_neighbours(box, rc, three, 5, per_atom=True)
    assert not got["signature_counts"][1].any() and not got["type_counts"][:, 1].any() and got["type_counts"][:, [0, 2]].any()
    assert engine.adaptive_common_neighbours(box, 1.3 * rc)["signature_counts"].any()
