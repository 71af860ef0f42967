"""The local order parameters on the GPU (psa_local_order, psa_debug_qlm, their Engine methods and the calculator method): Q by
`debug_qlm` and the per-atom qbar2, W, S and xi against the spherical-angle float64 reference of tests/qlm64.py inside the
allowances of tests/qlm_cases.py -- random walks with one, two and three species, a scalar cut-off and a matrix with a zero
entry, one, two and four orders, the origin steps --; the edges of the centre tile and of the item; centres with 0 to 64
neighbours; a truncated ball and its incomplete surroundings; a coincident pair; lattices whose values are known; every
histogram against its bin rule applied to the returned values, exactly; every identity; consistency with psa_bond_order and
psa_debug_neighbour_lists; budgets, blocks and repeated calls bit for bit; permutations; the calculator; every refusal; no
trace in later calls.

Every comparison first asserts the excluded share under the cap, then prints the largest shares of the allowances."""
import functools

import numpy as np
import pytest

import angle64 as A
import angle_cases as Q
import order_cases as OC
import pair_cases as P
import qlm64 as L
import qlm_cases as C
import scratch_cases as S
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = Q.BOXES
PER_ORIGIN = 1040                                                          # work bytes per atom and origin of the lists


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


def _table(ls):
    from psa_amd import local_order
    return local_order.w3j_blocks(ls)


@functools.lru_cache(maxsize=None)
def _walk(box, n_atoms, n_frames, seed=11):
    return P.walk(n_atoms, n_frames, seed, box=BOXES[box])["wrapped"]


def _named(raw):
    return dict(zip(("hist", "qbar2", "w", "wbar", "xi", "n"), raw))


def _call(engine, box, rc, ls, n_q, n_w, listing, step=1, solid_l=None, thr=0.7, per_atom=True, w_range=0.2):
    return _named(engine.local_order(box, rc, ls, n_q, n_w, _table(ls), listing, step, w_range, ls[-1] if solid_l is None else solid_l, thr,
                                     per_atom))


def _held(engine, pos, box, groups, listing, rc, step, ls, n_q, n_w, what, ref=None, thr=0.7):
    """one call with per-atom output held to the reference, the bin rules and the identities, and Q of the first and the last
    origin by debug_qlm; returns what the engine gave"""
    ref = C.reference(pos, box, groups, rc, step, list(ls), ls[-1], thr) if ref is None else ref
    assert C.excluded_share(ref) <= C.EXCLUDED_CAP and C.loose_share(ref) <= C.EXCLUDED_CAP, what     # before anything else
    _resident(engine, pos)
    got = _call(engine, box, rc, ls, n_q, n_w, listing, step, thr=thr)
    S_, n_o, n_a, n_l = len(groups), A.n_origins(pos.shape[0], step), sum(len(g) for g in groups), len(ls)
    assert got["hist"].dtype == np.uint64 and got["hist"].shape == (S_, n_l * n_q + 2 * n_l * n_w + 65 + 4 + 4 * n_l)
    assert all(got[k].dtype == np.float64 and got[k].shape == (n_o, n_a, n_l) for k in ("qbar2", "w", "wbar"))
    assert all(got[k].dtype == np.int32 and got[k].shape == (n_o, n_a) for k in ("xi", "n"))
    assert C.check(got, ref, what), what
    sizes = [len(g) for g in groups]
    assert np.array_equal(C.fold_left_out(got["hist"], n_l, n_q, n_w), C.rows_of(got, sizes, n_l, n_q, n_w, 0.2)), what   # the bin rules, exactly
    assert C.identities(got["hist"], sizes, n_o, n_l, n_q, n_w), what
    at = n_l * n_q + 2 * n_l * n_w + 65
    start = np.concatenate([[0], np.cumsum(sizes)])
    kinds = np.array([[(ref["why"][:, start[s]:start[s + 1]] == k).sum() for k in (1, 2, 3, 4)] for s in range(S_)], np.int64)
    if not ref["excluded"].any():
        assert np.array_equal(got["hist"][:, at:at + 4].astype(np.int64), kinds.reshape(S_, 4)), what   # each kind of centre left out
    for o in sorted({0, n_o - 1}):
        q = engine.debug_qlm(box, rc, o * step, ls, listing)
        assert q.dtype == np.int64 and q.shape == (n_a, sum(l + 1 for l in ls), 2) and C.check_q(q, ref, o, f"{what} origin {o}"), what
    return got


# ---- random walks against the reference -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family_reference(name, kind, matrix, step, ls):
    pos, box, r_cut = C.family(name)
    groups = _groups(kind, pos.shape[1])
    rc = Q.matrix_cutoff(r_cut, len(groups)) if matrix else r_cut
    return pos, box, groups, rc, C.reference(pos, box, groups, rc, step, list(ls), ls[-1], 0.7)


@pytest.mark.parametrize("name,kind,matrix,step,ls", [
    ("cubic130", "one", False, 1, (4, 6)), ("triclinic130", "one", False, 1, (4, 6)), ("cubic37", "one", False, 1, (4, 6)),
    ("triclinic257", "one", False, 1, (4, 6)), ("cubic130", "two", True, 3, (2,)), ("triclinic130", "three", False, 1, (12,)),
    ("cubic37", "three", True, 3, (6, 8, 10, 12)), ("triclinic257", "two", False, 1, (4, 6))])
def test_per_atom_against_the_reference(engine, name, kind, matrix, step, ls):
    pos, box, groups, rc, ref = _family_reference(name, kind, matrix, step, ls)
    got = _held(engine, pos, box, groups, _listing(kind, groups), rc, step, ls, 200, 200, f"{name} {kind} matrix {matrix} step {step} ls {ls}",
                ref)
    if kind == "three":
        assert not got["hist"][1].any()                                     # the empty species


# ---- the edges of the tile, the item and the list --------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [63, 64, 65, 255, 256, 257])
def test_tile_and_item_edges(engine, n_atoms):
    pos = _walk("triclinic", n_atoms, 2)
    _held(engine, pos, Q.TRICLINIC, [np.arange(n_atoms)], None, 5.0 if n_atoms > 100 else 8.0, 1, (4, 6), 7, 7, f"{n_atoms} centres")


@pytest.mark.parametrize("n_on", [0, 1, 2, 3, 63, 64])
def test_neighbour_counts_of_a_centre(engine, n_on):
    """a centre with exactly n_on atoms on a sphere around it; the atoms on the sphere bond to the centre alone, so each has one
    leg: its Q is a single harmonic, S = sum |Q|^2 2^-80 = 1, and its w is that harmonic's"""
    pos = Q.sphere(max(n_on, 1), 3.0)
    groups = [np.arange(1), np.arange(1, pos.shape[1])]
    listing = [np.asarray(g, np.int32) for g in groups]
    rc = np.array([[0.0, 3.5 if n_on else 0.0], [3.5 if n_on else 0.0, 0.0]])
    ls = (2, 4, 6)
    got = _held(engine, pos, Q.CUBIC, groups, listing, rc, 1, ls, 1024, 1024, f"sphere of {n_on}")
    assert got["n"][0, 0] == n_on
    if n_on == 0:
        assert np.all(got["xi"] == -1) and np.all(np.isnan(got["qbar2"])) and got["hist"][:, 3 * 3 * 1024 + 65 + 1].tolist() == [1, 1]
        return
    assert np.all(got["n"][0, 1:] == 1) and np.all(got["xi"] >= 0)
    q = engine.debug_qlm(Q.CUBIC, rc, 0, ls, listing)
    at = 0
    for j, l in enumerate(ls):
        one = C.full_vector(q[1:, at:at + l + 1], l)
        assert np.abs((np.abs(one) ** 2).sum(axis=1) - 1.0).max() <= (2 * l + 1) * 2.0 ** -38
        legs = pos[0, 1:].astype(np.float64) - pos[0, 0].astype(np.float64)
        want = np.array([L.w_hat(-leg[None], l) for leg in legs])           # (the leg of a sphere atom points at the centre)
        assert np.abs(got["w"][0, 1:, j] - want).max() <= 1e-5
        at += l + 1


def test_truncated_ball_and_its_incomplete_surroundings(engine):
    """66 atoms in a ball are truncated; two atoms beside it see part of the ball: incomplete; three far away see each other"""
    ball = Q.ball(66, 2, 6.0, n_outside=3)
    H = np.asarray(Q.CUBIC, np.float32).astype(np.float64)
    centre = np.array([0.3, 0.4, 0.5]) @ H
    side = np.stack([centre + [8.0, 0.0, 0.0], centre - [0.0, 8.0, 0.0]]).astype(np.float32)
    pos = np.ascontiguousarray(np.concatenate([ball, np.broadcast_to(side, (2, 2, 3))], axis=1))
    groups = [np.arange(pos.shape[1])]
    ref = C.reference(pos, Q.CUBIC, groups, 6.0, 1, [4, 6], 6, 0.7)
    assert np.all(ref["why"][:, :66] == 1) and np.all(ref["why"][:, 69:] == 4) and np.all(ref["why"][:, 66:69] == 0)
    assert np.all((ref["n"][:, 69:] > 0) & (ref["n"][:, 69:] <= 64))
    got = _held(engine, pos, Q.CUBIC, groups, None, 6.0, 1, (4, 6), 50, 50, "ball", ref)
    at = 2 * 50 + 4 * 50 + 65
    assert got["hist"][0, at:at + 4].tolist() == [132, 0, 0, 4] and np.all(got["n"][:, :66] >= 65)    # (65 in the ball, and the atoms beside it)
    calc = _calculator(engine, pos, Q.CUBIC)
    with pytest.raises(ValueError, match="species 0: 132.*smaller r_cut"):
        calc.calculate_local_order(6.0)


def test_coincident_pair(engine):
    """two atoms at one place: each has a leg of length 0 and is undefined at every origin; their other neighbours are
    incomplete; everyone else is what the reference says"""
    pos = _walk("cubic", 37, 12).copy()
    pos[:, 5] = pos[:, 9]
    groups = [np.arange(37)]
    ref = C.reference(pos, Q.CUBIC, groups, 8.0, 1, [4, 6], 6, 0.7)
    assert np.all(ref["why"][:, [5, 9]] == 3) and (ref["why"] == 3).sum() == 24 and (ref["why"] == 4).sum() > 24 and (ref["why"] == 0).sum() > 100
    got = _held(engine, pos, Q.CUBIC, groups, None, 8.0, 1, (4, 6), 200, 200, "coincident", ref)
    at = 2 * 200 + 4 * 200 + 65
    assert got["hist"][0, at + 2] == 24 and got["hist"][0, at + 3] == (ref["why"] == 4).sum() and np.all(got["xi"][:, [5, 9]] == -1)


# ---- known structures -------------------------------------------------------------------------------------------------------
W_KNOWN = {"fcc": (-0.159317, -0.013161), "hcp": (+0.134097, -0.012442), "bcc8": (-0.159317, +0.013161)}


@pytest.mark.parametrize("name", ["diamond", "fcc", "bcc8", "bcc14", "hcp"])
def test_known_structures(engine, name):
    """every atom of a perfect lattice has the same shell: every histogram one spike, xi = n, q-bar = q and w-bar = w"""
    pos, box, rc, n_nb = {"diamond": lambda: (Q.diamond(2)[0], Q.CUBIC, 2.8, 4), "fcc": lambda: (C.fcc_block(), Q.CUBIC, 4.6, 12),
                          "bcc8": lambda: (C.bcc_block(), Q.CUBIC, 5.0, 8), "bcc14": lambda: (C.bcc_block(), Q.CUBIC, 6.0, 14),
                          "hcp": lambda: C.hcp_block() + (3.5, 12)}[name]()
    n_atoms, ls = pos.shape[1], (4, 6)
    got = _held(engine, pos, box, [np.arange(n_atoms)], None, rc, 1, ls, 200, 200, name)
    assert np.all(got["n"] == n_nb) and np.all(got["xi"] == n_nb)
    q2 = OC.reference(pos[:1], box, [np.arange(n_atoms)], rc, 1, list(ls))["xq"][0, 0] / n_nb ** 2      # q_l^2 of the shell
    for j, l in enumerate(ls):
        assert np.abs(got["qbar2"][..., j] - q2[j]).max() <= 1e-5 and np.abs(got["wbar"][..., j] - got["w"][..., j]).max() <= 1e-4
        for part, (lo, width, value) in enumerate(((0, 200, got["qbar2"][0, 0, j]), (400, 200, got["w"][0, 0, j]), (800, 200, got["wbar"][0, 0, j]))):
            row = got["hist"][0, lo + j * width:lo + (j + 1) * width].astype(np.int64)
            spike = np.zeros(width, np.int64)
            spike[C.q_bin(value, 200) if part == 0 else C.w_bin(value, 200, 0.2)] = 2 * n_atoms
            assert np.array_equal(row, spike), (name, l, part)
        if name in W_KNOWN:
            assert abs(got["w"][0, 0, j] - W_KNOWN[name][j]) <= 2e-5, (name, l)
    assert got["hist"][0, 1200 + n_nb] == 2 * n_atoms


def test_icosahedral_cluster(engine):
    pos = C.icosahedral_cluster()
    got = _held(engine, pos, Q.CUBIC, [np.arange(13)], None, 3.1, 1, (6,), 200, 200, "icosahedron")
    assert got["n"][0].tolist() == [12] + [1] * 12 and abs(got["w"][0, 0, 0] + 0.169754) <= 2e-5


# ---- the histograms, the identities, the other entries ------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 7, 200, 1024])
def test_histograms_are_the_bin_rules(engine, bins):
    pos, box, groups, rc, ref = _family_reference("triclinic130", "three", False, 1, (12,))
    _held(engine, pos, box, groups, _listing("three", groups), rc, 1, (12,), bins, 1025 - bins if bins in (1, 1024) else bins, f"bins {bins}", ref)


def test_consistency_with_bond_order_and_the_lists(engine):
    """sum_m |Q_lm|^2 2^-80 = n^2 q_l^2 is what psa_bond_order returns as X 2^-24: inside the sum of the two allowances"""
    pos, box, groups, rc, ref = _family_reference("triclinic130", "one", False, 1, (4, 6))
    oref = OC.reference(pos, box, groups, rc, 1, [4, 6])
    _resident(engine, pos)
    x, n_order = engine.bond_order(box, rc, (4, 6), 10, per_atom=True)[4:]
    got = _call(engine, box, rc, (4, 6), 10, 10, None)
    assert np.array_equal(got["n"], n_order)
    for o in range(pos.shape[0]):
        assert np.array_equal(got["n"][o], engine.debug_neighbour_lists(box, rc, o)[0])
    q = engine.debug_qlm(box, rc, 0, (4, 6))
    keep, at = (ref["why"][0] == 0) & ~ref["excluded"][0], 0
    for j, l in enumerate((4, 6)):
        v = C.full_vector(q[:, at:at + l + 1], l)
        s, norm, E = (np.abs(v) ** 2).sum(axis=1), np.linalg.norm(ref["v"][j][0], axis=1), ref["E"][j][0]
        allowed = 2.0 * norm * E + E * E + oref["allowed"][0, :, j] + 1e-9
        assert np.all(np.abs(s - x[0, :, j] / OC.ONE)[keep] <= allowed[keep])
        at += l + 1


# ---- bit for bit ----------------------------------------------------------------------------------------------------------
def _equal(x, y):
    return all((a is None and b is None) or np.array_equal(a, b, equal_nan=True) for a, b in zip(x.values(), y.values()))


def test_budgets_blocks_and_repeats(engine):
    from psa_amd import _hip
    pos, box, r_cut = C.family("cubic37")                                  # 40 frames
    n = pos.shape[1]
    groups = Q.two_species(n)
    listing = _listing("two", groups)
    rc = Q.matrix_cutoff(r_cut, 2)
    ls, cols = (4, 6, 12), 5 + 7 + 13
    _resident(engine, pos)
    whole = _call(engine, box, rc, ls, 200, 100, listing, solid_l=6)
    assert whole["hist"].any() and _equal(whole, _call(engine, box, rc, ls, 200, 100, listing, solid_l=6))
    bare = _call(engine, box, rc, ls, 200, 100, listing, solid_l=6, per_atom=False)
    assert bare["qbar2"] is None and bare["xi"] is None and np.array_equal(bare["hist"], whole["hist"])
    for origins in (1, 7, 39):                                             # origins per block: 40, 6 and 2 blocks
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, (PER_ORIGIN + 16 * cols + 24 * 3 + 8) * n * origins + 5)
        assert _equal(whole, _call(engine, box, rc, ls, 200, 100, listing, solid_l=6)), origins
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, (PER_ORIGIN + 16 * cols) * n * origins + 5)
        assert np.array_equal(whole["hist"], _call(engine, box, rc, ls, 200, 100, listing, solid_l=6, per_atom=False)["hist"]), origins
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, (PER_ORIGIN + 16 * cols) * n - 1)
    with pytest.raises(_hip.PsaHipError, match=f"need {(PER_ORIGIN + 16 * cols) * n} bytes"):
        _call(engine, box, rc, ls, 200, 100, listing, solid_l=6, per_atom=False)


def test_walk_case_is_the_twin_exactly(engine):
    """`angle_cases.walk_case`, every branch of the centre walk of both passes: its five origins in blocks of 2, 2 and 1, and
    the five frames 200 times over in one block -- 3 items x 1000 origins are more workgroups than the 2696 that rows of
    6221 words leave the partials, so a slab holds two origins and a wavefront walks on from one into the next.  Q, q-bar^2,
    w, w-bar, the connections and n are the twin's (qlm_cases.model), exactly; the histograms are the bin rules of them"""
    from psa_amd import _hip
    pos, box, groups, rc = Q.walk_case()
    listing = [np.asarray(g, np.int32) for g in groups]
    ls, n_a = (4, 6), 70
    want = C.model(pos, box, groups, rc, 1, ls)
    assert Q.walk_counts(want["n"]) and (want["xi"] >= 0).any()

    rows = C.rows_of(want, [67, 3], 2, 1024, 1024, 0.2)                    # the bin rules of the twin's values, once

    def same(got, reps):
        return (all(np.array_equal(got[k], np.tile(want[k], (reps, 1, 1)), equal_nan=True) for k in ("qbar2", "w", "wbar"))
                and all(np.array_equal(got[k], np.tile(want[k], (reps, 1))) for k in ("xi", "n"))
                and np.array_equal(C.fold_left_out(got["hist"], 2, 1024, 1024), reps * rows))

    _resident(engine, pos)
    for f in range(5):
        assert np.array_equal(engine.debug_qlm(box, rc, f, ls, listing), want["q"][f]), f
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, (PER_ORIGIN + 16 * 12 + 24 * 2 + 8) * n_a * 2 + 5)
    assert same(_call(engine, box, rc, ls, 1024, 1024, listing), 1)
    reset(engine)
    _resident(engine, np.tile(pos, (200, 1, 1)))
    assert same(_call(engine, box, rc, ls, 1024, 1024, listing), 200)


def test_permutation_of_the_atoms(engine):
    """Q is the same bits after undoing the permutation, and so are n, xi and w; the gather of q-bar runs in another order:
    qbar2 moves by at most (n + 2) roundings of terms below 1, 2 (n + 2) 2^-53 (1 + qbar2), and w-bar = W / S^(3/2) by
    3 (n + 2) 2^-52 / sqrt(qbar2) relative to the largest |w| (1); a centre's bin may move only where its value is that close to
    an edge"""
    pos, box, r_cut = C.family("cubic37")
    groups = Q.two_species(37)
    listing = _listing("two", groups)
    _resident(engine, pos)
    whole = _call(engine, box, r_cut, (4, 6), 200, 200, listing)
    rng = np.random.default_rng(8)
    perms = [rng.permutation(len(g)) for g in listing]
    shuffled = [g[p] for g, p in zip(listing, perms)]
    moved = _call(engine, box, r_cut, (4, 6), 200, 200, shuffled)
    at = np.concatenate([np.argsort(p) + s for p, s in zip(perms, (0, len(listing[0])))])   # undo: column of atom i after the shuffle
    for f in (0, 39):
        assert np.array_equal(engine.debug_qlm(box, r_cut, f, (4, 6), shuffled)[at], engine.debug_qlm(box, r_cut, f, (4, 6), listing))
    for k in ("n", "xi", "w"):
        assert np.array_equal(moved[k][:, at], whole[k], equal_nan=True), k
    kept = whole["xi"] >= 0
    n2 = (whole["n"][kept].astype(np.float64) + 2.0)[:, None]
    a, b = whole["qbar2"][kept], moved["qbar2"][:, at][kept]
    bound_q = 2.0 * n2 * 2.0 ** -53 * (1.0 + a)
    assert np.all(np.abs(a - b) <= bound_q)
    wa, wb = whole["wbar"][kept], moved["wbar"][:, at][kept]
    bound_w = 3.0 * n2 * 2.0 ** -52 / np.sqrt(a) + 2.0 ** -50
    assert np.all(np.abs(wa - wb) <= bound_w)
    near_q = np.array([[C.q_bin(v - d, 200) != C.q_bin(v + d, 200) for v, d in zip(r, dr)] for r, dr in zip(a, bound_q)])
    near_w = np.array([[C.w_bin(v - d, 200, 0.2) != C.w_bin(v + d, 200, 0.2) for v, d in zip(r, dr)] for r, dr in zip(wa, bound_w)])
    if not near_q.any() and not near_w.any():
        assert np.array_equal(whole["hist"], moved["hist"])
    else:
        assert np.abs(whole["hist"].astype(np.int64) - moved["hist"].astype(np.int64)).sum() <= 2 * (near_q.sum() + near_w.sum())


# ---- no trace -----------------------------------------------------------------------------------------------------------
def test_no_trace(engine):
    """scratch memory filled with zeros and with NaN patterns before the call changes nothing; `angle_histogram`, `bond_order`,
    `pair_histogram` and `van_hove_self` give the bits they gave before the local-order calls in between"""
    pos, box, r_cut = C.family("cubic37")
    _resident(engine, pos)

    def others():
        return (*engine.angle_histogram(box, r_cut, 45), *engine.bond_order(box, r_cut, (4, 6), 50, per_atom=True),
                engine.pair_histogram(box, [0, 3], 0.25, 40), engine.van_hove_self(box, [0, 5], 0.25, 40, None, 2, True))

    def call(eng, loud=False):
        got = _call(eng, box, r_cut, (4, 6, 12), 64, 64, None, 3, solid_l=6)
        return [np.asarray(v).copy() for v in got.values()]
    before = others()
    engine.timings()                                                       # (reset)
    r0 = call(engine)
    t = engine.timings()
    assert t["gather"] > 0 and t["transpose"] > 0 and t["phase"] > 0 and t["epilogue"] > 0 and t["d2h"] > 0 and t["fft"] == 0
    try:
        S.check_poisoned(engine, "local_order per atom", call, r0)
    finally:
        engine.scratch_fill(-1)
    for a, b in zip(before, others()):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- the calculator and the refusals -----------------------------------------------------------------------------------------
def _calculator(engine, pos, box, types=None, dt=0.002):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, 1, 1, 1).attach(engine=engine)


def test_calculator(engine):
    from psa_amd import LocalOrder
    pos, box, groups, rc, ref = _family_reference("cubic130", "two", True, 3, (2,))
    types = np.ones(130, np.int32)
    types[groups[1]] = 2
    calc = _calculator(engine, pos, box, types)
    res = calc.calculate_local_order(rc, (2,), 50, 40, basis_atom_types=[1, 2], origin_step=3, solid_l=2, per_atom=True)
    assert isinstance(res, LocalOrder) and all(np.array_equal(a, b) for a, b in zip(res.groups, groups)) and res.origins == 4
    raw = _call(engine, box, rc, (2,), 50, 40, _listing("two", groups), 3)
    assert np.array_equal(res.neighbours, raw["n"]) and np.array_equal(res.connections_atoms, raw["xi"]) and C.check(raw, ref, "calculator")
    assert np.array_equal(res.qbar_atoms, np.sqrt(raw["qbar2"]), equal_nan=True) and np.array_equal(res.w_atoms, raw["w"], equal_nan=True)
    assert np.array_equal(res.qbar_counts.ravel(), raw["hist"][:, :50].ravel()) and np.array_equal(res.connections, raw["hist"][:, 130:195])
    assert np.array_equal(res.samples, [4 * 90, 4 * 40]) and res.mean.shape == (2, 1)
    assert np.all(res.qbar_counts.sum(axis=2)[:, 0] + res.truncated + res.isolated + res.undefined + res.incomplete == res.samples)
    xi = raw["xi"][:, :90]
    assert res.solid_fraction(1)[0] == pytest.approx((xi[xi >= 0] >= 1).mean())
    plain = calc.calculate_local_order(6.0)
    assert plain.qbar_counts.shape == (1, 2, 200) and plain.w_counts.shape == (1, 2, 200) and plain.qbar_atoms is None and plain.origins == 12


def test_refusals(engine):
    from psa_amd import _hip
    pos = _walk("triclinic", 37, 12)
    _resident(engine, pos)
    box, t46 = Q.TRICLINIC, _table((4, 6))

    def refused(word, ls=(4, 6), n_q=45, n_w=45, table=t46, **kw):
        with pytest.raises(_hip.PsaHipError, match=word):
            engine.local_order(box, 5.0, ls, n_q, n_w, table, **kw)
    assert engine.local_order(box, 5.0, (4, 6), 45, 45, t46)[0].any()
    refused("is odd.*vanishes identically", ls=(4, 5), table=_table((4, 5)), solid_l=4)
    refused("is odd", ls=(3,), table=_table((3,)), solid_l=3)
    refused("number of orders", ls=(2, 4, 6, 8, 10), table=_table((2, 4, 6, 8, 10)))
    refused("number of orders", ls=(), table=np.zeros(0))
    refused(r"outside \[2, 12\]", ls=(4, 14), table=_table((4, 14)))
    refused("strictly ascending", ls=(6, 4), table=_table((6, 4)))
    refused("solid_l = 8 is not among ls", solid_l=8)
    for bad in (0.0, 1.5, -0.5, float("nan")):
        refused("threshold", solid_threshold=bad)
    for bad in (0.0, -0.2, float("inf")):
        refused("w_range", w_range=bad)
    refused("number of q bins", n_q=0)
    refused("number of q bins", n_q=1025)
    refused("number of w bins", n_w=1025)
    refused("w3j holds", table=t46[:-1])
    refused("no 3j symbol", table=np.where(np.arange(t46.size) == 7, np.nan, t46))
    refused("origin_step", origin_step=0)
    with pytest.raises(_hip.PsaHipError, match="is odd"):
        engine.debug_qlm(box, 5.0, 0, (5,))
    with pytest.raises(_hip.PsaHipError, match="frame 12"):
        engine.debug_qlm(box, 5.0, 12, (4,))
    # a context that holds a communicator (one rank is enough) is refused, and serves again once the communicator is gone
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        with pytest.raises(_hip.PsaHipError, match="sharded context.*psa_local_order|psa_local_order.*sharded context"):
            engine.local_order(box, 5.0, (4, 6), 45, 45, t46)
    finally:
        engine.comm_destroy()
    assert engine.local_order(box, 5.0, (4, 6), 45, 45, t46)[0].any()
