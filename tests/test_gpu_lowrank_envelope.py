"""The low-rank k-path route (api_lowrank.hip, k1_planes_diff.hip, lowrank_combine.hip) against a float64 reference
(tests/ref64.py) at the edges of what its plan accepts: other lattice directions and the negative side, segments
away from Gamma, D at its limit (positions far from the origin, k-vectors off the line, mass weights), row tails of
the D pass's 512-row blocks and of the combine's 64-row / odd-row staging, frame and atom tails, incoherent groups
with different plans, long lists cut into k-blocks and split invariance.

Every case forces the route on (any list length, any launch size, planes for every group) and checks, besides the
global max-norm error, the error of each k-row against that row's own maximum.  In the "D at its limit" cases the
line-only reference (the route with its D term lost) must lie at least 10x the tolerance away from the true one, so a
D pass that is wrong cannot pass.  Each case prints its route, its errors and that margin."""
import time

import numpy as np
import pytest

from conftest import rel_max
from lowrank_cases import D_LIMIT, DIRECTIONS, LIMITS, N_ATOMS, geometry, mass_weights
from ref64 import intensity64, row_rel, sed64
from engine_state import reset

pytestmark = pytest.mark.gpu

TOL, TOL_ROW = 1e-6, 2e-6               # complex SED: global max-norm, worst row against its own max
SLOT = 1                                # _hip.SLOT_POSITIONS, projected as it is (no displacement flag)


def _force(engine):
    from psa_amd import _hip
    for opt, val in ((_hip.OPT_K1_LOWRANK, 1), (_hip.OPT_K1_LOWRANK_MIN_K, 1), (_hip.OPT_K1_LOWRANK_MIN_LOCAL, 1),
                     (_hip.OPT_PLANES_EAGER, 1), (_hip.OPT_PLANES_MIN_K, 1)):
        engine.set_option(opt, val)


@pytest.fixture
def forced(engine):
    _force(engine)
    try:
        yield engine
    finally:
        reset(engine)
        engine.release(SLOT)


def _data(T, N, seed):
    """seeded random velocities: every k-row of comparable magnitude"""
    return np.random.default_rng(seed).standard_normal((T, N, 3)).astype(np.float32)


def _project(engine, x, r, k, groups=None, flags=0, parts=None):
    """engine.project over the parts [lo, hi) of the list (one call each) + finalize; and the launches on the route"""
    T, K = x.shape[0], len(k)
    engine.ensure_resident(SLOT, x)
    n0 = engine.lowrank_launches()
    for lo, hi in parts or [(0, K)]:
        engine.project(SLOT, r, k[lo:hi], groups, flags, K_total=K, k_offset=lo)
    out = engine.finalize(T, K, bool(flags & 0x2))
    return out, engine.lowrank_launches() - n0


def _plan(k, r, idx=None, interval=None):
    from psa_amd import _hip
    p = _hip.lowrank_plan(k, r, idx)
    assert p is not None, "the plan declines the list"
    if interval is not None:
        assert p["interval"] == interval, p["interval"]
    return p


def _refs(x, r, k, idx=None, weights=None):
    """the float64 reference of one group and its line-only form (the line: the plan's u and k0, the same for every
    group of a list)"""
    return sed64(x, r, k, idx, weights), sed64(x, r, k, idx, weights, line=_plan(k, r, idx))


def _check(name, got, refs, launches, want_launches=1, tol=TOL, tol_row=TOL_ROW, sees_d=False, t0=None):
    """route taken, global and per-row error within bounds; refs = (reference, line-only reference), whose distance
    (the margin) is printed, and must be 10x the tolerance where the case is to see D"""
    ref, line = refs
    err, rows = rel_max(got, ref), row_rel(got, ref)
    margin = rel_max(line, ref)
    msg = (f"{name}: route {launches}/{want_launches} launches, rel_max {err:.2e}, worst row {rows.max():.2e} "
           f"(k {int(np.argmax(rows))}), line-only {margin:.2e} = {margin / tol:.1f} x tol"
           + (f", {time.perf_counter() - t0:.2f} s" if t0 is not None else ""))
    print(msg)
    assert launches == want_launches, msg
    assert np.all(np.isfinite(got)), msg
    assert err <= tol and rows.max() <= tol_row, msg
    if sees_d:
        assert margin >= 10 * tol, msg


# ---- directions, sides, segments away from Gamma ----------------------------------------------------------------
@pytest.mark.parametrize("name", DIRECTIONS)
def test_directions_and_sides(forced, name):
    t0 = time.perf_counter()
    k, r, interval = geometry(name)
    _plan(k, r, interval=interval)
    x = _data(256, len(r), 21)
    got, n = _project(forced, x, r, k)
    _check(name, got, _refs(x, r, k), n, t0=t0)


# ---- D at its limit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LIMITS + ["limit_shift_weighted"])
def test_d_at_its_limit(forced, name):
    t0 = time.perf_counter()
    k, r, interval = geometry(name.replace("_weighted", ""))
    p = _plan(k, r, interval=interval)
    assert D_LIMIT[0] <= p["d_bound"] <= D_LIMIT[1], p["d_bound"]
    w = mass_weights(len(r), 4) if name.endswith("_weighted") else None
    x = _data(256, len(r), 22)
    if w is not None:
        forced.set_atom_weights(w)
    got, n = _project(forced, x, r, k)
    _check(name + f" (d_bound {p['d_bound']:.2e})", got, _refs(x, r, k, weights=w), n, sees_d=True, t0=t0)


# ---- row tails: D pass M blocks of 512 rows (256 k-vectors), combine stages of 64 rows and odd last rows ----------
@pytest.mark.parametrize("K", [2, 3, 63, 64, 65, 129, 255, 256, 257, 513, 1025])
def test_row_tails(forced, K):
    t0 = time.perf_counter()
    k, r, _ = geometry("dir_1-10", K)
    _plan(k, r, interval=0)
    x = _data(64, len(r), 23)
    got, n = _project(forced, x, r, k)
    _check(f"K={K}", got, _refs(x, r, k), n, t0=t0)


# ---- frame and atom tails ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 16, 17, 65, 1000])
def test_frame_tails(forced, T):
    t0 = time.perf_counter()
    k, r, _ = geometry("dir_111")
    x = _data(T, len(r), 24)
    got, n = _project(forced, x, r, k)
    _check(f"T={T}", got, _refs(x, r, k), n, t0=t0)


@pytest.mark.parametrize("case", ["n_g=1", "n_g=31", "n_g=33", "dups"])
def test_atom_tails(forced, case):
    t0 = time.perf_counter()
    k, r, _ = geometry("dir_210")
    rng = np.random.default_rng(25)
    if case == "dups":
        idx = rng.integers(0, len(r), 40).astype(np.int32)
        idx[5] = idx[6] = idx[30]
    else:
        idx = rng.choice(len(r), int(case.split("=")[1]), replace=False).astype(np.int32)
    _plan(k, r, idx, interval=0)
    x = _data(100, len(r), 26)
    got, n = _project(forced, x, r, k, groups=[idx])
    _check(case, got, _refs(x, r, k, idx), n, t0=t0)


# ---- incoherent groups whose plans differ -------------------------------------------------------------------------
def test_incoherent_groups_with_different_plans(forced):
    """A thin slab across u, the whole box and one atom: three plans (x_c, node interval width), three uploads of L,
    phi and the fp64 table, one after the other.  The lone atom moves sqrt(N) times faster, so its group is not lost in
    the sum."""
    from psa_amd import _hip
    t0 = time.perf_counter()
    k, r, _ = geometry("plain_100")
    x_u = r[:, 0]
    slab = np.flatnonzero((x_u > 5.0) & (x_u < 7.0)).astype(np.int32)
    one = np.array([int(np.argmin(x_u))], np.int32)
    groups = [slab, np.arange(len(r), dtype=np.int32), one]
    plans = [_plan(k, r, g, interval=0) for g in groups]
    for a in range(3):
        for b in range(a + 1, 3):
            assert plans[a]["x_c"] != plans[b]["x_c"] and plans[a]["width"] != plans[b]["width"], (a, b)
    x = _data(128, len(r), 27)
    x[:, one[0], :] *= np.float32(np.sqrt(len(r)))
    got, n = _project(forced, x, r, k, groups=groups, flags=_hip.F_INTENSITY)
    refs = intensity64(x, r, k, groups), intensity64(x, r, k, groups, line=plans[1])
    _check("incoherent 3 groups", got, refs, n, want_launches=3, tol=2 * TOL, tol_row=2 * TOL_ROW, t0=t0)


# ---- long lists cut into k-blocks (PSA_PHASE_TABLE_MIB) -----------------------------------------------------------
def test_long_list_in_k_blocks(forced, monkeypatch):
    t0 = time.perf_counter()
    K = 1100
    k, r, _ = geometry("dir_1-10", K)
    x = _data(64, len(r), 28)
    whole, n = _project(forced, x, r, k)
    _check(f"K={K} uncut", whole, _refs(x, r, k), n)
    monkeypatch.setenv("PSA_PHASE_TABLE_MIB", "1")     # 16 KiB of table per k-vector at 2048 atoms: 64 per block
    cut, n = _project(forced, x, r, k)
    n_blocks = -(-K // 64)
    print(f"K={K} in {n_blocks} k-blocks: {n} launches on the route, {time.perf_counter() - t0:.2f} s")
    assert n == n_blocks
    assert np.array_equal(cut.view(np.uint32), whole.view(np.uint32))


# ---- split invariance on the negative side and away from Gamma ----------------------------------------------------
@pytest.mark.parametrize("name", ["neg_-1-10", "seg_1"])
def test_split_invariance(forced, name):
    k, r, _ = geometry(name)
    K = len(k)
    x = _data(128, len(r), 29)
    whole, n = _project(forced, x, r, k)
    _check(name + " whole", whole, _refs(x, r, k), n)
    for parts in ([(0, K // 2), (K // 2, K)], [(K // 2, K), (0, K // 2)], [(0, 97), (97, K)]):
        got, n = _project(forced, x, r, k, parts=parts)
        assert n == len(parts), parts
        assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), parts


# ---- the combine on tail shapes away from Gamma ------------------------------------------------------------------
def test_combine_on_tails(forced):
    """A segment away from Gamma x odd rows and 64-row-stage row tails x a 17-frame block"""
    x = _data(17, N_ATOMS, 30)
    for K in (3, 65, 257):
        t0 = time.perf_counter()
        k, r, interval = geometry("seg_1", K)
        _plan(k, r, interval=interval)
        got, n = _project(forced, x, r, k)
        _check(f"seg_1, K={K}, T=17", got, _refs(x, r, k), n, t0=t0)
