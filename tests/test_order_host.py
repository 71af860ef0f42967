"""The bond-order route on the host: the spherical-harmonic reference of tests/order64.py against the addition theorem and
against the known shells; the NumPy twin of the arithmetic stated at psa_bond_order inside the allowance of
tests/order_cases.py on every family, and each planted fault outside it on a named one -- so the allowance is tight enough
to see them; the integer bin rule against exact integers at every edge; the result type; the calculator's refusals and its
empty result; the ABI table, the header and the constants."""
import functools
import logging
import re
from pathlib import Path

import numpy as np
import pytest

import angle_cases as Q
import order64 as O
import order_cases as C

ROOT = Path(__file__).resolve().parents[1]
LS = (4, 6)


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_harmonics_equal_the_addition_theorem():
    rng = np.random.default_rng(2)
    ls = list(range(1, 13))
    for n in (1, 2, 3, 7, 12, 14, 33, 64):
        legs = rng.standard_normal((n, 3)) * rng.uniform(0.5, 3.0, (n, 1))
        assert np.abs(O.q_squared(legs, ls) - O.theorem(legs, ls)).max() <= 1e-12, n
    assert np.allclose(O.q_squared(rng.standard_normal((1, 3)), ls), 1.0, atol=1e-12)   # one leg: q_l = 1


KNOWN = {"fcc": (12, {3: 0.0, 4: 0.19094, 6: 0.57452, 8: 0.40391}), "hcp": (12, {4: 0.09722, 6: 0.48476}),
         "bcc": (8, {4: 0.50918, 6: 0.62854}), "sc": (6, {4: 0.76376, 6: 0.35355}),
         "tetrahedron": (4, {3: 0.74536, 4: 0.50918, 6: 0.62854}), "icosahedron": (12, {4: 0.0, 6: 0.66332, 12: 0.58542})}


@pytest.mark.parametrize("name", KNOWN)
def test_known_shells(name):
    n, want = KNOWN[name]
    legs = C.shell(name)
    assert legs.shape == (n, 3)
    turn = np.linalg.qr(np.random.default_rng(4).standard_normal((3, 3)))[0]    # any frame
    for shell in (legs, 2.5 * legs @ turn):
        q = np.sqrt(np.maximum(O.q_squared(shell, list(want)), 0.0))
        assert np.abs(q - np.array(list(want.values()))).max() <= 1e-5, (name, q)


# ---- the twin and the allowance ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name, kind="one", ls=LS):
    pos, box, rc = C.family(name)
    n = pos.shape[1]
    groups = [np.arange(n)] if kind == "one" else Q.two_species(n)
    r_cut = rc if kind == "one" else Q.matrix_cutoff(rc, 2)
    return pos, box, groups, r_cut, C.reference(pos, box, groups, r_cut, 1, list(ls))


@functools.lru_cache(maxsize=None)
def _ball():
    pos = Q.ball(66, 1, 6.0, n_outside=3)
    groups = [np.arange(69)]
    return pos, Q.CUBIC, groups, 6.0, C.reference(pos, Q.CUBIC, groups, 6.0, 1, list(LS))


def _inside(case, ls=LS, n_q=200, fault=None, what=""):
    pos, box, groups, r_cut, ref = case
    assert C.excluded_share(ref) <= C.EXCLUDED_CAP, what                  # the excluded share, before anything else
    got = C.model(pos, box, groups, r_cut, 1, list(ls), n_q, fault)
    return got, C.check(got[4], got[5], ref, what)


@pytest.mark.parametrize("name", C.FAMILIES)
def test_twin_inside_the_allowance(name):
    case = _case(name)
    assert not case[4]["excluded"].any()                                    # one species: no leg-borderline neighbour at all
    got, ok = _inside(case, what=name)
    assert ok
    hist, trunc, iso, undef, x, n = got
    sizes = [len(g) for g in case[2]]
    want, out = C.histogram_of(x, n, sizes, 200)
    assert np.array_equal(hist, want) and np.array_equal(trunc + iso + undef, out)
    assert np.all(hist.sum(axis=2) + (trunc + iso + undef)[:, None] == case[0].shape[0] * np.array(sizes)[:, None])


def test_twin_every_order_and_two_species():
    ls = (1, 2, 3, 5, 7, 8, 10, 12)
    case = _case("cubic37", "two", ls)
    assert _inside(case, ls, what="cubic37 two species, eight orders")[1]
    ref = case[4]
    assert np.allclose(ref["xq"][ref["why"] == 0][:, 0] >= 0, True) and (ref["why"] == 0).sum() > 1000


# the family each fault is held against
FAULT_FAMILY = {"no_n_term": "cubic130", "pairs_once": "triclinic130", "divide_by_n": "cubic37", "l_off_by_one": "triclinic257",
                "theta_not_cos": "cubic130", "first_64": "ball", "float_root_bin": "edges"}


@pytest.mark.parametrize("fault", [f for f in C.FAULTS if f != "float_root_bin"])
def test_planted_faults_leave_the_allowance(fault):
    name = FAULT_FAMILY[fault]
    case = _ball() if name == "ball" else _case(name)
    assert _inside(case, what=f"{name} clean")[1]
    assert not _inside(case, fault=fault, what=f"{name} {fault}")[1]


def test_twin_capacity():
    """66 atoms in a ball: 65 neighbours each, all truncated; the three outside see each other"""
    case = _ball()
    (hist, trunc, iso, undef, x, n), ok = _inside(case, what="ball")
    assert ok and trunc[0] == 66 and iso[0] == 0 and undef[0] == 0 and hist.sum() == 2 * 3
    assert np.all(n[0, :66] == 65) and np.all(x[0, :66] == -1) and np.all(n[0, 66:] == 2) and np.all(x[0, 66:] >= 0)


def test_faults_are_the_issue_s_list():
    assert set(FAULT_FAMILY) == set(C.FAULTS) and len(C.FAULTS) == 7


# ---- the bins ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 7, 200, 1024])
def test_integer_bins_at_every_edge(n_q):
    """the stated bisection against exact Python integers around every edge, X = 0, X = n^2 2^24 and the i^2 boundaries that
    are hit exactly among them; the float32 root is not that rule"""
    x, n = C.edge_samples(n_q)
    exact = np.array([C.exact_bin(a, b, n_q) for a, b in zip(x, n)])
    assert np.array_equal(C.bins_model(x, n, n_q), exact)
    full = n * n * C.ONE
    assert np.all(exact[x == 0] == 0) and np.all(exact[x == full] == n_q - 1) and exact.max() == n_q - 1
    hit = (x * n_q * n_q) % full == 0                                       # i^2 n^2 2^24 = X n_q^2 exactly: X opens bin i
    root = np.array([int(round((int(a) * n_q * n_q // int(f)) ** 0.5)) for a, f in zip(x[hit], full[hit])])
    assert hit.sum() >= 6 and np.array_equal(exact[hit], np.minimum(root, n_q - 1))
    # every bin is an interval [i, i + 1) / n_q of q: i^2 <= q^2 n_q^2 < (i + 1)^2, the last closed at q = 1
    lhs = x * n_q * n_q
    assert np.all(exact * exact * full <= lhs) and np.all(((exact + 1) ** 2 * full > lhs) | (exact == n_q - 1))
    if n_q == 1024:
        assert not np.array_equal(C.bins_model(x, n, n_q, "float_root_bin"), exact)


# ---- the result type ------------------------------------------------------------------------------------------------------
def test_result_type():
    import psa_amd
    from psa_amd import BondOrder, order
    assert "BondOrder" in psa_amd.__all__
    pos, box, groups, r_cut, _ = _case("cubic37", "two", LS)
    hist, trunc, iso, undef, x, n = C.model(pos, box, groups, r_cut, 1, list(LS), 50)
    res = order.result(hist.astype(np.uint64), trunc.astype(np.uint64), iso.astype(np.uint64), undef.astype(np.uint64), x, n, LS, 50,
                       pos.shape[0], groups)
    assert isinstance(res, BondOrder) and res.counts.shape == (2, 2, 50) and np.array_equal(res.ls, [4, 6])
    assert res.order(4) == 0 and res.order(6) == 1
    with pytest.raises(ValueError, match="order 5"):
        res.order(5)
    assert res.q_edges[0] == 0.0 and res.q_edges[-1] == 1.0 and np.allclose(res.q, 0.01 + 0.02 * np.arange(50))
    assert res.origins == pos.shape[0] and np.array_equal(res.samples, [pos.shape[0] * len(g) for g in groups])
    dens = res.density
    assert np.allclose((dens * 0.02).sum(axis=2), 1.0)
    assert np.array_equal(res.atoms, np.concatenate(groups)) and np.array_equal(res.neighbours, n)
    kept = x[..., 0] >= 0
    assert res.q_atoms.shape == x.shape and np.array_equal(np.isnan(res.q_atoms[..., 0]), ~kept)
    want = np.sqrt(x[kept] / (n[kept][:, None].astype(np.float64) ** 2 * 2.0 ** 24))
    assert np.array_equal(res.q_atoms[kept], want) and np.all((want >= 0.0) & (want <= 1.0))
    cut = len(groups[0])
    for a, cols in enumerate((slice(0, cut), slice(cut, None))):
        part = res.q_atoms[:, cols].reshape(-1, 2)
        assert np.allclose(res.mean[a], part[~np.isnan(part[:, 0])].mean(axis=0))
    # the bin of q_atoms is the bin counted (away from the edges, where the root may round across)
    bins = np.minimum((res.q_atoms[kept] * 50).astype(np.int64), 49)
    counted = np.array([[C.exact_bin(v, m, 50) for v in row] for row, m in zip(x[kept], n[kept])])
    assert (bins == counted).mean() > 0.999
    bare = order.result(hist, trunc, iso, undef, None, None, LS, 50, pos.shape[0], groups)
    assert bare.q_atoms is None and bare.neighbours is None and bare.atoms is None and bare.mean is None


def _calculator(pos, box, types=None):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, 1, 1, 1)


def test_calculator_refusals_and_the_empty_result(caplog):
    from psa_amd import BondOrder, max_pair_radius
    pos = C.family("cubic37")[0]
    calc = _calculator(pos, Q.CUBIC, (np.arange(37) % 2 + 1).astype(np.int32))
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="n_q"):
            calc.calculate_bond_order(3.0, n_q=bad)
    for bad in ((), (0,), (13,), (4, 4), (6, 4), (4.0, 6.0), tuple(range(1, 10)), [[4, 6]]):
        with pytest.raises(ValueError, match="ls must be"):
            calc.calculate_bond_order(3.0, ls=bad)
    with pytest.raises(TypeError, match="per_atom"):
        calc.calculate_bond_order(3.0, per_atom=1)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, 2.0]):
        with pytest.raises(ValueError, match="r_cut"):
            calc.calculate_bond_order(bad)
    with pytest.raises(ValueError, match="served radius"):
        calc.calculate_bond_order(max_pair_radius(Q.CUBIC) * 1.001)
    with pytest.raises(ValueError, match="symmetric"):
        calc.calculate_bond_order([[3.0, 2.0], [2.5, 3.0]], basis_atom_types=[1, 2])
    with pytest.raises(ValueError, match="origin_step"):
        calc.calculate_bond_order(3.0, origin_step=0)
    with pytest.raises(ValueError, match="disjoint"):
        calc.calculate_bond_order(3.0, basis_atom_indices=[[0, 1], [1, 2]])
    empty = _calculator(pos[:0], Q.CUBIC)
    with caplog.at_level(logging.WARNING):
        res = empty.calculate_bond_order(3.0, (4, 6, 8), 30, per_atom=True)
    assert "0 frames or 0 atoms" in caplog.text
    assert isinstance(res, BondOrder) and res.counts.shape == (1, 3, 30) and not res.counts.any() and res.origins == 0
    assert not res.density.any() and res.q_atoms is None and res.mean is None


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_abi_table_header_and_constants():
    from psa_amd import _hip
    head = (ROOT / "include" / "psa_hip.h").read_text()
    assert re.search(r"\bint psa_bond_order\(", head) and len(_hip.SIGNATURES["psa_bond_order"][1]) == 18
    for stated in ("__fmaf_rn(A_k, __fmul_rn(cos, P_k), -__fmul_rn(B_k, P_{k-1}))", "__float2ll_rn(__fmul_rn(P_l, 2^24))",
                   "i^2 n^2 2^24 <= X_l n_q^2", "truncated[alpha]", "isolated[alpha]", "undefined[alpha]"):
        assert stated in head, stated
    lib = _hip.load_library()
    assert lib.psa_abi_version() == _hip.ABI_VERSION == 6 and lib.psa_bond_order
    assert hasattr(_hip.Engine, "bond_order")
    ctx = (ROOT / "psa_amd" / "csrc" / "psa_ctx.h").read_text()
    for name in ("ORDER_MAX_L", "ORDER_MAX_LS", "ORDER_MAX_BINS", "ORDER_SHIFT"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", ctx).group(1)) == getattr(_hip, name)
    assert (_hip.ORDER_MAX_L, _hip.ORDER_MAX_LS, _hip.ORDER_MAX_BINS, _hip.ORDER_SHIFT) == (12, 8, 1024, 24)
    assert C.MAX_L == _hip.ORDER_MAX_L and C.SHIFT == _hip.ORDER_SHIFT and C.CAPACITY == _hip.ANGLE_MAX_NEIGHBOURS


def test_refusals_that_need_no_device():
    """a null context is refused before anything is touched"""
    from psa_amd import _hip
    lib = _hip.load_library()
    assert lib.psa_bond_order(None, None, None, None, None, 1, None, 1, None, 0, 0, None, 0, None, None, None, None, None) != 0
    assert lib.psa_last_error()
