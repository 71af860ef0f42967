"""The local-order route on the host: the 3j table against its sum rule, the closed form of (l l l; 0 0 0), sympy and the
quadrature of tests/qlm64.py; the spherical-angle reference against tests/order64.py, the known shells and a perfect lattice;
the NumPy twin of the arithmetic stated at psa_local_order inside the allowances of tests/qlm_cases.py on every family, and each
planted fault outside them on a named one; both bin rules against exact arithmetic at their edges; the result type; the
calculator's refusals and its empty result; the ABI table, the header and the constants."""
import functools
import logging
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import angle_cases as Q
import order64 as O
import qlm64 as L
import qlm_cases as C

ROOT = Path(__file__).resolve().parents[1]
LS = (4, 6)
EVEN = (2, 4, 6, 8, 10, 12)


# ---- the 3j table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", EVEN)
def test_3j_table_sum_rule_closed_form_and_quadrature(l):
    from psa_amd import wigner_3j_table
    t = wigner_3j_table(l)
    assert t.shape == (2 * l + 1, 2 * l + 1) and abs((t * t).sum() - 1.0) <= 1e-14
    assert abs(t[l, l] - L.three_j_zero(l)) <= 1e-15
    assert np.abs(t - L.three_j(l)).max() <= 1e-12                          # the integral of three harmonics
    m = np.arange(-l, l + 1)
    assert not t[np.abs(m[:, None] + m[None, :]) > l].any() and np.array_equal(t, t.T)


def test_3j_table_against_sympy():
    sympy_wigner = pytest.importorskip("sympy.physics.wigner")
    from psa_amd import wigner_3j_table
    for l in EVEN:
        t = wigner_3j_table(l)
        for m1 in range(-l, l + 1):
            for m2 in range(max(-l, -l - m1), min(l, l - m1) + 1):
                assert abs(t[m1 + l, m2 + l] - float(sympy_wigner.wigner_3j(l, l, l, m1, m2, -m1 - m2))) <= 1e-15, (l, m1, m2)


def test_3j_of_an_odd_order_makes_w_vanish():
    from psa_amd import wigner_3j_table
    t = wigner_3j_table(3)
    assert np.abs(t + t.T).max() <= 1e-15 and t[3, 3] == 0.0                # antisymmetric under a column exchange


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_reference_moduli_equal_order64():
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 12, 33, 64):
        legs = rng.standard_normal((n, 3)) * rng.uniform(0.5, 3.0, (n, 1))
        for l in EVEN:
            q2 = (np.abs(L.harmonics(legs, l).mean(axis=0)) ** 2).sum()
            assert abs(q2 - O.q_squared(legs, [l])[0]) <= 1e-12, (n, l)


def test_reference_is_rotation_invariant_and_pole_safe():
    rng = np.random.default_rng(5)
    legs = rng.standard_normal((9, 3))
    turn = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    turn *= np.sign(np.linalg.det(turn))
    for l in EVEN:
        assert abs(L.w_hat(legs, l) - L.w_hat(legs @ turn.T, l)) <= 1e-11
    near = np.array([[1e-7, 0.0, 1.0], [0.0, -1e-7, -1.0], [1.0, 0.0, 0.0]])
    assert np.abs(L.harmonics(near, 12)[:2, 12 + 1]) == pytest.approx(np.sqrt(12 * 13 / 4.0) * 1e-7, rel=1e-6)


# shell: (w_4, w_6); None: undefined (q_4 = 0)
KNOWN = {"fcc": (-0.159317, -0.013161), "hcp": (+0.134097, -0.012442), "bcc": (-0.159317, +0.013161), "sc": (+0.159317, +0.013161),
         "icosahedron": (None, -0.169754)}


@pytest.mark.parametrize("name", KNOWN)
def test_known_shells(name):
    legs = C.shell(name)
    turn = np.linalg.qr(np.random.default_rng(4).standard_normal((3, 3)))[0]
    turn *= np.sign(np.linalg.det(turn))
    for shell in (legs, 2.5 * legs @ turn.T):
        for l, want in zip((4, 6), KNOWN[name]):
            if want is None:
                assert (np.abs(L.harmonics(shell, l).sum(axis=0)) ** 2).sum() <= 1e-20
            else:
                assert abs(L.w_hat(shell, l) - want) <= 2e-6, (name, l, L.w_hat(shell, l))


@functools.lru_cache(maxsize=None)
def _lattice(name):
    pos, box, rc = {"fcc": lambda: (C.fcc_block(1), Q.CUBIC, 4.5), "bcc": lambda: (C.bcc_block(1), Q.CUBIC, 5.0),
                    "hcp": lambda: C.hcp_block(1) + (3.5,)}[name]()
    groups = [np.arange(pos.shape[1])]
    return pos, box, groups, rc, C.reference(pos, box, groups, rc, 1, list(LS), 6, 0.7)


@pytest.mark.parametrize("name,n", [("fcc", 12), ("bcc", 8), ("hcp", 12)])
def test_perfect_lattice_in_the_reference(name, n):
    """every atom has the same shell, so q-bar = q, w-bar = w and every bond is solid-like: xi = n"""
    pos, box, groups, rc, ref = _lattice(name)
    assert np.all(ref["n"] == n) and not ref["why"].any() and np.all(ref["xi"] == n) and not ref["xi_loose"].any()
    for j, l in enumerate(LS):
        assert np.abs(ref["vbar"][j] * n - ref["v"][j]).max() <= 1e-5       # (float32 positions: the shells differ by 1e-6)
    if name != "bcc":
        assert abs(L.w_form(ref["v"][0][0, 0], 4) / np.linalg.norm(ref["v"][0][0, 0]) ** 3 - KNOWN[name][0]) <= 1e-4


# ---- the twin and the allowance ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name, kind="one", ls=LS, threshold=0.7):
    pos, box, rc = C.family(name)
    n = pos.shape[1]
    groups = [np.arange(n)] if kind == "one" else Q.two_species(n)
    r_cut = rc if kind == "one" else Q.matrix_cutoff(rc, 2)
    return pos, box, groups, r_cut, C.reference(pos, box, groups, r_cut, 1, list(ls), ls[-1], threshold)


@functools.lru_cache(maxsize=None)
def _ball():
    pos = Q.ball(66, 1, 6.0, n_outside=3)
    groups = [np.arange(69)]
    return pos, Q.CUBIC, groups, 6.0, C.reference(pos, Q.CUBIC, groups, 6.0, 1, list(LS), 6, 0.7)


def _inside(case, ls=LS, fault=None, what=""):
    pos, box, groups, r_cut, ref = case
    assert C.excluded_share(ref) <= C.EXCLUDED_CAP and C.loose_share(ref) <= C.EXCLUDED_CAP, what      # before anything else
    got = C.model(pos, box, groups, r_cut, 1, list(ls), ref["solid_l"], ref["threshold"], fault)
    ok = all(C.check_q(got["q"][o], ref, o, f"{what} origin {o}") for o in (0, len(got["q"]) - 1))
    return got, C.check(got, ref, what) and ok


@pytest.mark.parametrize("name", C.FAMILIES)
def test_twin_inside_the_allowance(name):
    case = _case(name)
    got, ok = _inside(case, what=name)
    assert ok
    sizes, n_o = [len(g) for g in case[2]], case[0].shape[0]
    rows = C.rows_of(got, sizes, 2, 50, 40, 0.2)
    assert C.identities(rows, sizes, n_o, 2, 50, 40) and rows.sum() > 0


def test_twin_high_orders_and_two_species():
    ls = (6, 8, 10, 12)
    case = _case("cubic37", "two", ls)
    assert _inside(case, ls, what="cubic37 two species, four orders")[1]
    assert (case[4]["why"] == 0).sum() > 1000


# the family each fault is held against (the bond test without D > 0 needs anti-parallel vectors: a low threshold)
FAULT_FAMILY = {"centre_left_out": "cubic130", "divide_by_n": "triclinic130", "neighbour_not_normalised": "cubic37",
                "negative_m_dropped": "triclinic257", "no_sign_in_minus_m": "cubic130", "wrong_3j_m3": "triclinic130",
                "no_positive_d": "cubic37 low threshold", "first_64": "ball"}


@pytest.mark.parametrize("fault", C.FAULTS)
def test_planted_faults_leave_the_allowance(fault):
    name = FAULT_FAMILY[fault]
    case = _ball() if name == "ball" else _case("cubic37", threshold=0.2) if name.endswith("low threshold") else _case(name)
    assert _inside(case, what=f"{name} clean")[1]
    assert not _inside(case, fault=fault, what=f"{name} {fault}")[1]


def test_twin_capacity():
    """66 atoms in a ball: 65 neighbours each, all truncated; the three outside see each other"""
    got, ok = _inside(_ball(), what="ball")
    assert ok and np.all(got["n"][0, :66] == 65) and np.all(got["xi"][0, :66] == -1) and np.all(got["xi"][0, 66:] >= 0)
    assert np.all(got["q"][0][:66, 0, 1] == -1) and not got["q"][0][:66, 1:].any()


def test_faults_are_the_issue_s_list():
    assert set(FAULT_FAMILY) == set(C.FAULTS) and len(C.FAULTS) == 8


# ---- the bins ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 7, 200, 1024])
def test_q_bins_at_every_edge(n_q):
    """the stated bisection against exact rational arithmetic around every edge i^2 / n_q^2, at 0 and at 1"""
    edges = [Fraction(i * i, n_q * n_q) for i in range(n_q + 1)]
    values = sorted({float(np.nextafter(float(e), d)) for e in edges for d in (-1.0, 2.0)} | {float(e) for e in edges} | {0.0, 1.0})
    values = [v for v in values if 0.0 <= v <= 1.0]
    got = [C.q_bin(v, n_q) for v in values]
    assert got == [C.exact_q_bin(v, n_q) for v in values]
    assert got[0] == 0 and got[-1] == n_q - 1 and max(got) == n_q - 1 and sorted(got) == got


@pytest.mark.parametrize("n_w", [1, 7, 200, 1024])
def test_w_bins_at_every_edge(n_w):
    """the stated product against exact rational arithmetic of the same two roundings; -R opens bin 0, +R is outside"""
    R = 0.2
    c = np.float64(n_w) / (np.float64(2.0) * np.float64(R))
    values = [-R + 2.0 * R * i / n_w for i in range(n_w + 1)]
    values = sorted({float(np.nextafter(v, d)) for v in values for d in (-1.0, 1.0)} | set(values) | {0.0, -0.3, 0.3, float("nan")})
    for v in values:
        got = C.w_bin(v, n_w, R)
        if v != v:
            assert got == -1
            continue
        u = Fraction(float(np.float64(float(Fraction(v) + Fraction(R))) * c))   # both roundings, then exact
        want = int(u.numerator // u.denominator) if 0 <= u < n_w else -1
        assert got == want, v
    # (the sum w + R is rounded: the float64 just below R still gives 2 R, so the last bin is probed 2^-40 below R)
    assert C.w_bin(-R, n_w, R) == 0 and C.w_bin(R, n_w, R) == -1 and C.w_bin(R * (1.0 - 2.0 ** -40), n_w, R) == n_w - 1


# ---- the result type ------------------------------------------------------------------------------------------------------
def test_result_type_and_solid_fraction():
    import psa_amd
    from psa_amd import LocalOrder, local_order
    assert "LocalOrder" in psa_amd.__all__ and "wigner_3j_table" in psa_amd.__all__
    pos, box, groups, r_cut, ref = _case("cubic37", "two", LS)
    got = C.model(pos, box, groups, r_cut, 1, list(LS), 6, 0.7)
    sizes = [len(g) for g in groups]
    rows = C.rows_of(got, sizes, 2, 50, 40, 0.2).astype(np.uint64)
    res = local_order.result(rows, got["qbar2"], got["w"], got["wbar"], got["xi"].astype(np.int32), got["n"].astype(np.int32), LS, 50, 40, 0.2,
                             6, 0.7, pos.shape[0], groups)
    assert isinstance(res, LocalOrder) and res.qbar_counts.shape == (2, 2, 50) and res.w_counts.shape == res.wbar_counts.shape == (2, 2, 40)
    assert res.connections.shape == (2, 65) and res.w_outside.shape == res.wbar_undefined.shape == (2, 2) and res.truncated.shape == (2,)
    assert res.order(4) == 0 and res.order(6) == 1 and res.solid_l == 6 and res.solid_threshold == 0.7
    with pytest.raises(ValueError, match="order 5"):
        res.order(5)
    assert res.q_edges[0] == 0.0 and res.q_edges[-1] == 1.0 and res.w_edges[0] == -0.2 and res.w_edges[-1] == 0.2 and res.w.size == 40
    assert res.origins == pos.shape[0] and np.array_equal(res.samples, [pos.shape[0] * s for s in sizes])
    assert np.allclose((res.density * 0.02).sum(axis=2), 1.0)
    kept = got["xi"] >= 0
    assert np.array_equal(res.qbar_atoms[kept], np.sqrt(got["qbar2"][kept])) and np.all(np.isnan(res.qbar_atoms[~kept]))
    assert np.array_equal(res.atoms, np.concatenate(groups)) and np.array_equal(res.neighbours, got["n"])
    cut = sizes[0]
    for a, cols in enumerate((slice(0, cut), slice(cut, None))):
        part = res.qbar_atoms[:, cols].reshape(-1, 2)
        assert np.allclose(res.mean[a], part[~np.isnan(part[:, 0])].mean(axis=0))
        xi = got["xi"][:, cols]
        for k in (0, 1, 7):
            assert res.solid_fraction(k)[a] == pytest.approx((xi[xi >= 0] >= k).mean())
    with pytest.raises(ValueError, match="min_connections"):
        res.solid_fraction(65)
    bare = local_order.result(rows, None, None, None, None, None, LS, 50, 40, 0.2, 6, 0.7, pos.shape[0], groups)
    assert bare.qbar_atoms is None and bare.connections_atoms is None and bare.atoms is None and bare.mean is None
    with pytest.raises(ValueError, match="do not fit"):
        local_order.split_row(rows, 2, 50, 41)


def _calculator(pos, box, types=None):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, 1, 1, 1)


def test_calculator_refusals_and_the_empty_result(caplog):
    from psa_amd import LocalOrder, max_pair_radius
    pos = C.family("cubic37")[0]
    calc = _calculator(pos, Q.CUBIC, (np.arange(37) % 2 + 1).astype(np.int32))
    for name in ("n_q", "n_w"):
        for bad in (0, 1025, 2.5, True):
            with pytest.raises(ValueError, match=name):
                calc.calculate_local_order(3.0, **{name: bad})
    for bad in ((), (0,), (14,), (4, 4), (6, 4), (4.0, 6.0), (2, 4, 6, 8, 10), [[4, 6]]):
        with pytest.raises(ValueError, match="ls must be"):
            calc.calculate_local_order(3.0, ls=bad)
    for bad in ((3,), (4, 5), (5, 6)):
        with pytest.raises(ValueError, match="vanishes identically"):
            calc.calculate_local_order(3.0, ls=bad, solid_l=bad[-1])
    for bad in (8, 4.0, True):
        with pytest.raises(ValueError, match="solid_l"):
            calc.calculate_local_order(3.0, solid_l=bad)
    for bad in (0.0, 1.5, -0.7, float("nan")):
        with pytest.raises(ValueError, match="solid_threshold"):
            calc.calculate_local_order(3.0, solid_threshold=bad)
    for bad in (0.0, -0.2, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="w_range"):
            calc.calculate_local_order(3.0, w_range=bad)
    with pytest.raises(TypeError, match="per_atom"):
        calc.calculate_local_order(3.0, per_atom=1)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, 2.0]):
        with pytest.raises(ValueError, match="r_cut"):
            calc.calculate_local_order(bad)
    with pytest.raises(ValueError, match="served radius"):
        calc.calculate_local_order(max_pair_radius(Q.CUBIC) * 1.001)
    with pytest.raises(ValueError, match="symmetric"):
        calc.calculate_local_order([[3.0, 2.0], [2.5, 3.0]], basis_atom_types=[1, 2])
    with pytest.raises(ValueError, match="origin_step"):
        calc.calculate_local_order(3.0, origin_step=0)
    with pytest.raises(ValueError, match="disjoint"):
        calc.calculate_local_order(3.0, basis_atom_indices=[[0, 1], [1, 2]])
    empty = _calculator(pos[:0], Q.CUBIC)
    with caplog.at_level(logging.WARNING):
        res = empty.calculate_local_order(3.0, (4, 6, 8), 30, 20, per_atom=True)
    assert "0 frames or 0 atoms" in caplog.text
    assert isinstance(res, LocalOrder) and res.qbar_counts.shape == (1, 3, 30) and res.w_counts.shape == (1, 3, 20) and res.origins == 0
    assert not res.qbar_counts.any() and not res.connections.any() and not res.density.any() and res.qbar_atoms is None
    assert np.isnan(res.solid_fraction()[0])


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_abi_table_header_and_constants():
    from psa_amd import _hip
    head = (ROOT / "include" / "psa_hip.h").read_text()
    assert re.search(r"\bint psa_local_order\(", head) and len(_hip.SIGNATURES["psa_local_order"][1]) == 24
    assert re.search(r"\bint psa_debug_qlm\(", head) and len(_hip.SIGNATURES["psa_debug_qlm"][1]) == 11
    for stated in ("__double2ll_rn(Yt_lm(d_b / |d_b|) 2^40)", "Q_{l,-m} = (-1)^m conj Q_lm", "Condon-Shortley",
                   "(double)(i i) <= __dmul_rn(qbar2, (double)(n_q n_q))", "__dmul_rn(__dadd_rn(w, w_range), n_w / (2 w_range))",
                   "D > 0 and D D > thr^2 (A B)", "incomplete", "vanishes identically"):
        assert stated in head, stated
    assert "#define PSA_HIP_ABI_VERSION 6" in head
    lib = _hip.load_library()
    assert lib.psa_abi_version() == _hip.ABI_VERSION == 6 and lib.psa_local_order and lib.psa_debug_qlm
    assert hasattr(_hip.Engine, "local_order") and hasattr(_hip.Engine, "debug_qlm")
    ctx = (ROOT / "psa_amd" / "csrc" / "psa_ctx.h").read_text()
    for name in ("LOCAL_MAX_LS", "LOCAL_MAX_BINS", "LOCAL_SHIFT"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", ctx).group(1)) == getattr(_hip, name)
    assert (_hip.LOCAL_MAX_LS, _hip.LOCAL_MAX_BINS, _hip.LOCAL_SHIFT) == (4, 1024, 40) and C.SHIFT == _hip.LOCAL_SHIFT
    names, classes = [], []
    import ctypes as Ct
    for i in range(10 ** 4):
        name, cls = Ct.c_char_p(), Ct.c_int32()
        if lib.psa_debug_scratch_info(i, Ct.byref(name), Ct.byref(cls)) != 0:
            break
        names.append(name.value.decode()), classes.append(cls.value)
    at = names.index("d_local_tab")
    assert classes[at] == classes[names.index("d_angle_edges")] != classes[names.index("d_angle_work")]    # "real"


def test_refusals_that_need_no_device():
    """a null context is refused before anything is touched"""
    from psa_amd import _hip
    lib = _hip.load_library()
    assert lib.psa_local_order(None, None, None, None, None, 1, None, 1, None, 0, 0, 0, 0.2, 6, 0.7, None, 0, None, 0, None, None, None,
                               None, None) != 0
    assert lib.psa_last_error()
    assert lib.psa_debug_qlm(None, None, None, None, None, 1, None, 0, None, 0, None) != 0
