"""The 48-node folded low-rank route (psa_set_k1_lowrank_nodes) on the CPU.
  plan    psa_lowrank_plan_nodes(48): kappa, L, phi and C are a function of k_j, the node interval and the group alone (whole
          list and sub-lists agree bit for bit); Lebesgue constant <= 3.5; r_bound <= 1e-6 on every geometry of
          tests/lowrank_cases.py; with 64 nodes the entry reports psa_lowrank_plan's arrays, bit for bit.
  model   the NumPy model of tests/lowrank_n48_cases.py against the float64 reference under the bound derived there, on
          every input family, the other side of Gamma, a node interval away from it and 27 to 2587 atoms.
  faults  the image built without W_lo's share, D' of one row tile zeroed, and the image built from the 64-node plan
          against 48-node node rows each lie at least 5 x over the bound.
  residual  the interpolation residual alone, at its worst: 601 k from edge to edge of a node interval (the residual with the
          float32 rounding of L and phi peaks at 4.8e-7, inside it; 3.6e-7 at the edges), all atoms at the extremes of x,
          equal-sign data.  Dropping it from the image moves the result by 9.7 u B at most (r_bound is 8.1 u), which does NOT
          cross the by-difference bound (two images of |D'| <= 1e-3 rounded to float16: 33.9 u B): no input this test
          could construct tells the residual from the float16 rounding of the image that carries it.

Every figure here comes from the NumPy model on the CPU; none from a kernel."""
import numpy as np
import pytest

import lowrank_env_cases as E
import lowrank_n48_cases as N
from lowrank_cases import DIRECTIONS, LIMITS, geometry

U = E.U


# ---- the plan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain_100", "neg_-1-10", "seg_1"])
def test_sub_lists_get_the_same_plan(name):
    from psa_amd import _hip
    k, r, interval = geometry(name, 256)
    whole = _hip.lowrank_plan_nodes(k, r, None, 48)
    assert whole is not None and whole["interval"] == interval and whole["nodes"] == 48
    for lo, hi in [(0, 128), (128, 256), (0, 96), (96, 256), (37, 219)]:
        p = _hip.lowrank_plan_nodes(k[lo:hi], r, None, 48)
        assert p is not None
        for key in ("u", "k0", "kappa"):
            assert np.array_equal(p[key], whole[key]), key
        for key in ("x_c", "h_x", "width", "interval"):
            assert p[key] == whole[key], key
        for key in ("C", "L", "phi"):
            assert np.array_equal(p[key].view(np.uint32), whole[key][lo:hi].view(np.uint32)), key
        assert p["r_bound"] <= whole["r_bound"]


@pytest.mark.parametrize("name", DIRECTIONS + LIMITS + ["plain_100"])
def test_geometries_lebesgue_and_r_bound(name):
    from psa_amd import _hip
    k, r, interval = geometry(name)
    p = _hip.lowrank_plan_nodes(k, r, None, 48)
    assert p is not None and p["interval"] == interval
    N.plan_caps_n48(p)
    lam = float(np.abs(p["L"].astype(np.float64)).sum(axis=1).max())
    print(f"{name}: Lebesgue {lam:.3f}, r_bound {p['r_bound']:.2e}, d_bound {p['d_bound']:.2e}, e_bound {p['e_bound']:.2e}")
    assert lam <= 3.5 and 0 < p["r_bound"] <= 1e-6
    # C is the product of its factors, rounded once
    want = (p["phi"].astype(np.complex128)[:, None] * p["L"].astype(np.float64))
    assert np.max(np.abs(p["C"] - want)) <= 4 * U * 3.5
    # the nodes: 48 Chebyshev points of the first kind of the interval
    mid, half = (p["interval"] + 0.5) * p["width"], 0.5 * p["width"]
    assert np.allclose(p["kappa"], mid + half * np.cos(np.pi * (2 * np.arange(48) + 1) / 96.0), rtol=0, atol=1e-12 * abs(mid + half))


def test_r_bound_is_the_residual_of_the_tables():
    """r_bound against NumPy: max |P_line - phi L W| over rows and atoms, W in float64, L and phi the float32 tables"""
    c = N.case("quiet_frames", K=40, n=257)
    p = c["plan"]
    got = p["phi"].astype(np.complex128)[:, None] * (p["L"].astype(np.float64) @ E.node_table64(c, p))
    want = float(np.max(np.abs(got - E.line_phases64(c, p))))
    assert abs(p["r_bound"] - want) <= 1e-9 * want + 1e-15, (p["r_bound"], want)


def test_64_nodes_report_the_64_node_plan():
    from psa_amd import _hip
    for name in ("plain_100", "neg_-1-10", "seg_1"):
        k, r, _ = geometry(name, 100)
        a, b = _hip.lowrank_plan(k, r), _hip.lowrank_plan_nodes(k, r, None, 64)
        for key in ("u", "k0", "kappa", "C", "L", "phi"):
            assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
        for key in ("x_c", "h_x", "width", "interval", "d_bound", "dscale", "e_bound", "dscale_fold"):
            assert a[key] == b[key], key
        assert b["r_bound"] == 0.0


# ---- the model under the bound ------------------------------------------------------------------------------------------
def _under(c, tag):
    R = E.reference(c)
    b = N.bound_abs_n48(c, R)
    got = N.model_n48(c)
    e = E.excess(got, R["ref"], b)[0]
    print(f"{tag}: 48-node model {e:.3f} x the 48-node bound")
    assert e <= 1
    return got


@pytest.mark.parametrize("family", E.FAMILIES)
def test_families(family):
    got = _under(N.case(family), family)
    if family == "zeros":
        assert not got.any()


@pytest.mark.parametrize("geom", ["neg_-1-10", "seg_1"])
def test_other_side_and_other_interval(geom):
    c = N.case("quiet_frames", geom=geom)
    assert c["plan"]["interval"] == (-1 if geom.startswith("neg") else 1)
    _under(c, geom)


@pytest.mark.parametrize("n", [27, 91, 1275, 2587])
def test_atoms(n):
    _under(N.case("quiet_frames", n=n), f"n_g={n}")


# ---- discriminating power -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [27, 91, 257])
def test_planted_faults(n):
    c = N.case("quiet_frames", n=n)
    R = E.reference(c)
    b = N.bound_abs_n48(c, R)
    faults = {"the image without W_lo's share": dict(no_lo=True), "D' of one 16-row tile zeroed": dict(tile=1),
              "the image from the 64-node plan": dict(l64=True)}
    for name, lose in faults.items():
        with np.errstate(invalid="ignore", over="ignore"):
            bad = N.model_n48(c, lose)
        if not np.all(np.isfinite(bad)):
            print(f"    {name}: the image overflows float16, the result is not finite")
            continue
        e = E.excess(bad, R["ref"], b)[0]
        print(f"    n_g={n}, {name}: {e:.1f} x the bound")
        assert e >= 5, name


# ---- the residual alone -------------------------------------------------------------------------------------------------
def test_residual_at_its_worst_by_difference():
    from psa_amd import _hip
    n, T = 64, 16
    c = dict(N.case("quiet_frames", K=2, n=n, T=T))
    rng = np.random.default_rng(5)
    r = c["r"].copy()
    r[:, 0] = 20.0                                            # every atom at one extreme of x ...
    r[0, 0] = -20.0                                           # ... but the one that fixes the range: h_x = 20, width = 3
    c["r"] = r
    c["k"] = np.zeros((601, 3), np.float32)                   # node interval 0 from edge to edge: the worst row is among them
    c["k"][:, 0] = np.linspace(0.0, 3.0 - 2.0 ** -20, 601)
    c["data"] = (1.0 + 0.25 * rng.random((T, n, 3))).astype(np.float32)   # equal signs: the residuals of all atoms add up
    c["plan64"] = _hip.lowrank_plan(c["k"], c["r"], c["idx"])
    c["plan"] = N.plan48(c)
    p = c["plan"]
    assert p["interval"] == 0 and p["width"] == 3.0 and 4e-7 <= p["r_bound"] <= 1e-6, (p["width"], p["r_bound"])
    R = E.reference(c)
    kept, dropped = N.model_n48(c), N.model_n48(c, dict(no_residual=True))
    assert E.excess(kept, R["ref"], N.bound_abs_n48(c, R))[0] <= 1
    B = R["B"][None, :, :]
    moved = np.maximum(np.abs((dropped - kept).real), np.abs((dropped - kept).imag)) / B
    tot = p["d_bound"] + p["e_bound"] + p["r_bound"]
    by_diff = 2 * E.d_terms(n, tot) + 2 * U
    crosses = bool(moved.max() > by_diff)
    print(f"residual dropped: the result moves by {moved.max() / U:.2f} u B at most (r_bound {p['r_bound'] / U:.2f} u); the "
          f"by-difference bound is {by_diff / U:.2f} u B: {'crossed' if crosses else 'not crossed'}")
    assert moved.max() >= 0.5 * p["r_bound"], "the construction does not add the residuals up"
    assert not crosses, "the residual alone is now visible by difference: say so in the module docstring"
