"""The folded low-rank route (psa_set_k1_lowrank_fold) on the CPU: the NumPy model of tests/lowrank_fold_cases.py against the
float64 reference, under the route's existing per-element bound (lowrank_env_cases.bound_abs) and under the folded bound
derived there, on every input family, the other side of Gamma, a node interval away from it and 27 to 2587 atoms; the D
pass by difference under the existing bound_diff_abs; three planted faults; the plan's e_bound and dscale_fold.

Every figure here comes from the NumPy model on the CPU; none from a kernel."""
import numpy as np
import pytest

import lowrank_env_cases as E
import lowrank_fold_cases as F
from ref64 import project64, scale_B

U = E.U


def _under_both(c, tag):
    R = E.reference(c)
    old, new = E.bound_abs(c, R), F.bound_abs_fold(c, R)
    assert np.all(new >= old)
    got = F.model_fold(c)
    e_old, e_new = E.excess(got, R["ref"], old)[0], E.excess(got, R["ref"], new)[0]
    e_today = E.excess(E.model_lowrank(c), R["ref"], old)[0]
    print(f"{tag}: folded model {e_old:.3f} x the existing bound, {e_new:.3f} x the folded bound; today's model {e_today:.3f} x")
    assert e_old <= 1 and e_new <= 1
    return got


@pytest.mark.parametrize("family", E.FAMILIES)
def test_families(family):
    c = E.case(family)
    got = _under_both(c, family)
    if family == "zeros":
        assert not got.any()


@pytest.mark.parametrize("geom", ["neg_-1-10", "seg_1"])
def test_other_side_and_other_interval(geom):
    c = E.case("quiet_frames", geom=geom)
    assert c["plan"]["interval"] == (-1 if geom.startswith("neg") else 1)
    _under_both(c, geom)


@pytest.mark.parametrize("n", [27, 91, 1275, 2587])
def test_atoms(n):
    _under_both(E.case("quiet_frames", n=n), f"n_g={n}")


def _diff_setup(n):
    line, off = E.line_and_scattered(n=n)
    for name in ("L", "phi", "kappa"):
        assert np.array_equal(line["plan"][name].view(np.uint8), off["plan"][name].view(np.uint8)), name
    B = scale_B(line["data"], line["r"])
    ref = project64(off["data"], off["r"], off["k"]) - project64(line["data"], line["r"], line["k"])
    return line, off, B, ref, E.bound_diff_abs(line, off, B)


@pytest.mark.parametrize("n", [27, 91, 257])
def test_d_pass_by_difference_and_planted_faults(n):
    """got(scattered) - got(line): equal node rows and combine, and the same E in both images, so what is left is the two
    roundings of D + E and the D terms.  Each fault is planted in the scattered run alone and must lie at least 5 x over
    the by-difference bound or over the whole route's bound (a fault that makes the image overflow float16 counts as seen)"""
    line, off, B, ref, babs = _diff_setup(n)
    base = F.model_fold(line)
    e_good = E.excess(F.model_fold(off) - base, ref, babs)[0]
    print(f"n_g={n}: e_bound {off['plan']['e_bound']:.2e}, by difference {e_good:.3f} x bound_diff_abs "
          f"({float(babs.max() / B.max()) / U:.2f} u)")
    assert e_good <= 1
    R = E.reference(off)
    whole = E.bound_abs(off, R)
    faults = {"E lost from the image": dict(e_lost=True), "E built from the hi piece": dict(e_from_hi=True),
              "E of one 16-row tile lost": dict(e_tile=1)}
    for name, lose in faults.items():
        with np.errstate(invalid="ignore", over="ignore"):
            bad = F.model_fold(off, lose=lose)
        if not np.all(np.isfinite(bad)):
            print(f"    {name}: the image overflows float16, the result is not finite")
            continue
        e_diff, e_whole = E.excess(bad - base, ref, babs)[0], E.excess(bad, R["ref"], whole)[0]
        print(f"    {name}: {e_diff:.1f} x the by-difference bound, {e_whole:.1f} x the whole bound")
        assert max(e_diff, e_whole) >= 5, name


def test_plan_reports_e_bound_and_dscale_fold():
    for geom in ("plain_100", "neg_-1-10", "seg_1"):
        for K in (2, 40, 257):
            p = E.case("zeros", K=K, geom=geom)["plan"]
            F.plan_caps_fold(p)
            assert p["e_bound"] <= 2.0 ** 0.5 * E.LEBESGUE * 2.0 ** -12
            assert p["dscale_fold"] <= p["dscale"]
            print(f"{geom} K={K}: d_bound {p['d_bound']:.2e}, e_bound {p['e_bound']:.2e}, dscale 2^{int(np.log2(p['dscale']))}, "
                  f"dscale_fold 2^{int(np.log2(p['dscale_fold']))}")


def test_folded_bound_is_the_documented_one():
    u, d10 = 2.0 ** -24, 2.0 ** -10 * (1 + 2.0 ** -14)
    assert F.fold_terms(257, 2.0 ** -13, 2.0 ** -10) == (d10 + 9 * u) * (2.0 ** -13 + 2.0 ** -10) + 2 * u + 68 * u * 2.0 ** -10
    assert F.E_MAX == pytest.approx(1.2595e-3, rel=1e-3)
    # at the caps the folded D term is 2^-10 e_bound = 20.6 u and a little more than today's, of a whole of up to 336 u
    assert 20.5 * u < F.fold_terms(257, E.D_MAX, F.E_MAX) - E.d_terms(257, E.D_MAX) < 21 * u
