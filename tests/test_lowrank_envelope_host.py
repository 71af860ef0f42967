"""Proof, without a GPU, that the low-rank k-path route's per-element envelope (tests/test_gpu_lowrank_perelement.py) can
fail where the older low-rank tests cannot.

tests/lowrank_env_cases.py restates the route in NumPy with float64 accumulation (model_lowrank) and derives a bound for
every output element before the FFT.  For every input family that has quiet frames, at K = 40, n_g = 257, T = 96:
  * the correct model and the float32 oracle lie under the bound at every element;
  * the model that loses the second float16 piece of d on the quiet frames in the node rows lies at least 5 x over it
    (20 - 27 x as measured from this model on the CPU);
  * that same faulty output, after the FFT, is under TOL = 1e-6 in rel_max and TOL_ROW = 2e-6 in the worst k-row against
    its own maximum, the bars of tests/test_gpu_lowrank_envelope.py: the older tests would pass it.
The D pass is a few u of the ~100 u of the whole bound, and a D pass wrong on the quiet frames only is 2.7 x over the whole
bound at 257 atoms, less with more: not a margin to rely on.  It is held by difference: the same k-path with every vector on
the line and with a perpendicular scatter share the plan's L, phi and kappa bit for bit, so the two results differ by
their D terms alone.  On the quiet-frames input the model's difference lies under bound_diff, and D lost on the quiet frames, D of one 16-row tile lost and D applied to another component's hi piece
lie at least 5 x over it at 27, 91 and 257 atoms (12 - 81 x as measured from this model; at 1275 atoms the first two are about 5 x, 5.2 and 4.9: the D term adds up like
sqrt(n_g), B like n_g, so the GPU cases at 40 and 41 stages hold the bound and the smaller ones see the faults).

Every figure here comes from the NumPy model on the CPU; none from a kernel."""
import numpy as np
import pytest

import dense_cases as D
import lowrank_env_cases as E
from conftest import rel_max
from lowrank_cases import D_LIMIT
from ref64 import gamma, project64, row_rel, scale_B

TOL, TOL_ROW = 1e-6, 2e-6               # tests/test_gpu_lowrank_envelope.py, after the FFT
U = E.U


def _sed(q):
    """(T, K, 3): the SED of a projection (K, 3, T), as the older tests compare it"""
    return (np.fft.fft(q, axis=2) / q.shape[2]).transpose(2, 0, 1)


@pytest.mark.parametrize("family", E.QUIET_FAMILIES)
def test_lost_second_piece_is_seen_per_element_and_not_after_the_fft(family):
    c = E.case(family)
    R = E.reference(c)
    ref, babs = R["ref"], E.bound_abs(c, R)
    good, bad = E.model_lowrank(c), E.model_lowrank(c, lose=dict(x2=c["quiet"]))
    e_good, e_o32 = E.excess(good, ref, babs)[0], E.excess(D.oracle32(c), ref, babs)[0]
    e_bad, at = E.excess(bad, ref, babs)
    old, old_row = rel_max(_sed(bad), _sed(ref)), float(row_rel(_sed(bad), _sed(ref)).max())
    print(f"{family} K={len(c['k'])} n_g={c['n_g']} T={ref.shape[2]}: correct model {e_good:.3f} x bound, float32 oracle "
          f"{e_o32:.3f} x, second piece lost {e_bad:.1f} x at {at} (gamma {gamma(bad, ref, R['B']) / U:.0f} u); after the FFT "
          f"rel_max {old:.2e}, worst row {old_row:.2e}")
    assert e_good <= 1 and e_o32 <= 1
    assert e_bad >= 5
    assert old < TOL and old_row < TOL_ROW


@pytest.mark.parametrize("family", [f for f in E.FAMILIES if f not in E.QUIET_FAMILIES])
def test_model_and_oracle_are_under_the_bound(family):
    c = E.case(family)
    R = E.reference(c)
    babs = E.bound_abs(c, R)
    for name, got in (("model", E.model_lowrank(c)), ("oracle", D.oracle32(c))):
        e = E.excess(got, R["ref"], babs)[0]
        print(f"{family} {name}: {e:.3f} x bound")
        assert e <= 1
    if family == "zeros":
        assert not babs.any() and not E.model_lowrank(c).any()


@pytest.mark.parametrize("geom", ["neg_-1-10", "seg_1"])
def test_other_side_and_other_interval(geom):
    """phi != 1 (rot > 1) and a node interval away from Gamma: the model under the bound, the lost piece over it"""
    c = E.case("quiet_frames", geom=geom)
    p = c["plan"]
    assert p["interval"] == (-1 if geom.startswith("neg") else 1)
    R = E.reference(c)
    babs = E.bound_abs(c, R)
    e_good = E.excess(E.model_lowrank(c), R["ref"], babs)[0]
    e_bad = E.excess(E.model_lowrank(c, lose=dict(x2=c["quiet"])), R["ref"], babs)[0]
    print(f"{geom}: correct {e_good:.3f} x bound, second piece lost {e_bad:.1f} x")
    assert e_good <= 1 and e_bad >= 5


def test_interpolation_is_inside_its_share():
    for geom in ("plain_100", "neg_-1-10", "seg_1"):
        e = E.interpolation_error(E.case("zeros", geom=geom))
        print(f"{geom}: node sum against the line phase {e:.1e}")
        assert e <= E.INTERP


# ---- the D pass by difference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [27, 91, 257])
def test_d_pass_faults_are_seen_by_difference(n):
    line, off = E.line_and_scattered(n=n)
    pl, po = line["plan"], off["plan"]
    for name in ("L", "phi", "kappa"):
        assert np.array_equal(pl[name].view(np.uint8), po[name].view(np.uint8)), name
    assert pl["x_c"] == po["x_c"] and pl["interval"] == po["interval"]
    assert D_LIMIT[0] <= po["d_bound"] <= D_LIMIT[1], po["d_bound"]
    B = scale_B(line["data"], line["r"])
    ref = project64(off["data"], off["r"], off["k"]) - project64(line["data"], line["r"], line["k"])
    babs = E.bound_diff_abs(line, off, B)
    base = E.model_lowrank(line)
    e_good = E.excess(E.model_lowrank(off) - base, ref, babs)[0]
    faults = {"D lost on the quiet frames": dict(d_frames=line["quiet"]), "D of one 16-row tile lost": dict(d_tile=1),
              "D on another component": dict(d_comp=True)}
    print(f"n_g={n}: d_bound {po['d_bound']:.2e}, bound {float(babs.max() / B.max()) / U:.2f} u, correct {e_good:.3f} x")
    assert e_good <= 1
    for name, lose in faults.items():
        e = E.excess(E.model_lowrank(off, lose=lose) - base, ref, babs)[0]
        print(f"    {name}: {e:.1f} x bound")
        assert e >= 5, name
    # printed, not asserted: against the whole route's bound the quiet-frames fault is 2.7 x at 257 atoms, short of the
    # factor asked of a proof, which is why the D pass is held by difference
    R = E.reference(off)
    whole = E.excess(E.model_lowrank(off, lose=faults["D lost on the quiet frames"]), R["ref"], E.bound_abs(off, R))[0]
    print(f"    D lost on the quiet frames against the whole route's bound: {whole:.2f} x")


# ---- the formula, pinned ------------------------------------------------------------------------------------------------
def test_bounds_are_the_documented_ones():
    u = 2.0 ** -24
    d10 = 2.0 ** -10 * (1 + 2.0 ** -14)
    assert E.CHAIN == 68 and E.INTERP == 2.0 ** -40
    assert E.d_terms(257, 0.0) == 2 * u and E.d_terms(257, 2.0 ** -13) == (d10 + 9 * u) * 2.0 ** -13 + 2 * u
    # one node row taken as it is (lam = rot = 1), no node sum: the planes_lw bound, the combine on that error, D, final
    assert E.bound_units(257, 1.0, 1.0, 0.0, 0.0) == 16 * u + 68 * u * 16 * u + 2 * u + u + 2.0 ** -40
    assert E.bound_units(1000, 1.0, 1.0, 0.0, 0.0) == 18 * u + 68 * u * 18 * u + 3 * u + 2.0 ** -40
    # the shape of the whole: lam 3.61, a rotation of sqrt 2, the node sum at 0.64 B, D at its limit
    want = 2.0 ** 0.5 * 3.61 * 16 * u + 68 * u * (0.64 + 3.61 * 16 * u) + (d10 + 9 * u) * 2.0 ** -13 + 2 * u + u + 2.0 ** -40
    assert E.bound_units(257, 3.61, 2.0 ** 0.5, 0.64, 2.0 ** -13) == pytest.approx(want, rel=1e-14)
    assert 130 * u < want < 131 * u
    c = E.case("quiet_frames")
    R = E.reference(c)
    babs = E.bound_abs(c, R)
    p = c["plan"]
    j, comp, t = 7, 1, 5
    lam = float(np.abs(p["L"][j].astype(np.float64)).sum())
    rot = abs(float(p["phi"][j].real)) + abs(float(p["phi"][j].imag))
    N = float(np.abs(p["L"][j].astype(np.float64)) @ np.abs(R["Qn"][:, comp, t]))
    B = R["B"][comp, t]
    assert babs[j, comp, t] == pytest.approx(E.bound_units(257, lam, rot, N / B, p["d_bound"]) * B, rel=1e-12)
    worst = float(np.max(babs / R["B"][None])) / u
    print(f"base shape: max lam {np.abs(p['L']).sum(axis=1).max():.2f}, largest bound {worst:.1f} u")
    assert 90 < worst < 120
    # what no plan can exceed (plan_caps): the Lebesgue constant, a full rotation, the node sum at Lam B, D at its limit
    cap = E.bound_units(257, E.LEBESGUE, 2.0 ** 0.5, E.LEBESGUE, E.D_MAX)
    assert E.LEBESGUE == pytest.approx(3.6476, abs=1e-4) and 335 * u < cap < 336 * u and float(np.max(babs / R["B"][None])) <= cap
    bad = dict(p, L=p["L"] * np.float32(1.02))
    with pytest.raises(AssertionError, match="Lebesgue"):
        E.plan_caps(bad)


def test_cases_are_reproducible_and_planned_in_one_interval():
    for family in E.FAMILIES:
        a, b = E.case(family), E.case(family)
        assert np.array_equal(a["data"], b["data"]) and np.array_equal(a["r"], b["r"]) and np.array_equal(a["k"], b["k"])
        assert a["plan"]["interval"] == 0 and a["plan"]["d_bound"] <= 2.0 ** -13
        assert not np.any(a["k"][:, 1:]) and a["k"][0, 0] == 0                     # from Gamma along [100]
