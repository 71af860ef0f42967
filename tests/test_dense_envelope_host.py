"""Proof, without a GPU, that the dense kernels' float64 envelope (tests/test_gpu_dense_envelope.py) can fail.

The NumPy models of tests/dense_cases.py restate the "2 x f16" and the "3 x bf16" split with float64 accumulation.  For
every input family that has quiet frames:
  * the correct model and the float32 oracle lie under the bound of every form;
  * the model that loses the second piece of d on the quiet frames only lies at least 5 x over the bound of its form;
  * that same faulty output is under 2e-6 in rel_max, the tightest bar of the older dense tests: they would pass it.

The f16 rows run on the families as the GPU suite uses them (quiet frames at 2^-10).  The bf16 rows run on frames
quieter by another 2^-2 (2^-12, well within the 2^-17 of the envelope): the second bf16 piece is 2^-9 of a value, eight
times the float16 one, and with 2^-10 its loss sits at 1.2e-6 .. 2.0e-6 in rel_max, on the old bar instead of under it.
gamma does not depend on how quiet the frames are, so the factor over the bound is the same.

Known limit: the loss of the THIRD bf16 piece (2^-16 of a value) is below any bound that can be derived for one
unfolded chain over all stages ((6 + 2 S) u), so the envelope sees the second piece only."""
import numpy as np
import pytest

import dense_cases as D
from conftest import rel_max
from ref64 import gamma, project64, scale_B

MODELS = {"f16": (D.model_f16, -10), "bf16": (D.model_bf16, -12)}         # split: (model, exponent of the quiet frames)
OLD_BAR = 2e-6


def _reference(c):
    args = (c["data"], c["r"])
    return (project64(*args, c["k"], c["idx"], c["weights"], c["disp"]), scale_B(*args, c["idx"], c["weights"], c["disp"]))


@pytest.mark.parametrize("split", list(MODELS))
@pytest.mark.parametrize("family", D.QUIET_FAMILIES)
def test_lost_second_piece_is_seen_by_gamma_and_not_by_rel_max(family, split):
    model, quiet_exp = MODELS[split]
    c = D.case(family, quiet_exp=quiet_exp)
    ref, B = _reference(c)
    good, bad = model(c), model(c, lose=c["quiet"])
    # the tightest bound of the split's forms for what must pass, the loosest for what must fail (F = 8 or 10)
    bounds = [D.bound(f, c["n_g"]) for f in (("pair", "planes_wide") if split == "f16" else ("bf16x3",))]
    tight, loose = min(bounds), max(bounds)
    g_good, g_bad, g_o32 = gamma(good, ref, B), gamma(bad, ref, B), gamma(D.oracle32(c), ref, B)
    print(f"{family} {split} n_g={c['n_g']}: bound {tight:.2e} / {loose:.2e}, gamma correct {g_good:.2e}, float32 oracle "
          f"{g_o32:.2e}, second piece lost {g_bad:.2e} = {g_bad / loose:.1f} x bound, its rel_max {rel_max(bad, ref):.2e}")
    assert g_good <= tight and g_o32 <= tight
    assert g_bad >= 5 * loose
    assert rel_max(bad, ref) < OLD_BAR


@pytest.mark.parametrize("family", [f for f in D.FAMILIES if f not in D.QUIET_FAMILIES])
def test_models_and_oracle_are_under_every_bound(family):
    c = D.case(family)
    ref, B = _reference(c)
    tight = min(D.bound(f, c["n_g"]) for f in D.FORMS)
    for name, got in (("f16", D.model_f16(c)), ("bf16", D.model_bf16(c)), ("oracle", D.oracle32(c))):
        g = gamma(got, ref, B)
        print(f"{family} {name}: gamma {g:.2e}, tightest bound {tight:.2e}")
        assert g <= tight


@pytest.mark.parametrize("n_g", [257, 1000])
def test_factor_grows_with_fewer_atoms(n_g):
    """the error of a lost piece adds up like sqrt(n_g), B like n_g"""
    c = D.case("quiet_frames", n=n_g)
    ref, B = _reference(c)
    g = gamma(D.model_f16(c, lose=c["quiet"]), ref, B)
    assert g >= (40 if n_g == 257 else 15) * D.bound("pair", n_g), g


def test_bounds_are_the_documented_ones():
    u = 2.0 ** -24
    assert D.bound("pair", 1000) == 18 * u and D.bound("planes_lw", 257) == 16 * u and D.bound("planes128", 4096) == 30 * u
    assert D.bound("planes_wide", 1000) == 20 * u and D.bound("planes_wide", 321) == 18 * u
    assert D.bound("bf16x3", 1000) == 70 * u and D.bound("mfma32", 641) == 645 * u and D.bound("wave", 1) == 5 * u


def test_gamma_metric():
    ref = np.zeros((2, 3, 4), np.complex128)
    ref[0, 1, 2] = 1 + 1j
    B = np.ones((3, 4))
    B[0, 0] = 0.0
    got = ref.copy()
    got[0, 1, 2] += 1e-3j                            # the imaginary part on its own
    got[1, 2, 3] += 2e-3
    B[2, 3] = 4.0
    assert gamma(got, ref, B) == pytest.approx(1e-3)
    assert gamma(np.zeros_like(ref), ref, np.zeros((3, 4))) == 0.0
    got[1, 0, 0] = 1e-30                             # B = 0 there: must be exactly zero
    with pytest.raises(AssertionError):
        gamma(got, ref, B)


def test_families_are_reproducible_and_inside_the_envelope():
    for family in D.FAMILIES:
        a, b = D.case(family), D.case(family)
        assert np.array_equal(a["data"], b["data"]) and np.array_equal(a["r"], b["r"]) and np.array_equal(a["k"], b["k"])
        x = np.abs(a["data"][a["data"] != 0]) if not a["disp"] else None
        if x is not None and x.size:
            # the values that carry B (above 2^-17 of the maximum) are all but a vanishing share of it
            top = x.max()
            assert x[x < top * 2.0 ** -17].sum() <= 1e-6 * x.sum(), family
    top = np.abs(D.case("pow2_max_-30")["data"]).max()
    assert top == np.float32(2.0 ** -30) and np.abs(D.case("pow2_max_below_1")["data"]).max() < 1
