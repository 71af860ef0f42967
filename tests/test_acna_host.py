"""The adaptive common-neighbour analysis without a GPU: the NumPy float32 twin of the arithmetic stated at
psa_adaptive_common_neighbours equals the float64 reference of tests/acna64.py on every case of the GPU test, by the very
comparison that test makes (acna_cases.check); eight of the nine planted faults of the twin lie outside that comparison on an
input of the GPU test, and the ninth, a tie dropped in the rank, outside the closed form of perfect fcc instead (the thermal
inputs hold no exact tie for the comparison to see); the cap on the excluded centres and what the inputs hold, on the
reference alone; the header, the binding and the result type."""
import functools
import re

import numpy as np
import pytest

import acna64 as R
import acna_cases as C
from conftest import ROOT
# the feature's own constants, at import: without the feature nothing in this file runs
from psa_amd._hip import ACNA_MEMBERS, CNA_TABLE, CNA_TYPES
from psa_amd.acna import NO_BOND, AdaptiveCommonNeighbours

# the least ratio of a decision's distance to its tolerance that each input is held to, the rank labels among the decisions
# (measured: 4.57, 4.92, 2.70, 1.80; above 1 no centre is excluded).  The gas: none of the seeds 0 .. 63 reaches 3
CLEARANCE = {"fcc": 3.0, "bcc": 3.0, "hcp": 2.5, "gas": 1.75}


@functools.lru_cache(maxsize=None)
def _case(name, kind="one", matrix=False):
    pos, box, rc = C.case(name)
    groups = C.species(kind, pos.shape[1])
    r_cut = C.cutoffs(kind, rc, matrix)
    return pos, box, groups, r_cut, C.Reference(pos, box, groups, r_cut)


CONFIGS = [(name, "one", False) for name in C.CASES] + [("hcp", "two", False), ("gas", "two", True)]


# ---- the reference by hand ---------------------------------------------------------------------------------------------------
def test_reference_constants_and_cut_offs():
    assert ACNA_MEMBERS == R.MEMBERS == C.MEMBERS and NO_BOND == R.NO_BOND and CNA_TABLE == C.cna64.TABLE and CNA_TYPES == C.cna64.TYPES
    assert AdaptiveCommonNeighbours.__dataclass_fields__.keys() >= {"short", "cutoffs", "nearest"}
    assert R.K == pytest.approx(1.2071067811865475, abs=1e-15) and R.WEIGHT == pytest.approx(1.1547005383792517, abs=1e-15)
    # equal lengths: r_A = K rho; the two bcc shells at sqrt 3 / 2 a and a: r_B = K a
    assert R.local_cutoff(np.full(12, 2.0), "A") == pytest.approx(2.0 * R.K, rel=1e-15)
    rho = np.array([np.sqrt(3.0) / 2.0] * 8 + [1.0] * 6)
    assert R.local_cutoff(rho, "B") == pytest.approx(R.K, rel=1e-15)
    assert float(C.K12) == float(np.float32(R.K / 12.0)) and float(C.K14) == float(np.float32(R.K / 14.0))


# ---- the twin equals the reference, the cap, what the inputs hold ------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
def test_twin_equals_the_reference(config):
    pos, box, groups, r_cut, ref = _case(*config)
    assert ref.excluded().mean() <= C.EXCLUDED_CAP
    print(f"{config}: margin {ref.margin:.3g}, clearance {ref.clearance:.3g}, excluded {int(ref.excluded().sum())}, "
          f"test B on {ref.ran_b}, 12 or 13 candidates {ref.few}")
    for step in (1, 3, pos.shape[0] + 1):
        got = C.model(pos, box, groups, r_cut, step)
        assert C.check(got, ref.result(step), ref.excluded(step), ref.cut_tolerance(step), f"{config} step {step}")


def test_the_cap_and_what_the_inputs_hold():
    """on the reference alone: no centre excluded (so the cap holds, with a margin left after the tolerance), every decision
    -- the rank labels among them -- at CLEARANCE tolerances from its edge or more; at least 50 centres of the crystal's own
    type and 30 other in each thermal case; test B on at least 100 centres; a centre with 12 or 13 candidates; the gas: all
    other, every centre through test B, 200 signatures"""
    ran_b = few = 0
    for name in C.CASES:
        ref = _case(name)[4]
        res = ref.result()
        assert ref.excluded().mean() <= C.EXCLUDED_CAP and not ref.excluded().any() and ref.margin > 0.0, (name, ref.margin)
        assert ref.clearance >= CLEARANCE[name], (name, ref.clearance)
        census = res["type_counts"].sum(axis=(0, 1))
        if name in C.OWN_TYPE:
            assert census[C.OWN_TYPE[name]] >= 50 and census[0] >= 30, (name, census)
        else:
            assert census[0] == res["types"].size and ref.ran_b == res["types"].size and C.distinct_signatures(res) >= 200
        assert not res["truncated"].any() and not res["short"].any(), name
        ran_b, few = ran_b + ref.ran_b, few + ref.few
    assert ran_b >= 100 and few >= 1
    matrix = _case("gas", "two", True)[4]
    assert not matrix.excluded().any() and matrix.result()["short"][0] > 0 and matrix.few > 0


@pytest.mark.parametrize("name", ["fcc", "bcc", "hcp", "ico", "diamond"])
def test_closed_forms_of_the_twin_and_the_reference(name):
    pos, box, groups, r_cut = C.closed_inputs(name)
    pos = pos[:1]
    assert C.closed_form_holds(name, C.model(pos, box, groups, r_cut))
    if name != "bcc":                                                      # (perfect bcc: rho_11 = rho_12, the members of test A
        assert C.closed_form_holds(name, C.Reference(pos, box, groups, r_cut).result())   # are the tie rule's; test B decides)
    if name == "fcc":
        cut = C.model(pos, box, groups, r_cut)["cutoffs"]
        want = np.float32(R.K * float(np.float32(21.72)) / 4.0 / np.sqrt(2.0))
        assert np.all(np.abs(cut.astype(np.float32) - want) <= 4 * np.spacing(want))


# ---- every planted fault is caught ---------------------------------------------------------------------------------------------
# fault: the input of the GPU test that shows it -- a case of the comparison; tie_dropped alone: the closed form of perfect fcc
CATCHES = {"first_12": "fcc", "mean_of_all": "fcc", "r_cut_itself": "fcc", "bcc_first": "gas", "no_weight": "bcc", "thirteen": "fcc",
           "leg_difference": "hcp", "tie_dropped": "closed fcc", "bonds_of_a": "bcc"}


@pytest.mark.parametrize("fault", C.FAULTS)
def test_planted_fault_is_caught(fault):
    where = CATCHES[fault]
    if where.startswith("closed"):
        pos, box, groups, r_cut = C.closed_inputs(where.split()[1])
        assert not C.closed_form_holds(where.split()[1], C.model(pos[:1], box, groups, r_cut, 1, fault))
    else:
        pos, box, groups, r_cut, ref = _case(where)
        step = 1 if where == "hcp" else pos.shape[0] + 1                   # one origin shows it; hcp: a later frame
        assert not C.check(C.model(pos, box, groups, r_cut, step, fault), ref.result(step), ref.excluded(step), ref.cut_tolerance(step),
                           fault)


def test_faults_are_all_listed():
    assert set(CATCHES) == set(C.FAULTS) and len(C.FAULTS) == 9


# ---- the header, the binding, the result type -----------------------------------------------------------------------------------
def test_header_binding_and_exports():
    import psa_amd
    from psa_amd import _hip
    header = (ROOT / "include" / "psa_hip.h").read_text()
    assert "int psa_adaptive_common_neighbours(" in header
    assert int(re.search(r"#define\s+PSA_HIP_ABI_VERSION\s+(\d+)", header).group(1)) == _hip.ABI_VERSION
    for word in ("rank(i) = #{j : s_j < s_i} + #{j < i : s_j = s_i}", "K = (1 + sqrt 2) / 2", "float32(2 / sqrt 3)", "plus 12 n_a",
                 "plus 112 n_a", "nearest (n_o, n_a, 14)", "short_centres (S)"):
        assert word in header, word
    assert len(_hip.SIGNATURES["psa_adaptive_common_neighbours"][1]) == 22
    lib = _hip.load_library()
    assert lib.psa_adaptive_common_neighbours and hasattr(_hip.Engine, "adaptive_common_neighbours")
    assert _hip.ACNA_MEMBERS == R.MEMBERS
    assert psa_amd.AdaptiveCommonNeighbours is psa_amd.acna.AdaptiveCommonNeighbours and "AdaptiveCommonNeighbours" in psa_amd.__all__
    assert issubclass(psa_amd.AdaptiveCommonNeighbours, psa_amd.CommonNeighbours)
    assert hasattr(psa_amd.SEDCalculator, "calculate_adaptive_common_neighbours")
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert "psa_adaptive_common_neighbours" in integration


def test_result_type():
    from psa_amd import acna
    pos, box, groups, r_cut, ref = _case("hcp", "two", False)
    out = dict(ref.result(3))
    out["cutoffs"] = out["cutoffs"].astype(np.float32)
    res = acna.result(out, out["types"].shape[0], groups)
    assert res.structure_names == ("other", "fcc", "hcp", "bcc", "ico") and res.origins == 2 and res.sizes.tolist() == [len(g) for g in groups]
    assert res.signature_counts.shape == (2, 8, 16, 16) and res.signature_counts.dtype == np.uint64 and res.type_counts.shape == (2, 2, 5)
    assert res.short.shape == (2,) and res.truncated.shape == (2,) and res.types.dtype == np.int32 and res.neighbours.dtype == np.int32
    assert res.cutoffs.shape == (2, 64) and res.cutoffs.dtype == np.float32 and res.nearest.shape == (2, 64, 14) and res.nearest.dtype == np.int32
    assert res.bond_signatures.shape == (2, 64, 14) and res.bond_signatures.dtype == np.uint32 and res.atoms.shape == (64,)
    assert np.array_equal(res.bonds, out["signature_counts"].reshape(2, -1).sum(axis=1) + out["signature_outside"])
    assert np.array_equal(res.signature(4, 2, 1), out["signature_counts"][:, 4, 2, 1]) and res.fraction("hcp").shape == (2, 2)
    assert np.allclose(sum(res.fraction(t) for t in range(5)), 1.0) and np.array_equal(res.fraction("hcp"), res.fraction(2))
    assert 0.0 < res.share(4, 2, 1) < 1.0
    assert res.share(4, 2, 1) == pytest.approx(float(out["signature_counts"][:, 4, 2, 1].sum()) / float(res.bonds.sum()))
    assert np.array_equal(res.atoms_of(1, "hcp"), res.atoms[out["types"][1] == 2]) and res.atoms_of(1, "hcp").size > 0
    bare = acna.result(acna.empty(1), 0, [np.zeros(0, int)])
    assert bare.types is None and bare.cutoffs is None and bare.nearest is None and np.isnan(bare.share(4, 2, 1))
    assert bare.type_counts.shape == (0, 1, 5) and bare.short.tolist() == [0]
    with pytest.raises(ValueError, match="calculate_adaptive_common_neighbours"):
        bare.atoms_of(0, "fcc")
    with pytest.raises(ValueError, match="type must be one of"):
        res.fraction("sc")
    with pytest.raises(ValueError, match="the table holds"):
        res.signature(8, 0, 0)
    with pytest.raises(IndexError):
        res.atoms_of(2, 0)
