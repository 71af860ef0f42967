"""The common-neighbour analysis without a GPU: the NumPy twin of the arithmetic stated at psa_common_neighbours equals the
float64 reference of tests/cna64.py on every case of the GPU test, by the very comparison that test makes (cna_cases.check);
every planted fault of the twin is caught by that comparison, or by the closed form, on the very inputs the GPU test uses;
the graph code against hand-made graphs; the header, the binding and the result type."""
import functools
import re

import numpy as np
import pytest

import angle_cases as Q
import cna64 as R
import cna_cases as C
from conftest import ROOT

KINDS = ("one", "two", "three")


@functools.lru_cache(maxsize=None)
def _case(name, kind, matrix):
    pos, box, rc = Q.family(name)
    groups = C.species(kind, pos.shape[1])
    r_cut = C.cutoffs(kind, rc, matrix)
    return pos, box, groups, r_cut, C.Reference(pos, box, groups, r_cut)


# ---- the graph code, by hand -----------------------------------------------------------------------------------------------------
def _sig(nodes, edges):
    e = {frozenset(p) for p in edges}
    return R.signature(list(nodes), lambda u, v: frozenset((u, v)) in e)


def test_signatures_of_hand_made_graphs():
    assert _sig([], []) == (0, 0, 0) and _sig([1, 2, 3], []) == (3, 0, 0)
    assert _sig(range(4), [(0, 1), (2, 3)]) == (4, 2, 1)                   # fcc: two separate bonds
    assert _sig(range(4), [(0, 1), (1, 2)]) == (4, 2, 2)                   # hcp: a chain of two
    assert _sig(range(5), [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]) == (5, 5, 5)
    assert _sig(range(4), [(0, 1), (0, 2), (0, 3)]) == (4, 3, 3)           # a star: three bonds, the longest simple path has two
    assert _sig(range(6), [(0, 1), (2, 3), (3, 4), (4, 5), (5, 2)]) == (6, 5, 4)   # the largest piece is not the first
    assert R.pack(4, 2, 1) == 0x010204 and R.pack(63, 1953, 1953) == 63 | 255 << 8 | 255 << 16
    assert R.classify([(4, 2, 1)] * 12) == 1 and R.classify([(4, 2, 1)] * 6 + [(4, 2, 2)] * 6) == 2
    assert R.classify([(6, 6, 6)] * 8 + [(4, 4, 4)] * 6) == 3 and R.classify([(5, 5, 5)] * 12) == 4
    assert R.classify([(4, 2, 1)] * 11) == 0 and R.classify([]) == 0 and R.classify([(6, 6, 6)] * 8 + [(4, 4, 4)] * 4) == 0


def test_masks_of_the_twin_on_hand_made_graphs():
    """the flood over masks against the graph code, on random graphs up to 64 nodes (bit 63 among them)"""
    rng = np.random.default_rng(4)
    for n, p in ((1, 0.5), (2, 1.0), (7, 0.4), (12, 0.3), (33, 0.1), (64, 0.05), (64, 0.5)):
        adj = np.triu(rng.random((n, n)) < p, 1)
        adj = adj | adj.T
        rows = [sum(1 << int(j) for j in np.flatnonzero(r)) for r in adj]
        _, words = C.centre_model(rows, n)
        want = [R.pack(*R.signature([c for c in range(n) if adj[b, c]], lambda u, v: adj[u, v])) for b in range(n)]
        assert words == want, (n, p)


# ---- the twin equals the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(Q.FAMILIES))
def test_twin_equals_the_reference(name, kind, matrix):
    pos, box, groups, r_cut, ref = _case(name, kind, matrix)
    assert ref.excluded().mean() <= C.EXCLUDED_CAP
    print(f"{name} {kind} matrix {matrix}: {ref.bonds} bonds, {ref.branching} branching, closest |x - 1| = {ref.closest:.3g}, |r - r_cut| = {ref.closest_r:.3g}, "
          f"excluded {int(ref.excluded().sum())}")
    for step in (1, 3, pos.shape[0] + 1):
        got = C.model(pos, box, groups, r_cut, step)
        assert C.check(got, ref.result(step), ref.excluded(step), f"{name} {kind} {matrix} step {step}")


def test_no_pair_near_a_cut_off_and_what_the_inputs_hold():
    """over all frames of the four families: no pair's distance within 4e-6 of its cut-off (the nearest, in triclinic130, is
    1.15e-5 away, 1.9e-6 of r_cut: outside the tolerance, so no centre is excluded), more than 100 bonds,
    at least 50 distinct signatures, bonds whose common-neighbour graph branches, bonds outside the table"""
    for name in Q.FAMILIES:
        pos, box, groups, r_cut, ref = _case(name, "one", False)
        res = ref.result()
        assert ref.closest_r > 4e-6 and not ref.excluded().any(), (name, ref.closest_r)
        assert ref.bonds > 100 and C.distinct_signatures(res) >= 50 and ref.branching > 0 and res["signature_outside"].sum() > 0, name


def _walk_reference(split):
    """the walk case as the GPU test compares it: the integer route over the lists (here the twin's own lists)"""
    pos, box, groups, r_cut = C.walk_split() if split else Q.walk_case()
    frames = []
    for near in C.near32(pos, box, groups, r_cut):
        count = near.sum(axis=1).astype(np.int32)
        lists = np.full((near.shape[0], C.CAPACITY), -1, np.int32)
        for a, row in enumerate(near):
            nb = np.flatnonzero(row)[:C.CAPACITY]
            lists[a, :nb.size] = nb
        frames.append((count,) + C.from_lists(count, lists))
    return pos, box, groups, r_cut, C.with_groups(C.result_of(frames, groups), groups)


@pytest.mark.parametrize("split", [False, True])
def test_twin_equals_the_lists_route_on_the_walk_case(split):
    pos, box, groups, r_cut, ref = _walk_reference(split)
    assert Q.walk_counts(ref["n"]) or split
    assert (ref["n"] == 64).any() and (ref["n"] == 65).any() and (ref["types"] == -1).sum() == 2
    assert C.check(C.model(pos, box, groups, r_cut), ref, None, "walk case")


@pytest.mark.parametrize("name", ["fcc", "bcc", "hcp", "ico", "diamond"])
def test_closed_forms_of_the_twin_and_the_reference(name):
    pos, box, groups, r_cut = C.closed_inputs(name)
    ref = C.Reference(pos, box, groups, r_cut)
    assert ref.closest >= 0.098 and C.closed_form_holds(name, ref.result())   # the icosahedron's edge: 9.9 % of r_cut below it, 11 % of itself
    assert C.closed_form_holds(name, C.model(pos, box, groups, r_cut))


# ---- every planted fault is caught ---------------------------------------------------------------------------------------------
# fault: the input of the GPU test that shows it -- a family (name, kind, matrix), "walk" or a closed form
CATCHES = {"longest_path": ("cubic37", "one", True), "bonds_twice": ("cubic130", "one", False), "self_common": ("cubic37", "two", False),
           "first_component": ("triclinic130", "one", False), "bit63_dropped": "walk", "half_round_twice": ("cubic130", "two", False),
           "one_cutoff": ("triclinic257", "three", True), "bcc_at_12": "bcc", "first_64": "walk"}


@pytest.mark.parametrize("fault", C.FAULTS)
def test_planted_fault_is_caught(fault):
    where = CATCHES[fault]
    if where == "walk":
        pos, box, groups, r_cut, ref = _walk_reference(False)
        assert not C.check(C.model(pos, box, groups, r_cut, 1, fault), ref, None, fault)
    elif where == "bcc":
        pos, box, groups, r_cut = C.closed_inputs("bcc")
        assert not C.closed_form_holds("bcc", C.model(pos, box, groups, r_cut, 1, fault))
    else:
        pos, box, groups, r_cut, ref = _case(*where)
        assert not C.check(C.model(pos, box, groups, r_cut, 3, fault), ref.result(3), ref.excluded(3), fault)


def test_faults_are_all_listed():
    assert set(CATCHES) == set(C.FAULTS) and len(C.FAULTS) == 9


# ---- the header, the binding, the result type -----------------------------------------------------------------------------------
def test_header_binding_and_exports():
    import psa_amd
    from psa_amd import _hip
    header = (ROOT / "include" / "psa_hip.h").read_text()
    assert "int psa_common_neighbours(" in header and int(re.search(r"#define\s+PSA_HIP_ABI_VERSION\s+(\d+)", header).group(1)) == _hip.ABI_VERSION
    for word in ("signature_counts (S, 8, 16, 16)", "type_counts (n_o, S, 5)", "plus 8 n_a", "plus 256 n_a", "largest connected component"):
        assert word in header, word
    assert "psa_common_neighbours" in _hip.SIGNATURES and len(_hip.SIGNATURES["psa_common_neighbours"][1]) == 19
    lib = _hip.load_library()
    assert lib.psa_common_neighbours and hasattr(_hip.Engine, "common_neighbours")
    assert _hip.CNA_TABLE == R.TABLE and _hip.CNA_TYPES == R.TYPES
    assert psa_amd.CommonNeighbours is psa_amd.cna.CommonNeighbours and "CommonNeighbours" in psa_amd.__all__
    assert hasattr(psa_amd.SEDCalculator, "calculate_common_neighbours")
    assert psa_amd.cna.pack(4, 2, 1) == R.pack(4, 2, 1) and psa_amd.cna.pack(9, 300, 1000) == R.pack(9, 300, 1000)


def test_result_type():
    from psa_amd import cna
    pos, box, groups, r_cut, ref = _case("cubic37", "two", False)
    out = dict(ref.result(3))
    res = cna.result(out, out["types"].shape[0], groups)
    assert res.structure_names == ("other", "fcc", "hcp", "bcc", "ico") and res.origins == 14 and res.sizes.tolist() == [len(g) for g in groups]
    assert np.array_equal(res.bonds, out["signature_counts"].reshape(2, -1).sum(axis=1) + out["signature_outside"])
    assert np.array_equal(res.signature(2, 1, 1), out["signature_counts"][:, 2, 1, 1]) and res.fraction("other").shape == (14, 2)
    assert np.allclose(sum(res.fraction(t) for t in range(5)), 1.0) and np.array_equal(res.fraction("fcc"), res.fraction(1))
    assert res.share(2, 1, 1) == pytest.approx(float(out["signature_counts"][:, 2, 1, 1].sum()) / float(res.bonds.sum()))
    assert np.array_equal(res.atoms_of(2, "other"), res.atoms[out["types"][2] == 0]) and res.atoms.shape == (37,)
    bare = cna.result(cna.empty(1), 0, [np.zeros(0, int)])
    assert bare.types is None and np.isnan(bare.share(4, 2, 1)) and bare.type_counts.shape == (0, 1, 5)
    with pytest.raises(ValueError, match="per-atom output"):
        bare.atoms_of(0, "fcc")
    with pytest.raises(ValueError, match="type must be one of"):
        res.fraction("sc")
    with pytest.raises(ValueError, match="the table holds"):
        res.signature(8, 0, 0)
    with pytest.raises(IndexError):
        res.atoms_of(14, 0)
