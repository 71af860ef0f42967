"""The cluster analysis without a GPU: the host union-find of tests/cluster_cases.py against a brute-force transitive closure;
every planted fault changes an output on the case meant to catch it; the identities of the result type; the two new entries in
the header and in the ctypes table."""
import re

import numpy as np
import pytest

import angle_cases as Q
import cluster_cases as K
import qlm_cases as C
from conftest import ROOT


@pytest.mark.parametrize("seed", range(12))
def test_union_find_is_the_transitive_closure(seed):
    rng = np.random.default_rng(seed)
    n_a = int(rng.integers(1, 41))
    count, lists, solid = K.random_graph(n_a, seed, degree=float(rng.uniform(0.5, 3.0)), symmetric=bool(seed % 2))
    masks = rng.integers(0, 2 ** 63, (1, n_a)).astype(np.uint64) if seed % 3 == 0 else None
    for link in (0, 1):
        edges = K.edges_of(count[0], lists[0], solid[0], np.full(n_a, 2 ** 64 - 1, np.uint64) if masks is None else masks[0], link)
        got = K.components(count, lists, solid, masks, link, 8)
        assert np.array_equal(got["labels"][0], K.closure_labels(n_a, solid[0], edges))
        assert K.identities(got)
        lab = got["labels"][0]
        assert all(lab[a] == -1 or (lab[a] <= a and lab[lab[a]] == lab[a]) for a in range(n_a))     # the smallest member names it


@pytest.fixture(scope="module")
def walk():
    pos, box, r_cut = C.family("triclinic130")
    pos = np.ascontiguousarray(pos[:3])
    groups = Q.two_species(130)
    return pos, box, r_cut, groups, K.model(pos, box, groups, r_cut, 1, 6, 0.4, 3, 1, 4)


def test_the_twin(walk):
    pos, box, r_cut, groups, want = walk
    assert K.identities(want) and want["n_clusters"].min() >= 2 and want["largest"].max() > 4 and (want["labels"] < 0).any()
    assert np.array_equal(want["species_rows"].sum(axis=1), [3 * 90, 3 * 40])
    pop = np.vectorize(lambda m: bin(int(m)).count("1"))(want["bond_masks"])
    assert np.array_equal(pop, np.maximum(want["connections"], 0))
    # the bond test is symmetric: where a holds b at position s and b holds a at position t, the two bits agree
    for o in range(3):
        for a in range(130):
            for s in range(want["count"][o, a]):
                b = int(want["lists"][o, a, s])
                t = want["lists"][o, b, :want["count"][o, b]].tolist().index(a)
                assert (int(want["bond_masks"][o, a]) >> s) & 1 == (int(want["bond_masks"][o, b]) >> t) & 1


def test_every_fault_shows(walk):
    pos, box, r_cut, groups, want = walk

    def wrong(fault):
        return K.model(pos, box, groups, r_cut, 1, 6, 0.4, 3, 1, 4, fault)
    assert "labels" in K.differs(want, wrong("largest_member")) and "largest_label" in K.differs(want, wrong("largest_member"))
    assert K.differs(want, wrong("link_ignored")) != []
    assert K.differs(want, wrong("overflow_off_by_one")) != [] and want["size_counts"][4] > 0
    assert K.differs(want, wrong("both_lists")) == []                       # (these lists are symmetric: the fault shows on one-sided ones)
    count, lists, solid = K.random_graph(40, 3, symmetric=False)
    assert K.differs(K.components(count, lists, solid), K.components(count, lists, solid, fault="both_lists")) != []
    # left-out atoms treated as solid: a truncated ball and its surroundings
    ball = Q.ball(70, 1, 6.0, n_outside=4)
    groups = [np.arange(ball.shape[1])]
    right = K.model(ball, Q.CUBIC, groups, 6.0, 1, 6, 0.3, 1, 0, 4)
    assert (right["connections"] < 0).any() and np.all(right["labels"][right["connections"] < 0] == -1)
    assert K.differs(right, K.model(ball, Q.CUBIC, groups, 6.0, 1, 6, 0.3, 1, 0, 4, "left_out_solid")) != []


def test_result_type(walk):
    from psa_amd import SolidClusters, clusters
    pos, box, r_cut, groups, want = walk
    rows = np.zeros((2, 69), np.uint64)
    rows[:, :66] = want["species_rows"][:, :66]
    out = dict(want, species_rows=rows)
    res = clusters.result(out, 6, 0.4, 3, "solid_bonds", 4, 3, groups)
    assert isinstance(res, SolidClusters) and res.sizes.tolist() == [0, 1, 2, 3, 4, 5] and res.origins == 3
    exact = int((res.sizes[1:5] * res.size_counts[1:5].astype(np.int64)).sum())
    assert exact + res.large_atoms == int(res.n_solid.sum()) and int(res.size_counts.sum()) == int(res.n_clusters.sum())
    assert np.array_equal(res.largest, res.size_atoms.max(axis=1)) and res.size_counts[0] == 0
    assert np.array_equal(res.mean_size_counts, res.size_counts / 3.0)
    xi = want["connections"]
    assert res.solid_fraction == pytest.approx([(xi[:, :90] >= 3).mean(), (xi[:, 90:] >= 3).mean()])
    assert np.array_equal(res.samples, [270, 120]) and np.array_equal(res.connections.sum(axis=1) + res.truncated, res.samples)
    for o in range(3):
        members = res.largest_atoms(o)
        assert members.size == res.largest[o] and np.all(res.labels[o][np.isin(res.atoms, members)] == res.largest_label[o])
    bare = clusters.result(dict(out, labels=None), 6, 0.4, 3, "solid_bonds", 4, 3, groups)
    with pytest.raises(ValueError, match="per_atom"):
        bare.largest_atoms(0)
    with pytest.raises(IndexError):
        res.largest_atoms(3)
    empty = clusters.result(clusters.empty(1, 4), 6, 0.7, 7, "neighbours", 4, 0, [np.zeros(0, int)])
    assert empty.size_counts.shape == (6,) and empty.n_solid.shape == (0,) and np.isnan(empty.solid_fraction[0])
    assert clusters.link_code("neighbours") == 0 and clusters.link_code("solid_bonds") == 1
    for bad in ("bonds", 0, None):
        with pytest.raises(ValueError):
            clusters.link_code(bad)


def test_abi_agreement():
    """the two entries are declared, bound with as many arguments as the header gives them, and exported"""
    import ctypes

    from psa_amd import _hip
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "psa_hip.h").read_text(), flags=re.S)
    for name in ("psa_solid_clusters", "psa_debug_cluster_labels"):
        args = re.search(rf"\bint {name}\s*\(([^)]*)\)", header).group(1)
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == len([a for a in args.split(",") if a.strip()])
        assert hasattr(ctypes.CDLL(str(_hip.LIB_PATH)), name)
    assert int(re.search(r"#define\s+PSA_HIP_ABI_VERSION\s+(\d+)", header).group(1)) == 6
    assert _hip.CLUSTER_ROW_WORDS == 69 and _hip.CLUSTER_LINKS == ("neighbours", "solid_bonds")
