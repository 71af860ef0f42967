"""The bond-angle route on the host: the NumPy twin of the float32 arithmetic stated at psa_angle_histogram stays inside the
allowance of tests/angle_cases.py on every family, and each planted fault leaves it on a named family -- so the allowance
is tight enough to see them; the reference's own identities; the result type; the calculator's refusals and its empty
result; the ABI table."""
import functools
import logging
import re
from pathlib import Path

import numpy as np
import pytest

import angle64 as A
import angle_cases as Q

ROOT = Path(__file__).resolve().parents[1]


@functools.lru_cache(maxsize=None)
def _case(name, kind, n_theta):
    """(positions, box, groups, r_cut, reference) of a family: kind "one" species with a scalar cut-off, "two" with the
    matrix of angle_cases.matrix_cutoff"""
    pos, box, rc = Q.family(name)
    n = pos.shape[1]
    groups = [np.arange(n)] if kind == "one" else Q.two_species(n)
    r_cut = rc if kind == "one" else Q.matrix_cutoff(rc, 2)
    return pos, box, groups, r_cut, Q.reference(pos, box, groups, r_cut, 1, n_theta)


@functools.lru_cache(maxsize=None)
def _ball():
    pos = Q.ball(100, 2, 6.0, n_outside=3)
    groups = [np.arange(103)]
    return pos, Q.CUBIC, groups, 6.0, Q.reference(pos, Q.CUBIC, groups, 6.0, 1, 45)


def _borderline_first(ref, n_theta, what):
    assert ref["borderline"] <= Q.cap(n_theta) * max(ref["triplets"], 1), what


@pytest.mark.parametrize("n_theta", [45, 180, 1024])
@pytest.mark.parametrize("name", Q.FAMILIES)
def test_twin_inside_the_allowance(name, n_theta):
    pos, box, groups, r_cut, ref = _case(name, "one", n_theta)
    _borderline_first(ref, n_theta, name)
    assert ref["leg_borderline"] == 0 and 2 <= ref["most"] <= Q.CAPACITY and ref["triplets"] > 1000
    got = Q.model(pos, box, groups, r_cut, 1, n_theta)
    assert Q.check(got, ref, f"{name} n_theta {n_theta}")
    assert Q.identities(got, [len(g) for g in groups], pos.shape[0])
    assert Q.identities((ref["angles"], ref["coord"], ref["truncated"]), [len(g) for g in groups], pos.shape[0])


@pytest.mark.parametrize("name", ["cubic130", "triclinic257"])
def test_twin_two_species_and_a_matrix(name):
    pos, box, groups, r_cut, ref = _case(name, "two", 45)
    _borderline_first(ref, 45, name)
    got = Q.model(pos, box, groups, r_cut, 1, 45)
    assert Q.check(got, ref, f"{name} two species") and Q.identities(got, [len(g) for g in groups], pos.shape[0])
    assert not got[0][1, A.pair_row(1, 1, 2)].any() and got[1][1, 1, 0] == pos.shape[0] * len(groups[1])   # r_cut[1][1] = 0: no bond
    assert np.array_equal(got[0][:, A.pair_row(0, 1, 2)].sum(axis=1), ref["cross"][:, A.pair_row(0, 1, 2)])


def test_twin_capacity():
    pos, box, groups, r_cut, ref = _ball()
    assert ref["truncated"][0] == 2 * 100 and ref["most"] == 99 and ref["angles"].sum() == 2 * 3   # the three outside see each other
    got = Q.model(pos, box, groups, r_cut, 1, 45)
    assert Q.check(got, ref, "ball") and Q.identities(got, [103], 2)
    assert got[1][0, 0].sum() == 2 * 3 and got[1][0, 0, 2] == 2 * 3          # the three outside are the only centres counted


# the family each fault is held against
FAULT_FAMILY = {"no_image": ("triclinic130", "one"), "orthogonal_only": ("triclinic130", "one"), "one_cutoff": ("cubic130", "two"),
                "diagonal_doubled": ("cubic37", "one"), "self_included": ("cubic37", "one"), "angle_at_b": ("cubic130", "one"),
                "cos_bins": ("triclinic257", "one"), "bin_shift": ("cubic37", "one"), "first_64": ("ball", "one")}


@pytest.mark.parametrize("fault", Q.FAULTS)
def test_planted_faults_leave_the_allowance(fault):
    name, kind = FAULT_FAMILY[fault]
    pos, box, groups, r_cut, ref = _ball() if name == "ball" else _case(name, kind, 45)
    _borderline_first(ref, 45, name)
    assert Q.check(Q.model(pos, box, groups, r_cut, 1, 45), ref, f"{name} clean")
    assert not Q.check(Q.model(pos, box, groups, r_cut, 1, 45, fault=fault), ref, f"{name} {fault}")


def test_faults_are_the_issue_s_list():
    assert set(FAULT_FAMILY) == set(Q.FAULTS) and len(Q.FAULTS) == 9


def test_table_bins():
    """the table's bin of the edges themselves, of +-1 and between: cedge[i + 1] < cos <= cedge[i]"""
    for n_theta in (1, 45, 1024):
        edge = Q.cos_edges(n_theta)
        assert edge[0] == 1.0 and edge[-1] == -1.0 and np.all(np.diff(edge) < 0)
        i = np.arange(n_theta)
        assert np.array_equal(Q.table_bin(edge[:n_theta], edge), i)         # an edge is the upper end of its bin
        assert Q.table_bin(np.float32(-1.0), edge) == n_theta - 1
        assert np.array_equal(Q.table_bin(np.nextafter(edge[1:], np.float32(2.0)), edge), i)


def test_result_type():
    import psa_amd
    from psa_amd import BondAngleDistribution, angles
    assert "BondAngleDistribution" in psa_amd.__all__
    pos, box, groups, r_cut, ref = _case("cubic130", "two", 45)
    res = angles.distribution(ref["angles"].astype(np.uint64), ref["coord"].astype(np.uint64), ref["truncated"].astype(np.uint64), 45,
                              pos.shape[0], groups)
    assert isinstance(res, BondAngleDistribution) and res.counts.shape == (2, 3, 45) and res.undefined.shape == (2, 3)
    assert np.array_equal(res.pairs, [[0, 0], [0, 1], [1, 1]]) and res.origins == 12 and np.array_equal(res.samples, [12 * 90, 12 * 40])
    assert res.theta_edges[0] == 0.0 and res.theta_edges[-1] == 180.0 and np.allclose(res.theta, 2.0 + 4.0 * np.arange(45))
    assert np.array_equal(res.triplet(1, 0, 1), res.counts[1, 1]) and np.array_equal(res.triplet(1, 1, 0), res.counts[1, 1])
    dens = res.density
    assert np.allclose((dens * 4.0).sum(axis=2)[res.counts.sum(axis=2) > 0], 1.0) and not dens[1, 2].any()
    frac = res.coordination_fraction
    assert np.allclose(frac.sum(axis=2), 1.0) and res.coordination_counts.shape == (2, 2, 65)
    want = (ref["coord"] * np.arange(65)).sum(axis=2) / ref["coord"].sum(axis=2)
    assert np.allclose(res.mean_coordination, want) and res.mean_coordination[1, 1] == 0.0


def _calculator(pos, box, types=None):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, 1, 1, 1)


def test_calculator_refusals_and_the_empty_result(caplog):
    from psa_amd import BondAngleDistribution, max_pair_radius
    pos = Q.family("cubic37")[0]
    calc = _calculator(pos, Q.CUBIC, (np.arange(37) % 2 + 1).astype(np.int32))
    served = max_pair_radius(Q.CUBIC)
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="n_theta"):
            calc.calculate_bond_angles(3.0, bad)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, 2.0]):
        with pytest.raises(ValueError, match="r_cut"):
            calc.calculate_bond_angles(bad)
    with pytest.raises(ValueError, match="served radius"):
        calc.calculate_bond_angles(served * 1.001)
    with pytest.raises(ValueError, match="symmetric"):
        calc.calculate_bond_angles([[3.0, 2.0], [2.5, 3.0]], basis_atom_types=[1, 2])
    with pytest.raises(ValueError, match="symmetric"):
        calc.calculate_bond_angles(np.full((3, 3), 3.0), basis_atom_types=[1, 2])
    with pytest.raises(ValueError, match="origin_step"):
        calc.calculate_bond_angles(3.0, origin_step=0)
    with pytest.raises(ValueError, match="disjoint"):
        calc.calculate_bond_angles(3.0, basis_atom_indices=[[0, 1], [1, 2]])
    empty = _calculator(pos[:0], Q.CUBIC)
    with caplog.at_level(logging.WARNING):
        res = empty.calculate_bond_angles(3.0, 30)
    assert "0 frames or 0 atoms" in caplog.text
    assert isinstance(res, BondAngleDistribution) and res.counts.shape == (1, 1, 30) and not res.counts.any() and res.origins == 0
    assert not res.density.any() and not res.coordination_fraction.any() and res.coordination_counts.shape == (1, 1, 65)


def test_abi_table():
    from psa_amd import _hip
    head = (ROOT / "include" / "psa_hip.h").read_text()
    for name, n_args in (("psa_angle_histogram", 14), ("psa_debug_neighbour_lists", 10)):
        assert re.search(rf"\bint {name}\(", head) and len(_hip.SIGNATURES[name][1]) == n_args
    lib = _hip.load_library()
    assert lib.psa_abi_version() == _hip.ABI_VERSION and lib.psa_angle_histogram and lib.psa_debug_neighbour_lists
    assert hasattr(_hip.Engine, "angle_histogram") and hasattr(_hip.Engine, "debug_neighbour_lists")
