"""The bond persistence on the host: the NumPy twin of the float32 arithmetic stated at psa_bond_persistence stays inside the
allowance of tests/persist_cases.py on every family, and each planted fault leaves it on a named case -- so the allowance is
tight enough to see them; the inputs keep the borderline share of the bond events below the cap; the reference's own counts
are those of the brute force of tests/persist64.py and obey the identities; the result type's arithmetic; every refusal of
the Python layers; the ABI table."""
import functools
import logging
import re
from pathlib import Path

import numpy as np
import pytest

import angle_cases as Q
import persist64 as R
import persist_cases as C

ROOT = Path(__file__).resolve().parents[1]
# (the matrix of cut-offs?, r_break / r_cut, origin_step -- None: above T --, sample_step, continuous)
CONFIGS = [(False, 1.0, 1, 1, True), (True, C.HYSTERESIS, 1, 1, True), (False, C.HYSTERESIS, 3, 2, True), (True, 1.0, None, 1, False),
           (False, C.HYSTERESIS, 1, 2, False)]


@functools.lru_cache(maxsize=None)
def _frames(name, kind):
    pos, box, rc = Q.family(name)
    groups = C.species(kind, pos.shape[1])
    return pos, box, rc, groups, C.Frames(pos, box, groups), C.lengths32(pos, box, groups)


@functools.lru_cache(maxsize=None)
def _case(name, kind, config):
    matrix, factor, step, ss, cont = config
    pos, box, rc, groups, frames, lengths = _frames(name, kind)
    T = pos.shape[0]
    r_cut = C.cutoffs(kind, rc, matrix)
    r_break = C.breaks(r_cut, factor)
    args = (pos, box, groups, r_cut, r_break, C.lags_of(T, ss), T + 1 if step is None else step, ss, cont)
    return args, C.reference(*args, frames=frames), lengths


@functools.lru_cache(maxsize=None)
def _walk(split, factor, cont=True, ss=1):
    pos, box, groups, r_cut = C.walk_split() if split else Q.walk_case()
    args = (pos, box, groups, r_cut, C.breaks(r_cut, factor), [0, 2, 4] if ss == 2 else [0, 1, 2, 4], 1, ss, cont)
    return args, C.reference(*args), C.lengths32(pos, box, groups)


def _borderline_first(ref, what):
    assert ref["borderline"] <= C.BORDERLINE_CAP * max(ref["events"], 1) and ref["events"] > 1000, what


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("kind", ["one", "two", "three"])
@pytest.mark.parametrize("name", list(Q.FAMILIES))
def test_twin_inside_the_allowance(name, kind, config):
    args, ref, lengths = _case(name, kind, config)
    what = f"{name} {kind} {config}"
    _borderline_first(ref, what)
    assert 2 <= ref["most"] <= C.CAPACITY and ref["bonds"].sum() > 100
    got = C.model(*args, lengths=lengths)
    sizes, T = [len(g) for g in args[2]], args[0].shape[0]
    assert C.check(got, ref, what)
    assert C.identities(got, sizes, T, args[5], args[6], args[8]) and C.identities(ref, sizes, T, args[5], args[6], args[8])


@pytest.mark.parametrize("split", [False, True])
def test_twin_on_the_walk_case(split):
    args, ref, lengths = _walk(split, C.HYSTERESIS)
    _borderline_first(ref, "walk case")
    assert ref["most"] == 65 and ref["truncated"][:, 0].tolist() == [2, 2, 1, 1] and not ref["truncated_allowed"].any()
    got = C.model(*args, lengths=lengths, masks=True)
    assert C.check(got, ref, f"walk case, split {split}") and C.identities(got, [len(g) for g in args[2]], 5, args[5], 1)
    assert not got["alive_masks"][:, [0, 3], 0].any() and got["alive_masks"][0, 1, 0] == np.uint64(2 ** 64 - 1)
    assert got["lists"][1, 0].tolist() == ([5 + i for i in range(64)] if split else [1 + i for i in range(64)])   # atom 65 has left


def test_reference_is_the_brute_force():
    """the vectorised reference of persist_cases and the loop of persist64 count the same, on a case with a matrix of cut-offs,
    hysteresis, an origin step and a sample step -- and on the walk case with its truncated centre"""
    for args, ref, _ in (_case("cubic37", "two", (True, C.HYSTERESIS, 3, 1, True)), _case("cubic37", "three", (False, C.HYSTERESIS, 3, 2, True)),
                         _walk(True, C.HYSTERESIS), _walk(False, 1.0, False)):
        brute = R.counts64(*args)
        assert all(np.array_equal(brute[k], ref[k]) for k in C.KEYS)


# the case each fault is held against
FAULT_CASE = {"break_is_cut": ("cubic130", "two", (True, C.HYSTERESIS, 1, 1, True)),
              "all_origins": ("cubic37", "one", (False, 1.0, 1, 1, True)),
              "continuous_is_intermittent": ("triclinic130", "one", (False, 1.0, 1, 1, True)),
              "first_64": ("walk", False), "lost_from_count": ("cubic130", "one", (False, 1.0, 1, 1, True)),
              "transposed": ("walk", True), "sample_step_ignored": ("cubic37", "two", (False, C.HYSTERESIS, 3, 2, True))}


@pytest.mark.parametrize("fault", C.FAULTS)
def test_planted_faults_leave_the_allowance(fault):
    where = FAULT_CASE[fault]
    args, ref, lengths = _walk(where[1], C.HYSTERESIS) if where[0] == "walk" else _case(*where)
    _borderline_first(ref, where)
    assert C.check(C.model(*args, lengths=lengths), ref, f"{where} clean")
    assert not C.check(C.model(*args, lengths=lengths, fault=fault), ref, f"{where} {fault}")


def test_faults_are_the_issue_s_list():
    assert set(FAULT_CASE) == set(C.FAULTS) and len(C.FAULTS) == 7


def test_lags_of():
    assert C.lags_of(12) == [0, 1, 2, 7, 11] and C.lags_of(4) == [0, 1, 2, 3] and C.lags_of(40, 2) == [0, 2, 6, 38] and C.lags_of(4, 2) == [0, 2]


# ---- the result type ---------------------------------------------------------------------------------------------------------
def _result(continuous=True):
    from psa_amd import persistence
    bonds = np.array([[[10, 0], [0, 4]], [[8, 0], [0, 4]], [[6, 0], [0, 2]]], np.uint64)
    alive = np.array([[[10, 0], [0, 4]], [[6, 0], [0, 2]], [[3, 0], [0, 2]]], np.uint64)
    unbroken = np.array([[[10, 0], [0, 4]], [[4, 0], [0, 1]], [[1, 0], [0, 0]]], np.uint64)
    lost = np.zeros((3, 2, 65), np.uint64)
    lost[0, :, 0] = (5, 2)
    lost[1, 0, :3] = (2, 2, 0)
    lost[1, 1, :3] = (0, 2, 0)
    lost[2, 0, :4] = (1, 1, 1, 0)
    out = dict(bonds=bonds, alive=alive, unbroken=unbroken if continuous else np.zeros_like(bonds), lost=lost, truncated=np.zeros((3, 2), np.uint64),
               alive_masks=None, unbroken_masks=None)
    return persistence.result(out, [0, 2, 4], [5, 4, 3], [np.arange(5), np.arange(5, 7)], 0.5, continuous)


def test_result_type():
    import psa_amd
    from psa_amd import BondPersistence, persistence
    assert "BondPersistence" in psa_amd.__all__
    res = _result()
    assert isinstance(res, BondPersistence) and np.array_equal(res.times, [0.0, 1.0, 2.0]) and res.lags.dtype == np.int64
    inter, cont = res.intermittent, res.continuous
    assert inter.dtype == np.float64 and inter.shape == (3, 2, 2) and np.isnan(inter[:, 0, 1]).all() and np.isnan(cont[:, 1, 0]).all()
    assert inter[:, 0, 0].tolist() == [1.0, 0.75, 0.5] and cont[:, 0, 0].tolist() == [1.0, 0.5, 1.0 / 6.0] and cont[:, 1, 1].tolist() == [1.0, 0.25, 0.0]
    cage = res.cage()
    assert cage.shape == (3, 2) and cage[:2].tolist() == [[1.0, 1.0], [0.5, 0.0]] and cage[2, 0] == 1.0 / 3.0 and np.isnan(cage[2, 1])
    assert res.cage(2)[:, 0].tolist() == [1.0, 1.0, 2.0 / 3.0] and res.cage(65)[1].tolist() == [1.0, 1.0]
    for bad in (0, 66, 1.5, True):
        with pytest.raises(ValueError, match="c must be"):
            res.cage(bad)
    pair = res.pair(1, 1)
    assert pair["bonds"].tolist() == [4, 4, 2] and pair["alive"].tolist() == [4, 2, 2] and pair["continuous"].tolist() == [1.0, 0.25, 0.0]
    with pytest.raises(IndexError):
        res.pair(0, 2)
    # 1/e between the lags: continuous (0, 0) falls from 0.5 at 1 ps to 1/6 at 2 ps; (1, 1) from 1 at 0 ps to 0.25 at 1 ps
    level = 1.0 / np.e
    life = res.lifetime()
    assert life.shape == (2, 2) and np.isnan(life[0, 1]) and np.isnan(life[1, 0])
    assert life[0, 0] == pytest.approx(1.0 + (0.5 - level) / (0.5 - 1.0 / 6.0)) and life[1, 1] == pytest.approx((1.0 - level) / 0.75)
    assert np.isnan(res.lifetime("intermittent")[0, 0]) and res.lifetime("intermittent", 0.5)[0, 0] == 2.0
    assert res.lifetime("intermittent", 0.5)[1, 1] == 1.0
    with pytest.raises(ValueError, match="kind"):
        res.lifetime("both")
    bare = _result(False)
    assert bare.unbroken is None and bare.continuous is None and bare.pair(0, 0)["continuous"] is None and bare.alive_masks is None
    with pytest.raises(ValueError, match="not computed"):
        bare.lifetime()
    assert bare.lifetime("intermittent", 0.5)[0, 0] == 2.0
    empty = persistence.result(persistence.empty(1, 2), [0, 1], [0, 0], [np.zeros(0, int)], None, True)
    assert np.isnan(empty.intermittent).all() and np.isnan(empty.cage()).all() and empty.times.tolist() == [0.0, 1.0]


def test_check_lags_and_check_break():
    from psa_amd import persistence
    assert persistence.check_lags([0, 2, 4], 10, 2).tolist() == [0, 2, 4] and persistence.check_lags(3, 10, 1).tolist() == [3]
    for bad, word in (([], "between 1 and 1024"), (list(range(1025)), "between 1 and 1024"), ([0, 2, 2], "ascending"), ([3, 1], "ascending"),
                      ([0, 10], r"\[0, T - 1 = 9\]"), ([-1, 0], r"\[0, T - 1"), ([0, 3], "multiple of sample_step"), ([0.5], "integers"),
                      ([[0, 1]], "integers"), ([True], "integers")):
        with pytest.raises(ValueError, match=word):
            persistence.check_lags(bad, 10, 2 if "multiple" in word else 1)
    rc = np.array([[3.0, 2.0], [2.0, 0.0]])
    assert persistence.check_break(None, rc) is not None and np.array_equal(persistence.check_break(None, rc), rc)
    assert np.array_equal(persistence.check_break(3.5, rc), [[3.5, 3.5], [3.5, 0.0]]) and persistence.check_break(2.5, 2.0) == 2.5
    for bad, word in ((2.5, "at least r_cut"), ([[3.0, 2.5], [2.0, 0.0]], "symmetric"), ([[3.0, 2.0], [2.0, 1.0]], "0 exactly where"),
                      (float("nan"), "finite"), (np.full((3, 3), 4.0), "does not fit"), ([3.0, 3.0], "scalar or"),
                      ([[3.0, 2.0], [2.0, -1.0]], "at least r_cut")):
        with pytest.raises(ValueError, match=word):
            persistence.check_break(bad, rc)

# ---- the calculator's refusals --------------------------------------------------------------------------------------------
def _calculator(pos, box, types=None):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, 1, 1, 1)


def test_calculator_refusals_and_the_empty_result(caplog):
    from psa_amd import BondPersistence, max_pair_radius
    pos = Q.family("cubic37")[0]                                           # 40 frames
    calc = _calculator(pos, Q.CUBIC, (np.arange(37) % 2 + 1).astype(np.int32))
    served = max_pair_radius(Q.CUBIC)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, 2.0]):
        with pytest.raises(ValueError, match="r_cut"):
            calc.calculate_bond_persistence(bad, [0, 1])
    with pytest.raises(ValueError, match="served radius"):
        calc.calculate_bond_persistence(served * 1.001, [0, 1])
    with pytest.raises(ValueError, match="r_break.*served radius"):
        calc.calculate_bond_persistence(3.0, [0, 1], r_break=served * 1.001)
    with pytest.raises(ValueError, match="symmetric"):
        calc.calculate_bond_persistence([[3.0, 2.0], [2.5, 3.0]], [0, 1], basis_atom_types=[1, 2])
    for bad, word in ((2.5, "at least r_cut"), ([[3.0, 4.0], [3.5, 3.0]], "symmetric"), (float("inf"), "finite"), (np.full((3, 3), 4.0), "r_break")):
        with pytest.raises(ValueError, match=word):
            calc.calculate_bond_persistence(3.0, [0, 1], basis_atom_types=[1, 2], r_break=bad)
    with pytest.raises(ValueError, match="0 exactly where"):
        calc.calculate_bond_persistence([[3.0, 3.0], [3.0, 0.0]], [0, 1], basis_atom_types=[1, 2], r_break=np.full((2, 2), 3.5))
    for bad, word in (([], "between 1 and 1024"), ([0, 40], r"T - 1 = 39"), ([2, 1], "ascending"), ([0, 1.5], "integers")):
        with pytest.raises(ValueError, match=word):
            calc.calculate_bond_persistence(3.0, bad)
    with pytest.raises(ValueError, match="multiple of sample_step"):
        calc.calculate_bond_persistence(3.0, [0, 3], sample_step=2)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="sample_step"):
            calc.calculate_bond_persistence(3.0, [0, 1], sample_step=bad)
    with pytest.raises(ValueError, match="origin_step"):
        calc.calculate_bond_persistence(3.0, [0, 1], origin_step=0)
    with pytest.raises(TypeError, match="continuous"):
        calc.calculate_bond_persistence(3.0, [0, 1], continuous=1)
    with pytest.raises(TypeError, match="per_atom"):
        calc.calculate_bond_persistence(3.0, [0, 1], per_atom=1)
    with pytest.raises(ValueError, match="disjoint"):
        calc.calculate_bond_persistence(3.0, [0, 1], basis_atom_indices=[[0, 1], [1, 2]])

    class Sharded:
        nranks = 2
    calc._shard = Sharded()
    with pytest.raises(NotImplementedError, match="sharded calculator"):
        calc.calculate_bond_persistence(3.0, [0, 1])
    empty = _calculator(pos[:0], Q.CUBIC)
    with caplog.at_level(logging.WARNING):
        res = empty.calculate_bond_persistence(3.0, [0, 5], continuous=False)
    assert "0 frames or 0 atoms" in caplog.text
    assert isinstance(res, BondPersistence) and res.bonds.shape == (2, 1, 1) and not res.bonds.any() and res.unbroken is None
    assert res.lost.shape == (2, 1, 65) and res.origins.tolist() == [0, 0] and np.isnan(res.intermittent).all() and res.alive_masks is None


def test_abi_table():
    from psa_amd import _hip
    head = (ROOT / "include" / "psa_hip.h").read_text()
    assert re.search(r"\bint psa_bond_persistence\(", head) and len(_hip.SIGNATURES["psa_bond_persistence"][1]) == 24
    assert int(re.search(r"#define\s+PSA_HIP_ABI_VERSION\s+(\d+)", head).group(1)) == 6
    lib = _hip.load_library()
    assert lib.psa_abi_version() == _hip.ABI_VERSION == 6 and lib.psa_bond_persistence and hasattr(_hip.Engine, "bond_persistence")
    assert _hip.PERSIST_MAX_LAGS == 1024
    ctx = (ROOT / "psa_amd" / "csrc" / "psa_ctx.h").read_text()
    assert re.search(r"PERSIST_MAX_LAGS = 1024;", ctx)
    bufs = re.findall(r"\bd_r[sc]_\w+", re.search(r"psa::DevBuf\s+d_rs_[^;]*;", ctx).group(0))
    assert bufs == ["d_rs_idx", "d_rs_items", "d_rs_part", "d_rs_acc"]      # the call adds no buffer to the context
