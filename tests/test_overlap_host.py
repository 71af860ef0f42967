"""The self-overlap's reference, allowance and twin on the host (tests/overlap64.py, tests/overlap_cases.py): the NumPy
twin of the stated arithmetic inside the allowance on every family, each planted fault outside it, the borderline share
of the reference alone, chi4 against fractions.Fraction, the Python layer's refusals (the engine never touched), the
all-empty zeros, the result type, the ABI table and the header text."""
import re
from fractions import Fraction

import numpy as np
import pytest

import msd64 as R
import msd_cases as M
import overlap64 as O
import overlap_cases as OC
from conftest import ROOT

BOXES = {"cubic": M.CUBIC, "triclinic": M.TRICLINIC}
T = 250
LAGS = [0, 1, 7, 33, T - 1]


def _walk_case(box="triclinic", n_atoms=37):
    pos = M.random_walk(n_atoms, T, seed=21, box=BOXES[box])[0]
    u, n, S = R.unwrap64(pos, BOXES[box])
    order = np.random.default_rng(3).permutation(n_atoms)
    groups = [order[: n_atoms // 3], np.zeros(0, int), order[n_atoms // 3: n_atoms - 2]]
    return u, S, groups


def _far_case():
    """msd_cases.far cut so that single samples show: 8 atoms, each a group, 40000 frames, two origins (0 and T - 16), where
    |u| reaches 1e3 and a lag-1 displacement is 0.03"""
    n_t, n_atoms = 40000, 8
    u, n, S = R.unwrap64(M.far(n_atoms, n_t, seed=4), M.CUBIC)
    assert not n.any() and np.abs(u[-1]).max() > 500.0
    return u, S, [np.array([a]) for a in range(n_atoms)], list(range(1, 16)), n_t - 16


def _outside(got, ref, allowed):
    return not OC.inside(got, ref, allowed)


# ---- the twin inside the allowance ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", [1.0, 4.0, 12.0])
@pytest.mark.parametrize("box,step", [("cubic", 1), ("triclinic", 1), ("triclinic", 3), ("cubic", 7), ("triclinic", 249), ("cubic", 400)])
def test_twin_inside_the_allowance(box, step, cutoff):
    u, S, groups = _walk_case(box)
    Q, S1, S2 = O.overlap64(u, groups, LAGS, step, cutoff)
    allowed, borderline, total = OC.allowance(u, S, groups, LAGS, step, cutoff)
    assert total == sum(35 * R.n_origins(T, t, step) for t in LAGS) and borderline <= 1e-3 * total
    q, s1, s2 = OC.overlap_model(u, groups, LAGS, step, cutoff)
    a1, a2 = OC.sums_allowance(Q, allowed)
    assert OC.inside(q, Q, allowed) and OC.inside(s1, S1, a1) and OC.inside(s2, S2, a2)
    assert np.array_equal(s1, q.sum(axis=2)) and np.array_equal(s2, (q * q).sum(axis=2))
    assert not Q[:, 1].any() and np.array_equal(Q[0, 0, :R.n_origins(T, 0, step)], np.full(R.n_origins(T, 0, step), 12))
    for j, t in enumerate(LAGS):
        assert not Q[j, :, R.n_origins(T, t, step):].any()


def test_the_random_walk_is_not_degenerate():
    """q falls from 1 to 0 over the lags at a = 4.0 and chi4 is of order 0.2 at lag 7"""
    u, S, _ = _walk_case("cubic", 130)
    Q, S1, S2 = O.overlap64(u, [np.arange(130)], LAGS, 1, 4.0)
    n_o = np.array([T - t for t in LAGS])
    q = S1[:, 0] / (130.0 * n_o)
    assert q[0] == 1.0 and q[1] > 0.99 and 0.3 < q[2] < 0.5 and q[3] < 0.1 and q[4] < 0.05
    assert 0.1 < float(O.chi4_fraction(S1[2, 0], S2[2, 0], n_o[2], 130)) < 0.4


@pytest.mark.parametrize("cutoff", [0.1, 0.2])
def test_twin_inside_the_allowance_far(cutoff):
    u, S, groups, lags, step = _far_case()
    Q = O.overlap64(u, groups, lags, step, cutoff)[0]
    allowed, borderline, total = OC.allowance(u, S, groups, lags, step, cutoff)
    assert total == 8 * 2 * 15 and OC.inside(OC.overlap_model(u, groups, lags, step, cutoff)[0], Q, allowed)
    assert 0.1 < Q.sum() / total < 0.9


@pytest.mark.parametrize("cutoff", [0.5, 0.6])
def test_lattice_walk_is_exact(cutoff):
    pos = OC.lattice_walk(23, T, seed=8)
    u, n, S = R.unwrap64(pos, M.CUBIC)
    assert not n.any() and np.array_equal(u, pos.astype(np.float64) - pos[:1].astype(np.float64))
    groups, lags = [np.arange(0, 23, 2), np.arange(1, 23, 2)], [0, 1, 2, 5]
    Q, S1, S2 = O.overlap64(u, groups, lags, 1, cutoff)
    q, s1, s2 = OC.overlap_model(u, groups, lags, 1, cutoff)
    assert np.array_equal(q, Q) and np.array_equal(s1, S1) and np.array_equal(s2, S2)
    D = R.displacements(u, np.arange(23), 2)
    r2 = (D * D).sum(axis=2)                                                  # exact: multiples of 1/16
    half = r2 == 0.25
    assert half.sum() > 100                                                   # |D| = 0.5 exactly does occur
    counted = (r2 < 0.25).sum() + (half.sum() if cutoff > 0.5 else 0) + ((r2 == 0.3125).sum() if cutoff > 0.5 else 0)
    assert Q[2].sum() == counted                                              # at a = 0.5 the samples at 0.5 are not counted


# ---- the planted faults outside -------------------------------------------------------------------------------------------
def test_fault_le_is_caught_on_the_lattice():
    """only a sample with x = 1 exactly tells <= from <: the lattice family at a = 0.5, where the arithmetic is exact"""
    pos = OC.lattice_walk(23, T, seed=8)
    u = R.unwrap64(pos, M.CUBIC)[0]
    groups, lags = [np.arange(23)], [1, 2]
    Q = O.overlap64(u, groups, lags, 1, 0.5)[0]
    assert np.array_equal(OC.overlap_model(u, groups, lags, 1, 0.5)[0], Q)
    assert not np.array_equal(OC.overlap_model(u, groups, lags, 1, 0.5, fault="le")[0], Q)


@pytest.mark.parametrize("fault", ["o0_neighbour", "u32"])
def test_precision_faults_are_caught_on_the_far_family(fault):
    """the cut-off is put between the reference's and the faulty twin's length of the one sample the fault moves most,
    three quarters of the way to the faulty one; the allowance, from the reference alone, does not cover that sample, and
    the sound twin stays inside"""
    u, S, groups, lags, step = _far_case()
    best = (0.0, 0.0)
    for lag in lags:
        for atoms in groups:
            D = R.displacements(u, atoms, lag, step)
            r_ref = np.sqrt((D * D).sum(axis=2)).ravel()
            gain = np.sqrt(OC._r2(u, atoms, lag, step, fault)).astype(np.float64).ravel() - r_ref
            k = int(np.argmax(np.abs(gain)))
            if abs(gain[k]) > abs(best[0]):
                best = (float(gain[k]), float(r_ref[k]))
    cutoff = best[1] + 0.75 * best[0]
    print(f"{fault}: the fault moves a sample of length {best[1]:.6f} by {best[0]:.2e}")
    Q = O.overlap64(u, groups, lags, step, cutoff)[0]
    allowed = OC.allowance(u, S, groups, lags, step, cutoff)[0]
    assert OC.inside(OC.overlap_model(u, groups, lags, step, cutoff)[0], Q, allowed)
    assert _outside(OC.overlap_model(u, groups, lags, step, cutoff, fault=fault)[0], Q, allowed)


@pytest.mark.parametrize("fault", ["s2_of_mean", "groups_merged", "lag_shift", "origins_of_lag_0"])
def test_structural_faults_are_caught(fault):
    u, S, groups = _walk_case("triclinic")
    Q, S1, S2 = O.overlap64(u, groups, LAGS, 3, 4.0)
    allowed = OC.allowance(u, S, groups, LAGS, 3, 4.0)[0]
    a1, a2 = OC.sums_allowance(Q, allowed)
    q, s1, s2 = OC.overlap_model(u, groups, LAGS, 3, 4.0, fault=fault)
    if fault == "s2_of_mean":
        assert OC.inside(q, Q, allowed) and _outside(s2, S2, a2)
    else:
        grown = np.zeros(q.shape, np.int64)
        grown[:, :, :Q.shape[2]] = Q
        room = np.zeros(q.shape, np.int64)
        room[:, :, :Q.shape[2]] = allowed
        assert _outside(q, grown, room)


# ---- the result type ------------------------------------------------------------------------------------------------------
def test_chi4_is_the_exact_rational():
    from psa_amd import DynamicOverlap
    rng = np.random.default_rng(5)
    n_o = np.array([250, 249, 1, 3], np.int64)
    counts = np.array([37, 0, 2 ** 20], np.int64)
    Q = [[rng.integers(0, max(n, 1) + 1, int(k)) if n else np.zeros(int(k), np.int64) for n in counts] for k in n_o]
    s1 = np.array([[int(q.sum()) for q in row] for row in Q], np.uint64)
    s2 = np.array([[int((q.astype(object) ** 2).sum()) for q in row] for row in Q], np.uint64)
    r = DynamicOverlap(s1, s2, n_o, counts, 1.5, np.array([0, 1, 249, 100]), 0.002 * np.array([0, 1, 249, 100.0]), [np.arange(37)] * 3)
    chi, q = r.chi4, r.q
    assert chi.dtype == np.float64 and chi.shape == (4, 3) and np.all(np.isnan(chi[:, 1])) and np.all(np.isnan(q[:, 1]))
    for j in range(4):
        for g in (0, 2):
            want = Fraction(int(n_o[j]) * int(s2[j, g]) - int(s1[j, g]) ** 2, int(n_o[j]) ** 2 * int(counts[g]))
            assert chi[j, g] == float(want) and want >= 0
            assert q[j, g] == int(s1[j, g]) / (int(n_o[j]) * int(counts[g]))
    assert not chi[2, [0, 2]].any()                                           # one origin: no variance
    # sums beyond 2^53: the numerator is exact where float64 products are not
    big = DynamicOverlap(np.array([[3 * 2 ** 40 + 1]], np.uint64), np.array([[3 * 2 ** 60 + 2 ** 21 + 7]], np.uint64), np.array([3]),
                         np.array([2 ** 21]), 1.0, np.array([1]), np.array([1.0]), [np.arange(1)])
    assert big.chi4[0, 0] == float(Fraction(3 * (3 * 2 ** 60 + 2 ** 21 + 7) - (3 * 2 ** 40 + 1) ** 2, 9 * 2 ** 21))


def test_peak_and_relaxation_time():
    from psa_amd import DynamicOverlap, relaxation_time
    n_o, n_g = 100, 50
    t = np.arange(6.0)
    mean = np.array([50, 40, 25, 10, 5, 0])                                   # Q = mean +- spread on half the origins each
    spread = np.array([0, 2, 6, 3, 1, 0])
    s1 = (n_o * mean)[:, None].astype(np.uint64)
    s2 = (n_o * (mean ** 2 + spread ** 2))[:, None].astype(np.uint64)
    r = DynamicOverlap(s1, s2, np.full(6, n_o), np.array([n_g]), 1.0, np.arange(6), t, [np.arange(n_g)])
    assert np.allclose(r.q[:, 0], mean / n_g) and np.allclose(r.chi4[:, 0], spread ** 2 / n_g)
    t_star, height = r.peak()
    assert t_star.shape == (1,) and t_star[0] == 2.0 and np.isclose(height[0], 36 / 50)
    assert np.array_equal(r.relaxation_time(), relaxation_time(r.q, t)) and 2.0 < r.relaxation_time()[0] < 3.0
    empty = DynamicOverlap(np.zeros((6, 1), np.uint64), np.zeros((6, 1), np.uint64), np.full(6, n_o), np.array([0]), 1.0, np.arange(6), t,
                           [np.zeros(0, int)])
    assert np.isnan(empty.peak()[0][0]) and np.isnan(empty.peak()[1][0]) and np.isnan(empty.relaxation_time()[0])


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def _calculator(n_frames=64, n_atoms=8, shard=None):
    from psa_amd import SEDCalculator, Trajectory
    pos = M.random_walk(max(n_atoms, 1), max(n_frames, 2), seed=1)[0][:n_frames, :n_atoms]
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n_atoms, np.int32), np.arange(n_frames, dtype=np.float32), M.CUBIC,
                    np.diag(M.CUBIC).copy(), np.zeros(3, np.float32), 0.002)
    calc = SEDCalculator(tr, 1, 1, 1)
    calc._shard = shard
    return calc


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was asked for {name}")


def test_python_refusals():
    calc = _calculator()
    calc._engine = _Untouchable()

    def call(**kw):
        return calc.calculate_overlap([1], 2.0, **kw)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="origin_step"):
            call(origin_step=bad)
    with pytest.raises(TypeError, match="unwrap"):
        call(unwrap=1)
    with pytest.raises(TypeError, match="per_origin"):
        call(per_origin=1)
    with pytest.raises(ValueError, match="max_atoms"):
        call(max_atoms=0)
    with pytest.raises(ValueError, match="disjoint"):
        call(basis_atom_indices=[[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="out of bounds"):
        call(basis_atom_indices=[0, 8])
    for bad in ([64], [-1], [1.5]):
        with pytest.raises(ValueError, match="lag_frames"):
            calc.calculate_overlap(bad, 2.0)
    with pytest.raises(ValueError, match="lags"):
        calc.calculate_overlap([1] * 257, 2.0)
    with pytest.raises(ValueError, match="lags"):
        calc.calculate_overlap([], 2.0)
    for bad in (0.0, -1.0, np.inf, np.nan, True, "a"):
        with pytest.raises(ValueError, match="cutoff"):
            calc.calculate_overlap([1], bad)

    class Shard:
        nranks = 2
    with pytest.raises(NotImplementedError):
        _calculator(shard=Shard()).calculate_overlap([1], 2.0)


def test_nothing_to_do_gives_zeros():
    from psa_amd import DynamicOverlap
    calc = _calculator(n_atoms=0)
    calc._engine = _Untouchable()
    r = calc.calculate_overlap([0, 3], 2.0, origin_step=2, per_origin=True)
    assert isinstance(r, DynamicOverlap) and r.sum.shape == (2, 1) and r.sum.dtype == np.uint64 and not r.sum.any()
    assert not r.sum_squares.any() and np.array_equal(r.origins, [32, 31]) and np.array_equal(r.counts, [0])
    assert r.q_origins.shape == (2, 1, 32) and r.q_origins.dtype == np.uint32 and not r.q_origins.any()
    assert np.all(np.isnan(r.chi4)) and np.all(np.isnan(r.q)) and np.allclose(r.times, [0.0, 0.006])
    assert calc.calculate_overlap([1], 2.0).q_origins is None


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_table_and_header_text():
    import psa_amd
    from psa_amd import _hip
    header = (ROOT / "include" / "psa_hip.h").read_text()
    assert _hip.ABI_VERSION == 6 and re.search(r"#define\s+PSA_HIP_ABI_VERSION\s+6\b", header)
    assert len(_hip.SIGNATURES["psa_self_overlap"][1]) == 15
    assert re.search(r"\bint\s+psa_self_overlap\(psa_ctx\* ctx,", header)
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for text in ("Q[j,g,k] = #{ a in g : overlap(a, o_k, tau_j) }", "S2[j,g] = sum_k Q[j,g,k]^2", "a strict inequality",
                 "equals that count bit for bit", "a larger origin_step or fewer lags", "N_g^2 n_o >= 2^63",
                 "[5] unwrap, [6] the count kernel, [4] reduce and moments, [7] device->host"):
        assert text in flat, text
    ctx = (ROOT / "psa_amd" / "csrc" / "psa_ctx.h").read_text()
    assert _hip.OVERLAP_MAX_LAGS == 256 and re.search(r"constexpr int OVERLAP_MAX_LAGS = 256;", ctx)
    assert "DynamicOverlap" in psa_amd.__all__ and hasattr(psa_amd.SEDCalculator, "calculate_overlap")
    assert hasattr(_hip.Engine, "self_overlap")
