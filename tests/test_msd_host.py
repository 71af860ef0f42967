"""The displacement route's references, bounds and twin on the host (tests/msd64.py, tests/msd_cases.py): closed forms
(frozen and ballistic atoms, a Gaussian walk's alpha_2, the origin counts), wrapped against unwrapped references, the
NumPy twin of the stated arithmetic inside the bars, every planted fault outside them, the histogram's borderline share
in the reference alone, the Python layer's refusals and result types, the ABI table and the header text."""
import re

import numpy as np
import pytest

import msd64 as R
import msd_cases as M
from conftest import ROOT

BOXES = {"cubic": M.CUBIC, "triclinic": M.TRICLINIC}


# ---- closed forms ---------------------------------------------------------------------------------------------------
def test_frozen_atoms_give_exact_zeros():
    pos = M.frozen(12, 40, seed=3, box=M.TRICLINIC)
    u, n, S = R.unwrap64(pos, M.TRICLINIC)
    assert not u.any() and not n.any()
    groups = [np.arange(5), np.arange(5, 12)]
    assert not R.moments64(u, groups, 20).any() and not M.moments_bar(u, S, groups, 20).any()
    assert not M.moments_model(M.unwrap_model(pos, M.TRICLINIC)[0], groups, 20).any()
    c = R.counts64(u, groups, [0, 7, 39], 1, 0.25, 16)
    assert np.array_equal(c[:, :, 0], [[5 * 40, 7 * 40], [5 * 33, 7 * 33], [5, 7]]) and not c[:, :, 1:].any()


@pytest.mark.parametrize("box", BOXES)
def test_ballistic_closed_form(box):
    T, N = 120, 9
    pos, v = M.ballistic(N, T, seed=5, box=BOXES[box])
    assert M.tie_free(pos, BOXES[box])
    u, n, _ = R.unwrap64(pos, BOXES[box])
    assert np.abs(n).max() >= 1                                            # the atoms do cross the boundary
    got = R.moments64(u, [np.arange(N)], 60)
    t = np.arange(60.0)
    delta = 4 * 2.0 ** -24 * np.abs(np.asarray(BOXES[box], np.float64)).sum()   # the float32 positions' rounding in D
    vmax = np.abs(v).max()
    for c in range(3):
        assert np.all(np.abs(got[:, 0, c] - np.mean(v[:, c] ** 2) * t ** 2) <= 2 * vmax * t * delta + delta ** 2)
    r = np.sqrt(3.0) * vmax * t
    assert np.all(np.abs(got[:, 0, 3] - np.mean((v ** 2).sum(1) ** 2) * t ** 4) <= 4 * r ** 3 * 2 * delta + 1e-12)
    assert got[0].max() == 0.0


def test_gaussian_walk_alpha2_within_its_statistical_error():
    """independent Gaussian steps: at lag 1 the N n_o samples are independent, and by the delta method with the moments
    of chi^2_3 (E r^2, r^4, r^6, r^8 = 3, 15, 105, 945) Var alpha_2 = 8 / (15 n)"""
    T, N = 60, 400
    pos = M.random_walk(N, T, seed=11)[0]
    a2 = R.alpha2(R.moments64(R.unwrap64(pos, M.CUBIC)[0], [np.arange(N)], 2))
    assert np.isnan(a2[0, 0])
    assert abs(a2[1, 0]) <= 5.0 * np.sqrt(8.0 / (15.0 * N * (T - 1)))


@pytest.mark.parametrize("step", [1, 3, 7, 50, 51, 400])
def test_origin_counts(step):
    from psa_amd.displacements import origin_counts
    T = 50
    got = origin_counts(T, T, step)
    for t in range(T):
        want = len([o for o in range(0, T, step) if o + t <= T - 1])
        assert got[t] == want == R.n_origins(T, t, step) == R.origins(T, t, step).size
    assert np.all(got >= 1)


# ---- wrapped against unwrapped --------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", BOXES)
def test_wrapped_and_unwrapped_references_agree(box):
    T, N = 250, 37
    wrapped, unwrapped, w64, u64 = M.random_walk(N, T, seed=2, box=BOXES[box])
    assert M.tie_free(wrapped, BOXES[box])
    H, inv = R.box64(BOXES[box])
    turns = np.rint((u64 - w64) @ inv).astype(np.int64)
    uw, nw, _ = R.unwrap64(wrapped, BOXES[box])
    assert np.array_equal(nw, turns - turns[:1])                           # the true path, image for image
    uu, nu, _ = R.unwrap64(unwrapped, BOXES[box])
    assert not nu.any()
    assert np.array_equal(uu, R.unwrap64(unwrapped, BOXES[box], unwrap=False)[0])
    tol = 2.0 * 2.0 ** -24 * np.abs(unwrapped).max()                       # the float32 rounding of the unwrapped input
    assert np.abs(uw - uu).max() <= tol
    mw, mu = R.moments64(uw, [np.arange(N)], 40), R.moments64(uu, [np.arange(N)], 40)
    assert np.all(np.abs(mw - mu)[:, :, :3] <= 4 * np.sqrt(mu[:, :, :3].max()) * tol + 1e-12)


# ---- the twin inside the bars, the faults outside ------------------------------------------------------------------
def _far_case():
    """the far family cut so that single samples show: 8 atoms, each a group, 40000 frames, two origins (0 and T - 16)"""
    T, N, n_lags = 40000, 8, 16
    pos = M.far(N, T, seed=4)
    u, n, S = R.unwrap64(pos, M.CUBIC)
    assert not n.any() and np.abs(u[-1]).max() > 500.0
    return u, S, [np.array([a]) for a in range(N)], n_lags, T - n_lags


@pytest.mark.parametrize("box,step", [("cubic", 1), ("triclinic", 1), ("triclinic", 3), ("cubic", 249)])
def test_twin_inside_the_bar(box, step):
    T, N = 250, 37
    pos = M.random_walk(N, T, seed=7, box=BOXES[box])[0]
    u, n, S = R.unwrap64(pos, BOXES[box])
    um, nm = M.unwrap_model(pos, BOXES[box])
    assert np.array_equal(nm, n) and np.all(np.abs(um - u) <= M.unwrap_bound(S))
    groups = [np.arange(0, N, 2), np.arange(1, N, 2), np.zeros(0, int)]
    ref, bar = R.moments64(u, groups, T, step), M.moments_bar(u, S, groups, T, step)
    got = M.moments_model(um, groups, T, step)
    assert np.all(np.abs(got - ref) <= bar) and not got[:, 2].any()
    print("worst fraction of the bar", np.max(np.abs(got - ref)[:, :2] / bar[:, :2], initial=0.0, where=bar[:, :2] > 0))


def test_twin_inside_the_bar_far():
    u, S, groups, n_lags, step = _far_case()
    ref, bar = R.moments64(u, groups, n_lags, step), M.moments_bar(u, S, groups, n_lags, step)
    assert np.all(np.abs(M.moments_model(u, groups, n_lags, step) - ref) <= bar)
    ref1, bar1 = R.moments64(u, groups, 4, 1), M.moments_bar(u, S, groups, 4, 1)
    assert np.all(np.abs(M.moments_model(u, groups, 4, 1) - ref1) <= bar1)


def test_fault_u_as_float32_is_caught():
    u, S, groups, n_lags, step = _far_case()
    ref, bar = R.moments64(u, groups, n_lags, step), M.moments_bar(u, S, groups, n_lags, step)
    assert np.any(np.abs(M.moments_model(u, groups, n_lags, step, fault="u32") - ref) > bar)


def test_fault_float32_fractions_is_caught():
    """x = 12000002 + 4 t in a box of 7: d = 4/7 = 0.571, |d - rint d| = 0.43, m = 1 on every frame; the float32 fractional
    coordinates near 1.7e6 are multiples of 0.125, their differences 0.5 (rint: 0) or 0.625"""
    box = np.diag([7.0, 7.0, 7.0]).astype(np.float32)
    T = 50
    pos = np.zeros((T, 1, 3), np.float32)
    pos[:, 0, 0] = 12000002.0 + 4.0 * np.arange(T)
    assert np.array_equal(pos[:, 0, 0].astype(np.float64), 12000002.0 + 4.0 * np.arange(T)) and M.tie_free(pos, box)
    n = R.unwrap64(pos, box)[1]
    assert np.array_equal(n[:, 0, 0], -np.arange(T))
    assert np.array_equal(M.unwrap_model(pos, box)[1], n)
    assert not np.array_equal(M.unwrap_model(pos, box, fault="frac32")[1], n)


@pytest.mark.parametrize("fault", ["hop_off_by_one", "missing_image"])
def test_unwrap_faults_are_caught(fault):
    T, N = 250, 37
    pos = M.random_walk(N, T, seed=7, box=M.TRICLINIC)[0]
    u, n, S = R.unwrap64(pos, M.TRICLINIC)
    assert np.abs(n[..., 2]).max() >= 1
    uf, _ = M.unwrap_model(pos, M.TRICLINIC, fault=fault)
    assert np.any(np.abs(uf - u) > M.unwrap_bound(S))
    groups = [np.arange(N)]
    ref, bar = R.moments64(u, groups, 60), M.moments_bar(u, S, groups, 60)
    assert np.any(np.abs(M.moments_model(uf, groups, 60) - ref) > bar)


@pytest.mark.parametrize("fault", ["norm_T", "m4_of_means"])
def test_moment_faults_are_caught(fault):
    T, N = 250, 37
    pos = M.random_walk(N, T, seed=7, box=M.TRICLINIC)[0]
    u, n, S = R.unwrap64(pos, M.TRICLINIC)
    groups = [np.arange(N)]
    ref, bar = R.moments64(u, groups, 60, 3), M.moments_bar(u, S, groups, 60, 3)
    assert np.any(np.abs(M.moments_model(u, groups, 60, 3, fault=fault) - ref) > bar)


# ---- the histogram ----------------------------------------------------------------------------------------------------
def _histogram_case(box, dr, n_r):
    T, N = 96, 12
    pos = M.random_walk(N, T, seed=9, box=box)[0]
    u, n, S = R.unwrap64(pos, box)
    groups, lags = [np.arange(7), np.arange(7, 12)], [0, 1, 7, 33, T - 1]
    ref = R.counts64(u, groups, lags, 1, dr, n_r)
    allowed, borderline, total = M.histogram_allowance(u, S, groups, lags, 1, dr, n_r)
    return u, groups, lags, ref, allowed, borderline, total


@pytest.mark.parametrize("dr,n_r,overflow", [(2.0, 64, False), (0.25, 64, True), (0.05, 1024, False), (0.3, 1, True)])
def test_histogram_twin_and_borderline_share(dr, n_r, overflow):
    u, groups, lags, ref, allowed, borderline, total = _histogram_case(M.TRICLINIC, dr, n_r)
    T = u.shape[0]
    assert total == sum(12 * (T - t) for t in lags) and borderline <= 1e-3 * total
    assert np.array_equal(ref.sum(axis=2), [[7 * (T - t), 5 * (T - t)] for t in lags])
    assert (ref[:, :, n_r].sum() > 0) == overflow
    got = M.histogram_model(u, groups, lags, 1, dr, n_r)
    assert np.array_equal(got.sum(axis=2), ref.sum(axis=2)) and np.all(np.abs(got - ref) <= allowed)
    assert np.any(np.abs(M.histogram_model(u, groups, lags, 1, dr, n_r, fault="bin_shift") - ref) > allowed)


# ---- the Python layer -------------------------------------------------------------------------------------------------
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
    for bad in (65, 0, 2.5, True):
        with pytest.raises(ValueError, match="lags"):
            calc.calculate_msd(lags=bad)
    for call in (calc.calculate_msd, lambda **kw: calc.calculate_van_hove([1], 2.0, **kw)):
        for bad in (0, -1, 1.5, True):
            with pytest.raises(ValueError, match="origin_step"):
                call(origin_step=bad)
        with pytest.raises(TypeError, match="unwrap"):
            call(unwrap=1)
        with pytest.raises(ValueError, match="max_atoms"):
            call(max_atoms=0)
        with pytest.raises(ValueError, match="disjoint"):
            call(basis_atom_indices=[[0, 1], [1, 2]])
        with pytest.raises(ValueError, match="out of bounds"):
            call(basis_atom_indices=[0, 8])
    with pytest.raises(ValueError, match="lag_frames"):
        calc.calculate_van_hove([64], 2.0)
    with pytest.raises(ValueError, match="lag_frames"):
        calc.calculate_van_hove([-1], 2.0)
    with pytest.raises(ValueError, match="lag_frames"):
        calc.calculate_van_hove([1.5], 2.0)
    with pytest.raises(ValueError, match="lags"):
        calc.calculate_van_hove(list(range(64)) + [1], 2.0)
    with pytest.raises(ValueError, match="lags"):
        calc.calculate_van_hove([], 2.0)
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError, match="n_r"):
            calc.calculate_van_hove([1], 2.0, n_r=bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="r_max"):
            calc.calculate_van_hove([1], bad)

    class Shard:
        nranks = 2
    with pytest.raises(NotImplementedError):
        _calculator(shard=Shard()).calculate_msd()
    with pytest.raises(NotImplementedError):
        _calculator(shard=Shard()).calculate_van_hove([1], 2.0)


def test_nothing_to_do_gives_zeros():
    calc = _calculator(n_atoms=0)
    calc._engine = _Untouchable()
    r = calc.calculate_msd(lags=5)
    assert r.msd.shape == (5, 1) and r.components.shape == (5, 1, 3) and not r.msd.any() and np.all(np.isnan(r.alpha2))
    v = calc.calculate_van_hove([0, 3], 2.0, n_r=10)
    assert v.counts.shape == (2, 1, 10) and v.counts.dtype == np.uint64 and v.overflow.shape == (2, 1) and not v.counts.any()
    assert v.radial_density.shape == (2, 1, 10) and not v.radial_density.any()


def test_result_classes():
    from psa_amd import MeanSquareDisplacement, VanHoveSelf
    t = 0.5 * np.arange(20.0)
    comp = np.stack([2.0 * t, 4.0 * t, 6.0 * t], axis=1)[:, None, :] + 0.25
    r = MeanSquareDisplacement(comp.sum(axis=2), comp, np.zeros((20, 1)), np.zeros((20, 1)), t, np.arange(20, 0, -1), [np.arange(3)],
                               np.array([3]), 0.5)
    assert np.allclose(r.diffusion(fit=(1.0, 8.0)), [2.0]) and np.allclose(r.diffusion(fit=(1.0, 8.0), per_axis=True), [[1.0, 2.0, 3.0]])
    with pytest.raises(ValueError, match="fewer than two"):
        r.diffusion(fit=(1.1, 1.4))
    edges = 0.5 * np.arange(5.0)
    counts = np.array([[[1, 2, 3, 2]]], np.uint64)
    v = VanHoveSelf(counts, np.array([[2]], np.uint64), edges, 0.5 * (edges[1:] + edges[:-1]), np.array([[10]]), np.array([3]),
                    np.array([1.5]), [np.arange(2)], 0.5)
    assert np.isclose((v.radial_density * 0.5).sum(), 1.0 - 2 / 10)
    assert np.allclose(v.g_s[0, 0] * (4 * np.pi / 3) * (edges[1:] ** 3 - edges[:-1] ** 3), counts[0, 0] / 10.0)


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_abi_table_and_header_text():
    from psa_amd import _hip
    header = (ROOT / "include" / "psa_hip.h").read_text()
    assert _hip.ABI_VERSION == 6 and re.search(r"#define\s+PSA_HIP_ABI_VERSION\s+6\b", header)
    for name, n_args in (("psa_displacement_moments", 11), ("psa_van_hove_self", 14), ("psa_debug_unwrap", 8)):
        assert len(_hip.SIGNATURES[name][1]) == n_args
        assert re.search(r"\bint\s+%s\(psa_ctx\* ctx," % name, header)
    flat = re.sub(r"\s*\n \*\s*", " ", header)                             # the comments' line breaks folded
    for text in ("m[t,a,j] = rint(d_j)", "n_o(t) = (T-1-t) / s + 1", "alpha_2 = 3 M4 / (5 msd^2) - 1", "bin = x < n_r ? (int) floorf(x) : n_r",
                 "[5] unwrap, [6] the moments kernel, [4] reduce and finish, [7] device->host", "a budget below one atom",
                 "half a box length"):
        assert text in flat, text
    assert (_hip.MSD_LAGS, _hip.MSD_ORIGINS, _hip.MSD_WINDOW, _hip.MSD_MAX_GROUPS, _hip.MSD_MAX_BINS, _hip.MSD_MAX_VH_LAGS) == \
        (256, 1024, 1280, 8, 1024, 64)
    ctx = (ROOT / "psa_amd" / "csrc" / "psa_ctx.h").read_text()
    for name in ("MSD_LAGS", "MSD_ORIGINS", "MSD_WINDOW", "MSD_MAX_GROUPS", "MSD_MAX_BINS", "MSD_MAX_VH_LAGS", "MSD_UNWRAP_FRAMES",
                 "MSD_UNWRAP_ATOMS"):
        assert re.search(r"constexpr int %s = %d;" % (name, getattr(_hip, name)), ctx), name
