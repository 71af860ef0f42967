"""The real-space self dynamics on the GPU (psa_displacement_moments, psa_van_hove_self, psa_debug_unwrap and the two
calculator methods) against the float64 references of tests/msd64.py inside the bars of tests/msd_cases.py: the unwrap
pass (image counts exact, u within its operation count), the moments at every edge of the lag and origin tiles and of the
origin step, the families (far, ballistic, frozen, wrapped against unwrapped), the histogram under its borderline
condition, the small-Q limit of F_s, blockings and reproducibility, the draws, every refusal (a context with a
communicator among them), no trace in later calls.

The worst fraction of each bar a run on an MI355X printed, per family: see DESIGN.md section 7."""
import ctypes as Ct
import functools

import numpy as np
import pytest

import msd64 as R
import msd_cases as M
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = {"cubic": M.CUBIC, "triclinic": M.TRICLINIC}
T = 250


@pytest.fixture(autouse=True)
def _clean(engine):
    reset(engine)
    yield
    reset(engine)


@pytest.fixture(scope="module", autouse=True)
def _forget(engine):
    yield
    engine.invalidate()


def _resident(engine, pos):
    from psa_amd import _hip
    engine.ensure_resident(_hip.SLOT_POSITIONS, pos)


def _calculator(engine, pos, box, types=None, dt=0.002):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, 1, 1, 1).attach(engine=engine)


@functools.lru_cache(maxsize=None)
def _walk(box, n_atoms, n_frames=T, seed=21):
    wrapped, unwrapped, _, _ = M.random_walk(n_atoms, n_frames, seed=seed, box=BOXES[box])
    assert M.tie_free(wrapped, BOXES[box])
    u, n, S = R.unwrap64(wrapped, BOXES[box])
    return dict(pos=wrapped, unwrapped=unwrapped, u=u, n=n, S=S, box=BOXES[box])


def _listing(kind, n_atoms, seed=3):
    """(groups for the engine, or None: all atoms)"""
    if kind == "all":
        return None
    order = np.random.default_rng(seed).permutation(n_atoms).astype(np.int32)
    if kind == "shuffled":
        return [order[: n_atoms - 5]]
    return [order[: n_atoms // 3], np.zeros(0, np.int32), order[n_atoms // 3: n_atoms - 2]]


def _groups(listing, n_atoms):
    return [np.arange(n_atoms)] if listing is None else listing


@functools.lru_cache(maxsize=None)
def _reference(box, n_atoms, kind, n_lags, step, n_frames=T):
    w = _walk(box, n_atoms, n_frames)
    groups = _groups(_listing(kind, n_atoms), n_atoms)
    return R.moments64(w["u"], groups, n_lags, step), M.moments_bar(w["u"], w["S"], groups, n_lags, step)


def _inside(got, ref, bar, what):
    err = np.abs(got - ref)
    frac = np.max(np.divide(err, bar, out=np.zeros_like(err), where=bar > 0))
    print(f"{what}: worst fraction of the bar {frac:.3f}")
    assert np.all(err <= bar), what


# ---- the unwrap pass ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all", "shuffled"])
@pytest.mark.parametrize("n_atoms", [37, 130])
@pytest.mark.parametrize("box", BOXES)
def test_debug_unwrap(engine, box, n_atoms, kind):
    w = _walk(box, n_atoms)
    _resident(engine, w["pos"])
    listing = _listing(kind, n_atoms)
    idx = None if listing is None else listing[0]
    sel = slice(None) if idx is None else idx
    u, img = engine.debug_unwrap(w["box"], idx)
    assert np.abs(w["n"]).max() >= 1 and np.array_equal(img, w["n"][:, sel])
    _inside(u, w["u"][:, sel], M.unwrap_bound(w["S"][:, sel]), f"unwrap {box} {n_atoms} {kind}")
    assert not u[0].any()
    plain, zero = engine.debug_unwrap(w["box"], idx, unwrap=False)
    r = w["pos"].astype(np.float64)
    assert not zero.any() and np.array_equal(plain, (r - r[:1])[:, sel])
    u2, none = engine.debug_unwrap(w["box"], idx, images=False)
    assert none is None and np.array_equal(u2, u)
    # an unwrapped input: no hop anywhere
    _resident(engine, w["unwrapped"])
    uu, m = engine.debug_unwrap(w["box"], idx)
    r = w["unwrapped"].astype(np.float64)
    assert not m.any() and np.array_equal(uu, (r - r[:1])[:, sel])


def test_debug_unwrap_long_in_blocks(engine):
    """T = 1500: 24 frame tiles, and a budget of 7 atoms per block"""
    from psa_amd import _hip
    w = _walk("triclinic", 20, 1500)
    _resident(engine, w["pos"])
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * 1500 * 7 + 100)
    u, img = engine.debug_unwrap(w["box"])
    assert np.array_equal(img, w["n"])
    _inside(u, w["u"], M.unwrap_bound(w["S"]), "unwrap T = 1500")


# ---- the moments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all", "shuffled", "three"])
@pytest.mark.parametrize("n_atoms", [37, 130])
@pytest.mark.parametrize("box", BOXES)
def test_moments_shapes(engine, box, n_atoms, kind):
    w = _walk(box, n_atoms)
    _resident(engine, w["pos"])
    listing = _listing(kind, n_atoms)
    got = engine.displacement_moments(w["box"], 125, listing)
    ref, bar = _reference(box, n_atoms, kind, 125, 1)
    assert got.shape == ref.shape and got.dtype == np.float64
    _inside(got, ref, bar, f"moments {box} {n_atoms} {kind}")
    assert not got[0].any()
    if kind == "three":
        assert not got[:, 1].any() and got[1:, 0].all() and got[1:, 2].all()


@pytest.mark.parametrize("step", [1, 3, 7, 249, 400])
@pytest.mark.parametrize("n_lags", [1, 2, 125, 250])
def test_moments_lags_and_origin_steps(engine, n_lags, step):
    w = _walk("triclinic", 37)
    _resident(engine, w["pos"])
    listing = _listing("three", 37)
    got = engine.displacement_moments(w["box"], n_lags, listing, origin_step=step)
    ref, bar = _reference("triclinic", 37, "three", 250, step)
    _inside(got, ref[:n_lags], bar[:n_lags], f"moments n_lags {n_lags} step {step}")


@pytest.mark.parametrize("step", [1, 2, 5])
@pytest.mark.parametrize("n_lags", [255, 256, 257, 300])
def test_moments_tile_edges(engine, n_lags, step):
    """T = 1500 crosses the lag tile (256 lags) and the origin tiles (1024, 513 and 205 origins at steps 1, 2, 5); the
    last tiles hold lags with fewer origins than their neighbours"""
    from psa_amd import _hip
    assert _hip.MSD_LAGS == 256 and _hip.MSD_WINDOW < 1500
    w = _walk("cubic", 3, 1500)
    _resident(engine, w["pos"])
    got = engine.displacement_moments(w["box"], n_lags, [np.array([2, 0], np.int32), np.array([1], np.int32)], origin_step=step)
    groups = [np.array([2, 0]), np.array([1])]
    ref, bar = R.moments64(w["u"], groups, n_lags, step), M.moments_bar(w["u"], w["S"], groups, n_lags, step)
    _inside(got, ref, bar, f"tile edges n_lags {n_lags} step {step}")


def test_moments_all_lags_of_a_long_run(engine):
    """n_lags = T = 1500: every lane of the last lag tiles runs out of origins at its own place"""
    w = _walk("cubic", 3, 1500)
    _resident(engine, w["pos"])
    got = engine.displacement_moments(w["box"], 1500, None, origin_step=3)
    groups = [np.arange(3)]
    _inside(got, R.moments64(w["u"], groups, 1500, 3), M.moments_bar(w["u"], w["S"], groups, 1500, 3), "n_lags = T = 1500")


# ---- the families ---------------------------------------------------------------------------------------------------
def test_far_family(engine):
    """|u| reaches 1e3 where a lag-1 displacement is 0.03: one atom per group and two origins (0 and T - 16) show single
    samples, where float32 storage of u would miss the bar (tests/test_msd_host.py); then all origins"""
    n_t, n_atoms = 40000, 8
    pos = M.far(n_atoms, n_t, seed=4)
    u, n, S = R.unwrap64(pos, M.CUBIC)
    assert not n.any() and np.abs(u[-1]).max() > 500.0
    _resident(engine, pos)
    groups = [np.array([a], np.int32) for a in range(n_atoms)]
    for n_lags, step in ((16, n_t - 16), (4, 1)):
        got = engine.displacement_moments(M.CUBIC, n_lags, groups, origin_step=step)
        _inside(got, R.moments64(u, groups, n_lags, step), M.moments_bar(u, S, groups, n_lags, step), f"far step {step}")
    same = engine.displacement_moments(M.CUBIC, 4, groups, unwrap=False)
    assert np.array_equal(same, got)


@pytest.mark.parametrize("box", BOXES)
def test_ballistic_and_frozen_closed_forms(engine, box):
    n_atoms = 9
    pos, v = M.ballistic(n_atoms, T, seed=5, box=BOXES[box])
    assert M.tie_free(pos, BOXES[box])
    u, n, S = R.unwrap64(pos, BOXES[box])
    _resident(engine, pos)
    got = engine.displacement_moments(BOXES[box], 100)
    groups = [np.arange(n_atoms)]
    _inside(got, R.moments64(u, groups, 100), M.moments_bar(u, S, groups, 100), f"ballistic {box}")
    t = np.arange(100.0)
    delta = 4 * 2.0 ** -24 * np.abs(np.asarray(BOXES[box], np.float64)).sum()
    for c in range(3):
        assert np.all(np.abs(got[:, 0, c] - np.mean(v[:, c] ** 2) * t ** 2) <= 3 * np.abs(v).max() * t * delta + 2 * delta ** 2)
    assert np.allclose(got[1:, 0, 3], np.mean((v ** 2).sum(1) ** 2) * t[1:] ** 4, rtol=1e-3)
    still = M.frozen(n_atoms, T, seed=6, box=BOXES[box])
    _resident(engine, still)
    assert not engine.displacement_moments(BOXES[box], T).any()
    counts = engine.van_hove_self(BOXES[box], [0, 7, T - 1], 0.25, 16)
    assert np.array_equal(counts[:, 0, 0], [n_atoms * T, n_atoms * (T - 7), n_atoms]) and not counts[:, :, 1:].any()


@pytest.mark.parametrize("box", BOXES)
def test_wrapped_against_unwrapped(engine, box):
    """wrapped input inside the bar of the unwrapped input's reference and the reverse, both widened by what the float32
    rounding of the unwrapped positions moves D by (two positions, 2^-24 of the largest each)"""
    w = _walk(box, 37)
    groups = [np.arange(37)]
    uu, nu, Su = R.unwrap64(w["unwrapped"], w["box"])
    assert not nu.any()
    tol = 2.0 * 2.0 ** -24 * np.abs(w["unwrapped"]).max()
    for pos, (u, S) in ((w["pos"], (uu, Su)), (w["unwrapped"], (w["u"], w["S"]))):
        _resident(engine, pos)
        got = engine.displacement_moments(w["box"], 60)
        ref, bar = R.moments64(u, groups, 60), M.moments_bar(u, S, groups, 60)
        rms = np.sqrt(ref[:, :, :3])
        wide = bar.copy()
        wide[:, :, :3] += 2.0 * rms * tol + tol * tol
        # |R2' - R2| <= dR = 2 sqrt(3 R2) tol + 3 tol^2 per sample, |R2'^2 - R2^2| <= dR (2 R2 + dR), and the means by Hoelder
        wide[:, :, 3] += 4.0 * np.sqrt(3.0) * tol * ref[:, :, 3] ** 0.75 + 18.0 * tol ** 2 * np.sqrt(ref[:, :, 3]) \
            + 12.0 * np.sqrt(3.0) * tol ** 3 * ref[:, :, 3] ** 0.25 + 9.0 * tol ** 4
        assert np.all(np.abs(got - ref) <= wide)


# ---- the self van Hove function -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dr,n_r,overflow", [(2.0, 64, False), (0.25, 64, True), (0.1, 1024, False), (0.3, 1, True), (1000.0, 1, False)])
@pytest.mark.parametrize("box", BOXES)
def test_van_hove(engine, box, dr, n_r, overflow):
    w = _walk(box, 37)
    _resident(engine, w["pos"])
    listing = _listing("three", 37)
    lags = [0, 1, 7, 33, T - 1]
    ref = R.counts64(w["u"], listing, lags, 1, dr, n_r)
    allowed, borderline, total = M.histogram_allowance(w["u"], w["S"], listing, lags, 1, dr, n_r)
    assert borderline <= 1e-3 * total and (ref[:, :, n_r].sum() > 0) == overflow
    got = engine.van_hove_self(w["box"], lags, dr, n_r, listing)
    assert got.dtype == np.uint64 and got.shape == ref.shape
    got = got.astype(np.int64)
    sizes = np.array([g.size for g in listing])
    assert np.array_equal(got.sum(axis=2), np.array([T - t for t in lags])[:, None] * sizes[None, :])     # exact totals
    print(f"van Hove {box} dr {dr} n_r {n_r}: {borderline} borderline of {total}, {int(np.abs(got - ref).sum())} moved")
    assert np.all(np.abs(got - ref) <= allowed)
    assert got[0, :, 1:].sum() == 0                                           # lag 0: everything in bin 0


def test_van_hove_origin_step_and_long_run(engine):
    w = _walk("cubic", 3, 1500)
    _resident(engine, w["pos"])
    groups = [np.arange(3, dtype=np.int32)]
    lags = [0, 5, 700, 1499]
    for step in (1, 7, 2000):
        ref = R.counts64(w["u"], groups, lags, step, 0.5, 100)
        allowed, borderline, total = M.histogram_allowance(w["u"], w["S"], groups, lags, step, 0.5, 100)
        got = engine.van_hove_self(w["box"], lags, 0.5, 100, groups, origin_step=step).astype(np.int64)
        assert np.array_equal(got.sum(axis=2), ref.sum(axis=2)) and np.all(np.abs(got - ref) <= allowed)


# ---- the small-Q limit of F_s -----------------------------------------------------------------------------------------
def test_msd_against_self_correlations(engine):
    """exp(-Q^2 msd / 6) against F_s(Q,t) of the smallest shell of the cubic box (the six vectors +-(1,0,0), ..: |k| = Q =
    2 pi / a exactly).  With y = Q D_c over all samples and axes, F_s = <cos y> and Q^2 msd / 6 = <y^2> / 2: equal for a
    Gaussian population, so the tolerance is the first correction, |alpha_2| (Q^2 msd)^2 / 72 times the exponential, plus
    five standard errors of the two estimates over n_eff = N max(1, (T - t) / t) independent samples -- Var cos y =
    (1 - e^-v)^2 / 2 at most, and the exponential's e^(-v/2) v sqrt(2 / n_eff) / 2 -- plus the 1e-5 of the float32 F_s."""
    n_atoms, n_lags = 400, 20
    pos = M.random_walk(n_atoms, T, seed=31)[0]
    calc = _calculator(engine, pos, M.CUBIC)
    a = float(M.CUBIC[0][0])
    Q = 2.0 * np.pi / a
    r = calc.calculate_msd(lags=n_lags)
    f = calc.calculate_powder_self_correlations(np.array([0.9 * Q, 1.1 * Q]), lags=n_lags)
    assert f.counts[0] == 6
    fs = f.normalized()[:, 0]
    v = Q * Q * r.msd[:, 0] / 3.0
    g = np.exp(-v / 2.0)
    t = np.arange(n_lags)
    n_eff = n_atoms * np.maximum(1.0, (T - t) / np.maximum(t, 1))
    tol = np.nan_to_num(np.abs(r.alpha2[:, 0])) * (Q * Q * r.msd[:, 0]) ** 2 / 72.0 * g \
        + 5.0 * ((1.0 - np.exp(-v)) / np.sqrt(2.0 * n_eff) + g * v * np.sqrt(2.0 / n_eff) / 2.0) + 1e-5
    print("F_s - exp(-Q^2 msd / 6), worst fraction of the tolerance", np.max(np.abs(fs - g) / tol), "at exp", g[-1])
    assert g[-1] < 0.7 and np.all(np.abs(fs - g) <= tol)
    assert np.all(np.abs(np.nan_to_num(r.alpha2[1:, 0])) < 0.1)


# ---- blockings, reproducibility, draws ----------------------------------------------------------------------------------
def test_blocking_and_reproducibility(engine):
    from psa_amd import _hip
    w = _walk("triclinic", 37)
    _resident(engine, w["pos"])
    listing = _listing("three", 37)
    lags = [0, 1, 7, 33, T - 1]
    whole = engine.displacement_moments(w["box"], T, listing, origin_step=3)
    counts = engine.van_hove_self(w["box"], lags, 0.25, 64, listing)
    assert np.array_equal(whole.view(np.uint64), engine.displacement_moments(w["box"], T, listing, origin_step=3).view(np.uint64))
    assert np.array_equal(counts, engine.van_hove_self(w["box"], lags, 0.25, 64, listing))
    for atoms in (1, 5, 11):
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * T * atoms + 7)
        cut = engine.displacement_moments(w["box"], T, listing, origin_step=3)
        a, b = whole.astype(np.float32), cut.astype(np.float32)
        assert np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))
        assert np.all(np.abs(cut - whole) <= 64 * 2.0 ** -53 * np.abs(whole))
        assert np.array_equal(counts, engine.van_hove_self(w["box"], lags, 0.25, 64, listing))
        # the integer reduce (blocks whose groups hold fewer chunks than its eight strands, or none; 2, 34 and 65 columns;
        # five lags x three groups): the three groups -- the middle one empty -- are, group by group, the three
        # one-group calls, and sum_i counts + overflow = samples
        n_r = {1: 1, 5: 33, 11: 64}[atoms]
        three = engine.van_hove_self(w["box"], lags, 0.25, n_r, listing)
        for g, members in enumerate(listing):
            assert np.array_equal(three[:, g:g + 1], engine.van_hove_self(w["box"], lags, 0.25, n_r, [members])), (atoms, g)
        assert np.array_equal(three.sum(axis=2), np.array([T - t for t in lags], np.uint64)[:, None] * np.array([12, 0, 23], np.uint64))


def test_calculator_methods_and_draws(engine):
    from psa_amd import MeanSquareDisplacement, VanHoveSelf, draw_atoms
    w = _walk("triclinic", 130)
    types = (np.arange(130) % 3 + 1).astype(np.int32)
    calc = _calculator(engine, w["pos"], w["box"], types)
    r = calc.calculate_msd(basis_atom_types=[1, 3], lags=40, origin_step=2, max_atoms=10, seed=5)
    want = [draw_atoms(np.flatnonzero(types == s), 10, 5) for s in (1, 3)]
    assert isinstance(r, MeanSquareDisplacement) and all(np.array_equal(a, b) for a, b in zip(r.groups, want))
    assert np.array_equal(r.counts, [10, 10]) and np.array_equal(r.origins, (T - 1 - np.arange(40)) // 2 + 1)
    direct = engine.displacement_moments(np.asarray(w["box"], np.float32).astype(np.float64), 40, want, origin_step=2)
    assert np.array_equal(r.components, direct[:, :, :3]) and np.array_equal(r.fourth, direct[:, :, 3])
    assert np.array_equal(r.msd, direct[:, :, :3].sum(axis=2)) and np.allclose(r.times, 0.002 * np.arange(40))
    ref, bar = R.moments64(w["u"], want, 40, 2), M.moments_bar(w["u"], w["S"], want, 40, 2)
    _inside(direct, ref, bar, "calculator")
    assert np.isnan(r.alpha2[0]).all() and np.allclose(r.alpha2[1:], R.alpha2(direct)[1:])
    assert r.diffusion(fit=(0.01, 0.07)).shape == (2,) and r.diffusion(fit=(0.01, 0.07), per_axis=True).shape == (2, 3)
    assert calc.calculate_msd().msd.shape == (T // 2, 1)
    v = calc.calculate_van_hove([1, 20], 8.0, 32, basis_atom_types=[1, 3], max_atoms=10, seed=5)
    assert isinstance(v, VanHoveSelf) and v.counts.shape == (2, 2, 32) and v.counts.dtype == np.uint64
    assert np.array_equal(v.samples, [[10 * (T - 1)] * 2, [10 * (T - 20)] * 2])
    assert np.array_equal(v.counts.sum(axis=2) + v.overflow, v.samples.astype(np.uint64))
    assert np.allclose((v.radial_density * 0.25).sum(axis=2), 1.0 - v.overflow / v.samples)
    ref = R.counts64(w["u"], want, [1, 20], 1, 0.25, 32)
    allowed, borderline, total = M.histogram_allowance(w["u"], w["S"], want, [1, 20], 1, 0.25, 32)
    assert borderline <= 1e-3 * total
    assert np.all(np.abs(v.counts.astype(np.int64) - ref[:, :, :32]) <= allowed[:, :, :32])
    assert np.all(np.abs(v.overflow.astype(np.int64) - ref[:, :, 32]) <= allowed[:, :, 32])


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    from psa_amd import _hip
    w = _walk("triclinic", 37)
    _resident(engine, w["pos"])
    lib, h = engine._lib, engine._h
    f64p, i32p, i64p, u64p = Ct.POINTER(Ct.c_double), Ct.POINTER(Ct.c_int32), Ct.POINTER(Ct.c_int64), Ct.POINTER(Ct.c_uint64)
    H, inv = R.box64(w["box"])
    H, inv = np.ascontiguousarray(H), np.ascontiguousarray(inv)
    idx = np.arange(10, dtype=np.int32)
    start = np.array([0, 4, 10], np.int64)
    lags = np.array([0, 5], np.int64)
    out, cnt = np.empty((10, 2, 4)), np.empty((2, 2, 9), np.uint64)
    uo = np.empty((T, 10, 3))

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)

    def refused(rc, word):
        msg = lib.psa_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def mom(box=H, binv=inv, ix=idx, st=start, G=2, n_lags=10, step=1, unwrap=1, o=out, nbytes=None):
        return lib.psa_displacement_moments(h, ptr(box, f64p), ptr(binv, f64p), ptr(ix, i32p), ptr(st, i64p), G, n_lags, step, unwrap,
                                            ptr(o, f64p), out.nbytes if nbytes is None else nbytes)

    def vh(box=H, binv=inv, ix=idx, st=start, G=2, lg=lags, n_vh=2, step=1, unwrap=1, dr=0.5, n_r=8, o=cnt, nbytes=None):
        return lib.psa_van_hove_self(h, ptr(box, f64p), ptr(binv, f64p), ptr(ix, i32p), ptr(st, i64p), G, ptr(lg, i64p), n_vh, step,
                                     unwrap, dr, n_r, ptr(o, u64p), cnt.nbytes if nbytes is None else nbytes)

    def dbg(box=H, binv=inv, ix=idx, n_g=10, unwrap=1, o=uo):
        return lib.psa_debug_unwrap(h, ptr(box, f64p), ptr(binv, f64p), ptr(ix, i32p), n_g, unwrap, ptr(o, f64p), None)

    assert mom() == 0 and vh() == 0 and dbg() == 0
    singular = H.copy()
    singular[2] = singular[0] + singular[1]
    for call in (mom, vh, dbg):
        refused(call(box=None), "null")
        refused(call(binv=None), "null")
        refused(call(o=None), "null")
        refused(call(box=singular), "singular")
        refused(call(binv=2.0 * inv), "not the inverse")
        refused(call(box=H * np.nan), "finite")
        refused(call(unwrap=2), "unwrap")
        refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 37], np.int32)), "out of bounds")
        refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1], np.int32)), "out of bounds")
        refused(call(ix=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 3], np.int32)), "twice")
    for call in (mom, vh):
        refused(call(G=0), "groups")
        refused(call(G=9), "groups")
        refused(call(st=None), "null")
        refused(call(st=np.array([1, 4, 10], np.int64)), "must be 0")
        refused(call(st=np.array([0, 6, 4], np.int64)), "ascending")
        refused(call(ix=None), "n_groups must be 1")
        refused(call(step=0), "origin_step")
        refused(call(nbytes=8), "out_bytes")
    refused(mom(n_lags=0), "n_lags")
    refused(mom(n_lags=T + 1), "n_lags")
    refused(vh(n_vh=0), "number of lags")
    refused(vh(n_vh=65), "number of lags")
    refused(vh(lg=None), "null")
    refused(vh(lg=np.array([0, T], np.int64)), "outside [0, T - 1")
    refused(vh(lg=np.array([-1, 3], np.int64)), "outside [0, T - 1")
    for dr in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
        refused(vh(dr=dr), "bin width")
    refused(vh(n_r=0, nbytes=0), "number of bins")
    refused(vh(n_r=1025), "number of bins")
    # one group of all atoms
    assert lib.psa_displacement_moments(h, ptr(H, f64p), ptr(inv, f64p), None, None, 1, 10, 1, 1, ptr(out, f64p), out.nbytes // 2) == 0
    # a budget below one atom names the bytes
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * T - 1)
    for call in (mom, vh, dbg):
        refused(call(), f"need {24 * T} bytes")
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 24 * T)
    assert mom() == 0 and vh() == 0 and dbg() == 0
    # no positions resident
    engine.release(_hip.SLOT_POSITIONS)
    engine.invalidate(_hip.SLOT_POSITIONS)
    for call in (mom, vh, dbg):
        refused(call(), "positions slot holds no array")


def test_sharded_context_is_refused(engine):
    """a context that holds a communicator (one rank is enough) is refused by all three entry points, and serves again
    once the communicator is gone"""
    w = _walk("triclinic", 37)
    _resident(engine, w["pos"])
    lib, h = engine._lib, engine._h
    f64p, i64p, u64p = Ct.POINTER(Ct.c_double), Ct.POINTER(Ct.c_int64), Ct.POINTER(Ct.c_uint64)
    H, inv = (np.ascontiguousarray(a) for a in R.box64(w["box"]))
    hp, ip = H.ctypes.data_as(f64p), inv.ctypes.data_as(f64p)
    lags = np.array([0, 5], np.int64)
    out, cnt, uo = np.empty((10, 1, 4)), np.empty((2, 1, 9), np.uint64), np.empty((T, 37, 3))

    entries = {
        "psa_displacement_moments": lambda: lib.psa_displacement_moments(h, hp, ip, None, None, 1, 10, 1, 1, out.ctypes.data_as(f64p),
                                                                         out.nbytes),
        "psa_van_hove_self": lambda: lib.psa_van_hove_self(h, hp, ip, None, None, 1, lags.ctypes.data_as(i64p), 2, 1, 1, 0.5, 8,
                                                           cnt.ctypes.data_as(u64p), cnt.nbytes),
        "psa_debug_unwrap": lambda: lib.psa_debug_unwrap(h, hp, ip, None, 0, 1, uo.ctypes.data_as(f64p), None),
    }
    assert [call() for call in entries.values()] == [0, 0, 0]
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        got = {name: (call(), lib.psa_last_error().decode()) for name, call in entries.items()}
    finally:
        engine.comm_destroy()
    for name, (rc, msg) in got.items():
        assert rc == -1 and "sharded context" in msg and name in msg, (name, rc, msg)
    assert [call() for call in entries.values()] == [0, 0, 0]


# ---- no trace -----------------------------------------------------------------------------------------------------------
def test_no_trace_in_the_other_entry_points(engine):
    """`calculate`, `calculate_self_spectra` and `calculate_self_correlations` give the bits they gave before the
    displacement calls in between; atom weights and segments set on the context change nothing; the stage times are
    where the header says"""
    from psa_amd import Segments, commensurate_vectors
    w = _walk("cubic", 37)
    calc = _calculator(engine, w["pos"], w["box"])
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    half = commensurate_vectors(w["box"], 1.2, 0.1)[0][:12]
    for _ in range(2):
        calc.calculate(mags, vecs)
    weights = np.linspace(0.5, 2.0, 37).astype(np.float32)
    s = Segments(64, 32, "hann")

    def spectra():
        return (calc.calculate(mags, vecs).sed, calc.calculate_self_spectra(half, segments=s, atom_weights=weights).density,
                calc.calculate_self_correlations(half, lags=50, atom_weights=weights).density)
    before = spectra()
    engine.timings()                                                       # (reset)
    r = calc.calculate_msd(lags=60)
    t = engine.timings()
    assert t["gather"] > 0 and t["transpose"] > 0 and t["epilogue"] > 0 and t["d2h"] > 0 and t["fft"] == 0 and t["project"] == 0
    v = calc.calculate_van_hove([1, 30], 6.0, 48)
    t = engine.timings()
    assert t["gather"] > 0 and t["transpose"] > 0 and t["epilogue"] > 0 and t["d2h"] > 0 and t["fft"] == 0 and t["project"] == 0
    for a, b in zip(before, spectra()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    engine.set_atom_weights(weights)
    engine.set_segments(s)
    assert np.array_equal(calc.calculate_msd(lags=60).msd.view(np.uint64), r.msd.view(np.uint64))
    assert np.array_equal(calc.calculate_van_hove([1, 30], 6.0, 48).counts, v.counts)
