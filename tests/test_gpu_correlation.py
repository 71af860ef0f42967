"""The time correlations on the GPU (psa_lattice_correlations, psa_self_correlations and the four calculator methods): the
back-transform alone, element by element inside the operation-count bar of tests/correlation_cases.py at every edge of its
two layouts, with a table index that passes 2^31; the calculator methods against the time-domain float64 reference
(tests/correlation64.py) on the explicit full sphere of both boxes, per vector and as shells; the closed forms (ballistic
and frozen atoms), wrapped against unwrapped coordinates; the draws; the sum rules; blockings; a smaller transform length
after a larger one against a fresh context; every refusal; no trace in a later calculation.

The worst fraction of the end-to-end bar 1e-5 F64[0] L / (L - t) a run on an MI355X printed, per family: see DESIGN.md
section 7."""
import ctypes as Ct

import numpy as np
import pytest

import correlation64 as R
import correlation_cases as CC
import lattice64 as L64
import self_cases as S
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = {"cubic": S.CUBIC, "triclinic": S.TRICLINIC}
T = 250
EDGES = np.array([0.05, 0.2, 0.45, 0.65, 0.85, 1.0, 1.15])                # those of test_gpu_lattice.py: the first shell is empty
N0 = np.array([2, -1, 3], np.int32)
FIELDS = ("density", "longitudinal", "transverse")


@pytest.fixture(autouse=True)
def _clean(engine):
    reset(engine)
    yield
    reset(engine)


@pytest.fixture(scope="module", autouse=True)
def _forget(engine):
    yield
    engine.invalidate()


def _calculator(engine, pos, box, vel=None, dt=0.002, cells=(1, 1, 1)):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos) if vel is None else vel, np.ones(n, np.int32), np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, *cells).attach(engine=engine)


def _segments(case):
    """(Segments or None, L, H, n_lags) of a SEGMENT_CASES key"""
    from psa_amd import Segments
    t, L, H, n_lags = CC.SEGMENT_CASES[case]
    assert t == T
    return (None if L == T else Segments(L, H, "boxcar")), L, H, n_lags


def _shells(box):
    from psa_amd import commensurate_vectors, shell_bins
    half, _, q = commensurate_vectors(box, EDGES[-1], EDGES[0])
    b, sel, avail, used = shell_bins(q, EDGES)
    half, b, q = half[sel], b[sel], q[sel]
    assert 100 <= half.shape[0] <= 300 and avail[0] == 0 and np.all(avail[1:] > 0)
    return half, b, q, avail


# ---- the back-transform alone ------------------------------------------------------------------------------------------
# (P, cols, n_lags, fields, float32 input); n_lags = P is the largest legal (L = P); the columns form begins at 64 columns
TRANSFORM_CASES = [
    (1, 1, 1, 1, False), (1, 65, 1, 3, True),
    (2, 1, 2, 1, True), (2, 64, 2, 3, False), (2, 257, 1, 1, False),
    (64, 63, 33, 3, False), (64, 64, 64, 1, True), (64, 65, 1, 1, False), (64, 257, 2, 3, True), (64, 1, 33, 3, True),
    (96, 1, 96, 3, False), (96, 257, 49, 1, False), (96, 63, 2, 1, True), (96, 64, 96, 3, True), (96, 65, 1, 3, False),
    (8192, 1, 4097, 1, False), (8192, 65, 4097, 1, True), (8192, 257, 2, 3, False), (8192, 1, 8192, 1, True),
    (8192, 64, 1, 1, False), (8192, 63, 2, 3, True),
]


@pytest.mark.parametrize("case", TRANSFORM_CASES, ids=lambda c: f"P{c[0]}_cols{c[1]}_lags{c[2]}_f{c[3]}_{'f32' if c[4] else 'f64'}")
def test_back_transform_within_the_operation_count(engine, case):
    P, cols, n_lags, fields, f32 = case
    L, n_seg = (P, 1) if n_lags == P else (n_lags + 5, 3)
    X = np.random.default_rng(P + cols).uniform(0.0, 1e3, (fields, P, cols))
    X[:, ::3] *= 1e-3
    if f32:
        X = X.astype(np.float32).astype(np.float64)                        # what the device holds
    got = engine.debug_correlation_transform(X, L, n_seg, n_lags, as_float32=f32)
    assert got.shape == (fields, n_lags, cols) and got.dtype == np.float32
    ref = CC.transform64(X, L, n_seg, n_lags)
    bar = CC.transform_bar(X, L, n_seg, n_lags, ref)
    frac = np.abs(got.astype(np.float64) - ref) / bar
    print(f"{case}: worst fraction of the bar {frac.max():.3f}")
    assert frac.max() <= 1.0
    again = engine.debug_correlation_transform(X, L, n_seg, n_lags, as_float32=f32)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_back_transform_table_index_past_2_31(engine):
    """P = 65536, 40000 lags: o t reaches 2.6e9.  Single lines, so the reference is the closed form cos(2 pi o0 t / P) / P"""
    P, n_lags = 65536, 40000
    X = np.zeros((1, P, 2))
    X[0, 65535, 0] = 1.0
    X[0, 1, 1] = X[0, 40000, 1] = 1.0
    ref = np.stack([CC.single_line(65535, P, n_lags), CC.single_line(1, P, n_lags) + CC.single_line(40000, P, n_lags)], axis=1)
    ref = (ref / CC.origins(n_lags, 1, n_lags)[:, None])[None]
    assert 65535 * (n_lags - 1) > 2 ** 31
    for f32 in (False, True):
        got = engine.debug_correlation_transform(X, n_lags, 1, n_lags, as_float32=f32)
        frac = np.abs(got.astype(np.float64) - ref) / CC.transform_bar(X, n_lags, 1, n_lags, ref)
        print(f"float32 input {f32}: worst fraction of the bar {frac.max():.3f}")
        assert frac.max() <= 1.0


# ---- the coherent fields against float64 ------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(BOXES))
def wave(request):
    """T = 250, N = 130, the half space of |k| < 1.15 in 6 shells of which the first is empty, a travelling wave on one of its
    vectors, sqrt(mass) weights; the float64 projections of the explicit full sphere"""
    box = BOXES[request.param]
    inv = S.inverse(box)
    half, b, q, avail = _shells(box)
    pos, vel = S.C.travelling_wave(130, T, box, half[np.flatnonzero(b == 2)[3]], bin0=20)
    w = S.weights("sqrt_mass", 130, seed=23)
    full, b_full = np.concatenate([half, -half]), np.concatenate([b, b])
    return dict(name=request.param, box=box, inv=inv, half=half, bins=b, q=q, avail=avail, pos=pos, vel=vel, w=w, full=full,
                b_full=b_full, q_full=L64.project64(pos, vel, full, inv, None, w, True))


def _check_fields(label, got, ref, L, bar=CC.PARITY):
    worst = {}
    for name, g, r in zip(FIELDS, got, ref):
        if r is None:
            assert g is None
            continue
        assert g.shape == r.shape and g.dtype == np.float32, (name, g.shape, r.shape)
        worst[name] = CC.worst_fraction(g, r, L, bar)
    print(f"{label}: worst fraction of the bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (label, worst)


@pytest.mark.parametrize("case", list(CC.SEGMENT_CASES))
def test_coherent_parity_float64_on_the_full_sphere(engine, wave, case):
    from psa_amd import PowderTimeCorrelations, TimeCorrelations
    s, L, H, n_lags = _segments(case)
    n_seg = 1 + (T - L) // H
    calc = _calculator(engine, wave["pos"], wave["box"], wave["vel"])
    ref = R.fields64(wave["q_full"], wave["full"], wave["inv"], L, H, n_lags)
    per = calc.calculate_lattice_correlations(wave["full"], atom_weights=wave["w"], lags=n_lags, segments=s)
    assert isinstance(per, TimeCorrelations) and per.density.shape == (n_lags, wave["full"].shape[0])
    np.testing.assert_allclose(per.times, np.arange(n_lags) * 0.002)
    np.testing.assert_array_equal(per.origins, n_seg * (L - np.arange(n_lags)))
    np.testing.assert_allclose(per.k_vectors, L64.lattice_k(wave["full"], wave["inv"]), rtol=0, atol=1e-13)
    assert np.array_equal(per.atoms, np.arange(130))
    got = (per.density, per.longitudinal, per.transverse)
    # every field has F[0] > 0 -- but for the vectors along y of the cubic box, which are perpendicular to the wave's
    # polarisation (0.6, 0, 0.8): their longitudinal field is exactly zero in the reference and on the device
    for g, r in zip(got, ref):
        assert np.array_equal(g[0] > 0, r[0] > 0) and np.all(g[0] >= 0) and np.count_nonzero(r[0] > 0) >= r.shape[1] - 6
    assert np.all(got[0][0] > 0) and np.all(got[2][0] > 0)
    _check_fields(f"{wave['name']} {case}: per vector", got, ref, L)
    # the powder average against the mean over the explicit full sphere, nothing folded
    pw = calc.calculate_powder_correlations(EDGES, atom_weights=wave["w"], lags=n_lags, segments=s)
    assert isinstance(pw, PowderTimeCorrelations) and pw.density.shape == (n_lags, 6)
    got_pw = (pw.density, pw.longitudinal, pw.transverse)
    _check_fields(f"{wave['name']} {case}: shells", got_pw, R.shell_mean64(ref, wave["b_full"], 6), L)
    host = R.shell_mean64([g.astype(np.float64) for g in got], wave["b_full"], 6)
    _check_fields(f"{wave['name']} {case}: shells against the per-vector form averaged on the host", got_pw, host, L, CC.SHELL)
    for g in got_pw:
        assert not g[:, 0].any() and np.all(g[0, 1:] > 0)                  # the empty shell; F[0] > 0 elsewhere
    np.testing.assert_array_equal(pw.counts, 2 * np.bincount(wave["bins"], minlength=6))
    np.testing.assert_array_equal(pw.available, 2 * wave["avail"])
    assert np.array_equal(pw.indices, wave["half"]) and np.array_equal(pw.bin_index, wave["bins"])
    np.testing.assert_array_equal(pw.origins, per.origins)
    # the density alone: the same bits as the first field of the full call (its series and its passes do not depend on NC)
    only = calc.calculate_lattice_correlations(wave["full"][:40], atom_weights=wave["w"], lags=n_lags, segments=s, currents=False)
    assert only.longitudinal is None and only.transverse is None
    _check_fields(f"{wave['name']} {case}: density only", (only.density,), (ref[0][:, :40],), L)


def test_coherent_shuffled_list_signed_weights_and_the_draw(engine, wave):
    s, L, H, n_lags = _segments("63_31_40")
    w = S.weights("signed", 130, seed=6)
    idx = np.random.default_rng(5).permutation(130)[:77]
    calc = _calculator(engine, wave["pos"], wave["box"], wave["vel"])
    ref = R.lattice_correlations64(wave["pos"], wave["vel"], wave["full"], wave["inv"], np.sort(idx), w, True, L, H, n_lags)
    per = calc.calculate_lattice_correlations(wave["full"], basis_atom_indices=idx, atom_weights=w, lags=n_lags, segments=s)
    assert per.weight_norm == pytest.approx(float(np.sum(w[idx].astype(np.float64) ** 2)))
    _check_fields(f"{wave['name']}: 77 shuffled atoms, signed weights", (per.density, per.longitudinal, per.transverse), ref, L)
    # max_per_bin agrees with the explicit subset
    pw = calc.calculate_powder_correlations(EDGES, basis_atom_indices=idx, atom_weights=w, lags=n_lags, segments=s, max_per_bin=9, seed=3)
    np.testing.assert_array_equal(pw.counts, 2 * np.minimum(wave["avail"], 9))
    pos_in_full = {tuple(v): i for i, v in enumerate(wave["full"])}
    cols = np.array([pos_in_full[tuple(v)] for v in np.concatenate([pw.indices, -pw.indices])])
    want = R.shell_mean64([r[:, cols] for r in ref], np.concatenate([pw.bin_index, pw.bin_index]), 6)
    _check_fields(f"{wave['name']}: max_per_bin = 9", (pw.density, pw.longitudinal, pw.transverse), want, L)
    # default lags: L // 2
    assert calc.calculate_lattice_correlations(wave["half"][:3], segments=s, currents=False).density.shape == (L // 2, 3)


# ---- the self part against float64 ------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(BOXES))
def walk(request):
    """T = 250, 37 atoms of family (c), the same shells, signed weights; the float64 reference on the explicit full sphere,
    once per segment case"""
    box = BOXES[request.param]
    inv = S.inverse(box)
    half, b, q, avail = _shells(box)
    wrapped, unwrapped, _, _ = S.random_walk(37, T, seed=31, box=box)
    w = S.weights("signed", 37, seed=23)
    full, b_full = np.concatenate([half, -half]), np.concatenate([b, b])
    cache = {}

    def ref(case, idx=None):
        key = (case, None if idx is None else tuple(idx))
        if key not in cache:
            _, L, H, n_lags = CC.SEGMENT_CASES[case]
            cache[key] = R.self_correlations64(wrapped, full, inv, idx, w, L, H, n_lags)
        return cache[key]
    return dict(name=request.param, box=box, inv=inv, half=half, bins=b, avail=avail, pos=wrapped, unwrapped=unwrapped, w=w,
                full=full, b_full=b_full, ref=ref, norm=float(np.sum(w.astype(np.float64) ** 2)))


@pytest.mark.parametrize("case", list(CC.SEGMENT_CASES))
def test_self_parity_float64_on_the_full_sphere(engine, walk, case):
    from psa_amd import PowderTimeCorrelations, TimeCorrelations
    s, L, H, n_lags = _segments(case)
    calc = _calculator(engine, walk["pos"], walk["box"])
    ref = walk["ref"](case)
    per = calc.calculate_self_correlations(walk["full"], atom_weights=walk["w"], lags=n_lags, segments=s)
    assert isinstance(per, TimeCorrelations) and per.longitudinal is None and per.transverse is None
    assert per.weight_norm == pytest.approx(walk["norm"])
    _check_fields(f"{walk['name']} {case}: self, per vector", (per.density,), (ref,), L)
    # F_s(n, 0) = sum_a w_a^2 for every vector
    assert np.all(np.abs(per.density[0].astype(np.float64) - walk["norm"]) <= 1e-6 * walk["norm"])
    pw = calc.calculate_powder_self_correlations(EDGES, atom_weights=walk["w"], lags=n_lags, segments=s)
    assert isinstance(pw, PowderTimeCorrelations) and pw.density.shape == (n_lags, 6) and pw.longitudinal is None
    _check_fields(f"{walk['name']} {case}: self, shells", (pw.density,), R.shell_mean64([ref], walk["b_full"], 6), L)
    host = R.shell_mean64([per.density.astype(np.float64)], walk["b_full"], 6)
    _check_fields(f"{walk['name']} {case}: self, shells against the per-vector form averaged on the host", (pw.density,), host, L, CC.SHELL)
    assert not pw.density[:, 0].any()
    np.testing.assert_array_equal(pw.counts, 2 * np.bincount(walk["bins"], minlength=6))
    if case == "64_32_64":                                                  # the relaxation time of every shell, on the host
        from psa_amd import relaxation_time
        tau = relaxation_time(pw.density, pw.times)
        want = relaxation_time(R.shell_mean64([ref], walk["b_full"], 6)[0], pw.times)
        assert np.isnan(tau[0]) and np.all(np.isfinite(tau[1:]))
        np.testing.assert_allclose(tau[1:], want[1:], rtol=1e-3)


@pytest.mark.parametrize("box_name", list(BOXES))
def test_ballistic_and_frozen_closed_forms(engine, box_name):
    """family (b): n0.s_a advances by b_a / T turns per frame, so F_s[t] = sum_a w_a^2 cos(2 pi b_a t / T) at every lag, with
    no leakage; frozen atoms: F_s[t] = sum_a w_a^2 at every lag"""
    box = BOXES[box_name]
    pos, b = S.ballistic(100, T, seed=7, n0=N0, box=box)
    w = S.weights("sqrt_mass", 100, seed=8).astype(np.float64)
    ind = np.stack([N0, -N0]).astype(np.int32)
    t = np.arange(125)
    want = np.sum(w[None, :] ** 2 * np.cos(2 * np.pi * b[None, :] * t[:, None] / T), axis=1)
    per = _calculator(engine, pos, box).calculate_self_correlations(ind, atom_weights=w.astype(np.float32))
    assert per.density.shape == (125, 2)
    want2 = np.stack([want, want], axis=1)
    print(f"ballistic {box_name}: worst fraction of the bar {CC.worst_fraction(per.density, want2, T):.3f}")
    assert np.all(np.abs(per.density - want2) <= CC.end_to_end_bar(want2, T))
    frozen = S.frozen(37, T, seed=5, box=box)
    ws = S.weights("signed", 37, seed=6)
    ind = np.concatenate([S.C.mixed_indices(4, seed=4), S.C.corner_indices()[:2]])
    from psa_amd import Segments
    for s, L, n_lags in ((None, T, 125), (Segments(64, 32, "boxcar"), 64, 64)):
        got = _calculator(engine, frozen, box).calculate_self_correlations(ind, atom_weights=ws, lags=n_lags, segments=s).density
        flat = np.full(got.shape, float(np.sum(ws.astype(np.float64) ** 2)))
        print(f"frozen {box_name} L = {L}: worst fraction of the bar {CC.worst_fraction(got, flat, L):.3f}")
        assert np.all(np.abs(got - flat) <= CC.end_to_end_bar(flat, L))


def test_wrapped_against_unwrapped(engine, walk):
    s, L, H, n_lags = _segments("64_32_64")
    ind = walk["full"][::7]
    ref_w = walk["ref"]("64_32_64")[:, ::7]
    ref_u = R.self_correlations64(walk["unwrapped"], ind, walk["inv"], None, walk["w"], L, H, n_lags)
    kw = dict(atom_weights=walk["w"], lags=n_lags, segments=s)
    got_w = _calculator(engine, walk["pos"], walk["box"]).calculate_self_correlations(ind, **kw).density
    got_u = _calculator(engine, walk["unwrapped"], walk["box"]).calculate_self_correlations(ind, **kw).density
    _check_fields("wrapped against the unwrapped reference", (got_w,), (ref_u,), L)
    _check_fields("unwrapped against the wrapped reference", (got_u,), (ref_w,), L)


def test_max_atoms_agrees_with_the_explicit_subset(engine, walk):
    s, L, H, n_lags = _segments("63_31_40")
    calc = _calculator(engine, walk["pos"], walk["box"])
    some = calc.calculate_self_correlations(walk["full"], atom_weights=walk["w"], lags=n_lags, segments=s, max_atoms=21, seed=0)
    assert some.atoms.shape == (21,) and np.unique(some.atoms).size == 21
    assert some.weight_norm == pytest.approx(float(np.sum(walk["w"][some.atoms].astype(np.float64) ** 2)))
    ref = walk["ref"]("63_31_40", idx=some.atoms)
    _check_fields("max_atoms = 21", (some.density,), (ref,), L)
    explicit = calc.calculate_self_correlations(walk["full"], basis_atom_indices=some.atoms, atom_weights=walk["w"], lags=n_lags, segments=s)
    assert np.array_equal(some.density.view(np.uint32), explicit.density.view(np.uint32))
    pw = calc.calculate_powder_self_correlations(EDGES, atom_weights=walk["w"], lags=n_lags, segments=s, max_atoms=21, max_per_bin=9, seed=0)
    assert np.array_equal(pw.atoms, some.atoms)
    np.testing.assert_array_equal(pw.counts, 2 * np.minimum(walk["avail"], 9))
    pos_in_full = {tuple(v): i for i, v in enumerate(walk["full"])}
    cols = np.array([pos_in_full[tuple(v)] for v in np.concatenate([pw.indices, -pw.indices])])
    want = R.shell_mean64([ref[:, cols]], np.concatenate([pw.bin_index, pw.bin_index]), 6)
    _check_fields("max_atoms = 21, max_per_bin = 9", (pw.density,), want, L)


# ---- sum rules -----------------------------------------------------------------------------------------------------------
def test_lag_zero_is_the_sum_of_the_spectrum(engine, wave, walk):
    """Parseval: with the same boxcar segments F[0] = sum_o of the matching field of the spectra, to 1e-5"""
    from psa_amd import Segments
    s = Segments(64, 32, "boxcar")
    calc = _calculator(engine, wave["pos"], wave["box"], wave["vel"])
    cor = calc.calculate_lattice_correlations(wave["half"], atom_weights=wave["w"], lags=1, segments=s)
    spe = calc.calculate_lattice_spectra(wave["half"], atom_weights=wave["w"], segments=s)
    for name in FIELDS:
        a, b = getattr(cor, name)[0].astype(np.float64), getattr(spe, name).astype(np.float64).sum(0)
        print(f"{name}: F[0] against the sum of the spectrum, largest deviation {np.max(np.abs(a - b)[b > 0] / b[b > 0]):.2e}")
        assert np.all(np.abs(a - b) <= 1e-5 * b)
    pc = calc.calculate_powder_correlations(EDGES, atom_weights=wave["w"], lags=1, segments=s)
    ps = calc.calculate_powder_spectra(EDGES, atom_weights=wave["w"], segments=s)
    for name in FIELDS:
        a, b = getattr(pc, name)[0].astype(np.float64), getattr(ps, name).astype(np.float64).sum(0)
        assert np.all(np.abs(a - b) <= 1e-5 * b)
    calc = _calculator(engine, walk["pos"], walk["box"])
    a = calc.calculate_self_correlations(walk["half"], atom_weights=walk["w"], lags=1, segments=s).density[0].astype(np.float64)
    b = calc.calculate_self_spectra(walk["half"], atom_weights=walk["w"], segments=s).density.astype(np.float64).sum(0)
    assert np.all(np.abs(a - b) <= 1e-5 * b)
    assert np.all(np.abs(a - walk["norm"]) <= 1e-6 * walk["norm"])


# ---- blockings, a smaller transform after a larger one ---------------------------------------------------------------------
def _ulp_apart(one, cut):
    ulp = np.spacing(np.maximum(np.abs(one), np.abs(cut)))
    return float(np.max(np.abs(one - cut) / ulp))


def test_two_unit_budget(engine, wave, walk):
    from psa_amd import _hip
    s, L, H, n_lags = _segments("64_32_64")
    n_seg, P = 1 + (T - L) // H, CC.padded_length(L, n_lags)
    assert n_seg == 6 and P == 128
    # the self part: two units of SELF_ATOMS atoms x the largest tile x one padded segment -- atoms, vectors and segments are cut
    engine.ensure_resident(_hip.SLOT_POSITIONS, walk["pos"])
    engine.set_atom_weights(walk["w"])
    engine.set_segments(s)
    inv, half, bins = walk["inv"], walk["half"], walk["bins"]
    for b, nb in ((bins, 6), (None, 0)):
        one = engine.self_correlations(inv, half, n_lags, b, nb, None)
        assert np.array_equal(one.view(np.uint32), engine.self_correlations(inv, half, n_lags, b, nb, None).view(np.uint32))
        sizes = S.tiles(half, b)
        assert len(sizes) > 1 and -(-37 // _hip.SELF_ATOMS) > 2
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 2 * _hip.SELF_ATOMS * max(sizes) * P * 8)
        cut = engine.self_correlations(inv, half, n_lags, b, nb, None)
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
        print(f"self, {'shells' if nb else 'per vector'}: two blockings {_ulp_apart(one, cut):.2f} ulp apart")
        assert _ulp_apart(one, cut) <= 1.0
    assert not engine.self_correlations(inv, half, n_lags, bins, 6, np.zeros(0, np.int32)).any()
    # the coherent fields: two vectors of q and two (vector, padded segment) units
    engine.ensure_resident(_hip.SLOT_POSITIONS, wave["pos"])
    engine.ensure_resident(_hip.SLOT_VELOCITIES, wave["vel"])
    engine.set_atom_weights(wave["w"])
    inv, half, bins = wave["inv"], wave["half"], wave["bins"]
    small = 2 * (4 * T * 8 + 4 * P * 8)
    one = engine.lattice_correlations(inv, half, n_lags, bins, 6, None, True)
    assert np.array_equal(one.view(np.uint32), engine.lattice_correlations(inv, half, n_lags, bins, 6, None, True).view(np.uint32))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, small)
    cut = engine.lattice_correlations(inv, half, n_lags, bins, 6, None, True)
    print(f"coherent shells: two blockings {_ulp_apart(one, cut):.2f} ulp apart")
    assert _ulp_apart(one, cut) <= 1.0
    per_cut = engine.lattice_correlations(inv, half, n_lags, None, 0, None, True)
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
    per_one = engine.lattice_correlations(inv, half, n_lags, None, 0, None, True)
    # per vector, later sub-blocks of segments add to the float32 power, as psa_lattice_spectra documents: n_seg roundings
    # relative to each power value, hence to the lag-0 sum
    lim = n_seg * 2.0 ** -24 * np.abs(per_one[:, :1].astype(np.float64)) * (L / (L - np.arange(n_lags)))[None, :, None]
    assert np.all(np.abs(per_one.astype(np.float64) - per_cut) <= lim + np.spacing(np.abs(per_one)))
    assert not engine.lattice_correlations(inv, half, n_lags, bins, 6, np.zeros(0, np.int32), True).any()


def test_smaller_transform_after_a_larger_one_matches_a_fresh_context(engine, wave, walk):
    """the tails [L, P) are written for every block: what an earlier, longer call left in the buffers is never read"""
    from psa_amd import Segments, _hip
    fresh = _hip.Engine(0)
    try:
        results = []
        for eng, warm in ((engine, True), (fresh, False)):
            eng.set_atom_weights(walk["w"])
            eng.ensure_resident(_hip.SLOT_POSITIONS, walk["pos"])
            if warm:                                                        # P = 512, then P = 64 in the same buffers
                eng.set_segments(None)
                eng.self_correlations(walk["inv"], walk["half"], 200, walk["bins"], 6, None)
            eng.set_segments(Segments(40, 20, "boxcar"))
            a = eng.self_correlations(walk["inv"], walk["half"], 20, walk["bins"], 6, None)
            b = eng.self_correlations(walk["inv"], walk["half"][:70], 25, None, 0, None)
            eng.set_atom_weights(wave["w"])
            eng.ensure_resident(_hip.SLOT_POSITIONS, wave["pos"])
            eng.ensure_resident(_hip.SLOT_VELOCITIES, wave["vel"])
            if warm:
                eng.set_segments(None)
                eng.lattice_correlations(wave["inv"], wave["half"], 200, wave["bins"], 6, None, True)
                eng.lattice_correlations(wave["inv"], wave["half"], 200, None, 0, None, True)
            eng.set_segments(Segments(40, 20, "boxcar"))
            c = eng.lattice_correlations(wave["inv"], wave["half"], 20, wave["bins"], 6, None, True)
            d = eng.lattice_correlations(wave["inv"], wave["half"][:70], 25, None, 0, None, True)
            results.append((a, b, c, d))
        for x, y in zip(*results):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    finally:
        fresh.close()


# ---- refusals, and no trace ------------------------------------------------------------------------------------------------
def test_refusals(engine, wave):
    from psa_amd import Segments, _hip
    inv = np.ascontiguousarray(wave["inv"])
    engine.ensure_resident(_hip.SLOT_POSITIONS, wave["pos"])
    engine.ensure_resident(_hip.SLOT_VELOCITIES, wave["vel"])
    lib, h = engine._lib, engine._h
    f32p, i32p, f64p = Ct.POINTER(Ct.c_float), Ct.POINTER(Ct.c_int32), Ct.POINTER(Ct.c_double)
    ind, bins = np.ascontiguousarray(wave["half"][:9]), np.ascontiguousarray(wave["bins"][:9])
    out, sh = np.empty((3, 10, 9), np.float32), np.empty((3, 10, 6), np.float32)
    bp, ip, op, sp, binp = inv.ctypes.data_as(f64p), ind.ctypes.data_as(i32p), out.ctypes.data_as(f32p), sh.ctypes.data_as(f32p), bins.ctypes.data_as(i32p)
    third = out.nbytes // 3

    def refused(rc, word):
        msg = lib.psa_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def lat(n_lags=10, b=None, nb=0, o=op, nbytes=out.nbytes, box=bp, vec=ip, K=9):
        return lib.psa_lattice_correlations(h, box, vec, K, b, nb, None, 0, 1, n_lags, o, nbytes)

    def slf(n_lags=10, b=None, nb=0, o=op, nbytes=third, box=bp, vec=ip, K=9):
        return lib.psa_self_correlations(h, box, vec, K, b, nb, None, 0, n_lags, o, nbytes)

    for call, shell_bytes in ((lat, sh.nbytes), (slf, sh.nbytes // 3)):
        assert call() == 0
        assert call(b=binp, nb=6, o=sp, nbytes=shell_bytes) == 0
        refused(call(box=None), "null")
        refused(call(vec=None), "null")
        refused(call(o=None), "null")
        refused(call(K=0), "at least one")
        refused(call(n_lags=0), "at least one lag")
        refused(call(n_lags=-3), "at least one lag")
        refused(call(n_lags=T + 1), "n_lags")
        refused(call(nbytes=third - 4), "out_bytes")
        refused(call(b=binp, nb=6), "out_bytes")                           # the shell form is (.., n_lags, n_bins)
        refused(call(box=np.zeros(9).ctypes.data_as(f64p)), "singular")
        engine.set_segments(Segments(64, 32, "hann"))
        refused(call(), "boxcar")
        taper = np.ones(64)
        taper[17] = 1.0 - 2.0 ** -23
        engine.set_segments(Segments(64, 32, tuple(taper)))
        refused(call(), "boxcar")
        engine.set_segments(Segments(64, 32, "boxcar"))
        assert call() == 0
        refused(call(n_lags=65), "n_lags")
        engine.set_segments(Segments(512, 256, "boxcar"))
        refused(call(), "segment length")
        engine.set_segments(None)
    nn = ind.copy()
    nn[7] = (0, -1, 2)
    refused(lat(vec=nn.ctypes.data_as(i32p), b=binp, nb=6, o=sp, nbytes=sh.nbytes), "half-space")
    # the budget counts the padded length P = 512 where the spectra count L = 250
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 * 8 * (T + 512) - 1)
    refused(lat(n_lags=T), "budget")
    assert "a segment of 512" in lib.psa_last_error().decode()
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 * 8 * (T + 512))
    big = np.empty((3, T, 9), np.float32)
    assert lat(n_lags=T, o=big.ctypes.data_as(f32p), nbytes=big.nbytes) == 0
    unit = _hip.SELF_ATOMS * 9 * 512 * 8
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, unit - 1)
    refused(slf(n_lags=T, o=big.ctypes.data_as(f32p), nbytes=big.nbytes // 3), "budget")
    assert str(unit) in lib.psa_last_error().decode() and "512 frames" in lib.psa_last_error().decode()
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, unit)
    assert slf(n_lags=T, o=big.ctypes.data_as(f32p), nbytes=big.nbytes // 3) == 0
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
    # the back-transform's own entry
    X = np.ones((1, 8, 2))
    xp = X.ctypes.data_as(f64p)
    assert lib.psa_debug_correlation_transform(h, xp, 1, 8, 2, 5, 1, 5, 0, op) == 0
    refused(lib.psa_debug_correlation_transform(h, None, 1, 8, 2, 5, 1, 5, 0, op), "null")
    refused(lib.psa_debug_correlation_transform(h, xp, 1, 8, 2, 5, 1, 6, 0, op), "n_lags")
    refused(lib.psa_debug_correlation_transform(h, xp, 4, 2, 2, 5, 1, 2, 0, op), "fields")
    refused(lib.psa_debug_correlation_transform(h, xp, 1, 8, 2, 5, 0, 5, 0, op), "positive")
    X[0, 3, 1] = np.inf
    refused(lib.psa_debug_correlation_transform(h, xp, 1, 8, 2, 5, 1, 5, 0, op), "not finite")
    engine.release(_hip.SLOT_VELOCITIES)
    refused(lat(), "velocities")
    assert slf() == 0                                                      # the self part needs no velocities
    engine.release(_hip.SLOT_POSITIONS)
    refused(slf(), "positions")
    refused(lat(), "positions")


def test_no_trace_in_the_other_entry_points(engine, walk):
    """`calculate`, `calculate_powder_spectra` and `calculate_self_spectra` give the bits they gave before the correlation
    calls in between; the stage times of a correlation call are where the header says"""
    from psa_amd import Segments
    vel = S.C.trajectory(37, T, seed=41, box=walk["box"])[1]
    calc = _calculator(engine, walk["pos"], walk["box"], vel, cells=(1, 1, 1))
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    for _ in range(2):                      # (the first call uploads and projects at once, the next builds what is cached)
        calc.calculate(mags, vecs)
    s, box = Segments(64, 32, "hann"), Segments(64, 32, "boxcar")
    kw = dict(atom_weights=walk["w"])

    def spectra():
        return (calc.calculate(mags, vecs).sed, calc.calculate_powder_spectra(EDGES, segments=s, **kw).density,
                calc.calculate_powder_spectra(EDGES, segments=s, **kw).transverse,
                calc.calculate_self_spectra(walk["half"][:30], segments=s, **kw).density,
                calc.calculate_powder_self_spectra(EDGES, segments=box, **kw).density)
    before = spectra()
    engine.timings()                                                       # (reset)
    calc.calculate_powder_correlations(EDGES, segments=box, **kw)
    t = engine.timings()
    assert t["project"] > 0 and t["gather"] > 0 and t["fft"] > 0 and t["epilogue"] > 0 and t["phase"] > 0 and t["d2h"] > 0
    calc.calculate_powder_self_correlations(EDGES, segments=box, lags=64, **kw)
    t = engine.timings()
    assert t["transpose"] > 0 and t["gather"] > 0 and t["fft"] > 0 and t["epilogue"] > 0 and t["phase"] > 0 and t["d2h"] > 0
    calc.calculate_lattice_correlations(walk["half"][:20], lags=100)
    calc.calculate_self_correlations(walk["half"][:20], max_atoms=17)
    for a, b in zip(before, spectra()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
