"""The dynamic structure factor and the current correlations without a GPU: the float64 restatement of the definition
(tests/dynamic64.py) against closed forms and against tests/welch64.py, the kernel's bound (tests/dynamic_cases.py)
against a float32 model of its arithmetic -- and against the arithmetic it must not use --, and the argument checks of
the Python layer that need no device."""
import math

import numpy as np
import pytest

import dynamic64 as D
import dynamic_cases as C
import welch64
from psa_amd import DynamicSpectra, SEDCalculator, Segments, Trajectory, _hip


def bessel_j(n, z):
    """J_n(z): SciPy's if importable, else its integral (1/pi) int_0^pi cos(n tau - z sin tau) d tau -- the integrand is
    smooth and periodic, so the trapezoid rule converges geometrically"""
    try:
        from scipy.special import jv
        return float(jv(n, z))
    except ImportError:
        tau = np.linspace(0.0, 2 * np.pi, 4096, endpoint=False)
        return float(np.mean(np.cos(n * tau - z * np.sin(tau))))


# ---- (a) Jacobi-Anger ---------------------------------------------------------------------------------------------
CELLS, T_JA, BIN0, AMP = 4, 32, 3, 0.07


def wave(e_hat, dtype=np.float64):
    """a 4 x 4 x 4 simple cubic lattice (a = 1) displaced by A e cos(k0.R - w0 t), k0 = 2 pi / 4 along x, w0 on bin 3 of 32
    frames: lattice sites (N, 3), k0, positions and velocities (T, N, 3)"""
    R = np.stack(np.meshgrid(*[np.arange(CELLS)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    k0 = np.array([2 * np.pi / CELLS, 0.0, 0.0])
    w0 = 2 * np.pi * BIN0 / T_JA
    t = np.arange(T_JA)[:, None]
    phase = (R @ k0)[None, :] - w0 * t
    e = np.asarray(e_hat, np.float64)
    pos = R[None] + AMP * np.cos(phase)[..., None] * e
    vel = AMP * w0 * np.sin(phase)[..., None] * e
    return R, k0, pos.astype(dtype), vel.astype(dtype)


def test_jacobi_anger_lines_and_what_the_mean_position_projection_misses():
    e_hat = np.array([1.0, 0.0, 0.0])
    R, k0, pos, vel = wave(e_hat)
    G = np.array([2 * np.pi, 0.0, 0.0])                                   # a reciprocal-lattice vector of the cell
    ks = np.stack([k0 + G, 2 * k0 + G, k0, 2 * k0])
    den, _, _ = D.dynamic_spectra64(pos, vel, ks, currents=False)
    N = R.shape[0]
    for col, (n, k) in enumerate(((1, ks[0]), (2, ks[1]), (1, ks[2]), (2, ks[3]))):
        want = N * N * bessel_j(n, float(k @ e_hat) * AMP) ** 2
        got = den[n * BIN0, col]
        print(f"k = {k[0]:.4f}: |F|^2 at bin {n * BIN0} = {got:.12e}, N^2 J_{n}^2 = {want:.12e}")
        assert abs(got - want) <= 1e-10 * want
    # the mean-position projection of the same run, q[k,t] = sum_a u_x[t,a] exp(i k.R_a), has its line at (k0, w0) and
    # nothing at (2 k0, 2 w0): the second harmonic is the dynamic structure factor's alone
    u = pos[:, :, 0] - R[None, :, 0]
    q_mean = u @ np.exp(1j * (R @ ks[2:].T))                               # (T, 2)
    P = np.abs(np.fft.fft(q_mean, axis=0) / T_JA) ** 2
    assert P[BIN0, 0] > 0 and P[2 * BIN0, 1] < 1e-10 * P[BIN0, 0]
    assert den[2 * BIN0, 3] > 1e-4 * den[BIN0, 2]                          # ... where the density has N^2 J_2^2


def test_currents_of_the_wave_split_by_polarisation():
    _, k0, pos, vel = wave([1.0, 0.0, 0.0])
    _, lon, tra = D.dynamic_spectra64(pos, vel, k0[None])
    assert lon[BIN0, 0] > 0 and tra[BIN0, 0] < 1e-12 * lon[BIN0, 0]        # e parallel to k: longitudinal
    _, k0, pos, vel = wave([0.0, 1.0, 0.0])
    _, lon, tra = D.dynamic_spectra64(pos, vel, k0[None])
    assert tra[BIN0, 0] > 0 and lon[BIN0, 0] < 1e-12 * tra[BIN0, 0]        # e perpendicular to k: transverse


# ---- (b), (c) the Welch stage -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def thermal():
    pos, vel = C.trajectory(37, 100, seed=5)
    k = C.k_list(5, seed=6)
    w = C.weights("sqrt_mass", 37, seed=7)
    return pos, vel, k, w, D.project64(pos, vel, k, None, w)


def test_parseval(thermal):
    pos, vel, k, w, q = thermal
    L = 32                                                                # 3 segments, 4 frames unused
    den, lon, tra = D.spectra64(q, k, np.ones(L, np.float32), L, L)
    used = q[:, :, :96]
    np.testing.assert_allclose(den.sum(axis=0), np.mean(np.abs(used[:, 0]) ** 2, axis=1), rtol=1e-12)
    np.testing.assert_allclose((lon + 2 * tra).sum(axis=0), np.mean(np.sum(np.abs(used[:, 1:]) ** 2, axis=1), axis=1), rtol=1e-12)


@pytest.mark.parametrize("seg", [None, Segments(64, 32, "hann"), Segments(32, 32, "boxcar"), Segments(48, 7, "hann")])
def test_welch_stage_equals_welch64(thermal, seg):
    pos, vel, k, w, q = thermal
    T = q.shape[2]
    win, L, H = (np.ones(T, np.float32), T, T) if seg is None else (seg.window_array(), seg.length, seg.hop)
    den, lon, tra = D.spectra64(q, k, None if seg is None else win, L, H)
    q_t = np.transpose(q, (2, 0, 1))                                       # (T, K, NC), welch64's layout
    np.testing.assert_allclose(den, welch64.segment_intensity64(q_t[:, :, :1], win, L, H), rtol=1e-12, atol=0)
    np.testing.assert_allclose(lon + 2 * tra, welch64.segment_intensity64(q_t[:, :, 1:], win, L, H), rtol=1e-12, atol=0)
    # a k = 0 row has no direction: longitudinal 0, transverse half of sum_c |j_c|^2
    assert np.all(lon[:, 1] == 0) and np.all(tra[:, 1] > 0)
    # one k-vector along x: the longitudinal part is the x current's spectrum alone
    kx = np.array([[1.5, 0.0, 0.0]], np.float32)
    qx = D.project64(pos, vel, kx, None, w)
    _, lon_x, tra_x = D.spectra64(qx, kx, None if seg is None else win, L, H)
    np.testing.assert_allclose(lon_x, welch64.segment_intensity64(np.transpose(qx, (2, 0, 1))[:, :, 1:2], win, L, H), rtol=1e-12)


# ---- (d) the bound can fail -----------------------------------------------------------------------------------------
FAMILIES = [  # atoms, frames, K, offset, weights, index list, currents
    (64, 3, 3, 0.0, "unit", False, True),
    (64, 3, 3, C.OFFSET, "signed", False, True),          # the family of the proof below: |k.r| = 1e4 rad
    (64, 2, 1, C.OFFSET, "sqrt_mass", True, False),       # K = 1: 256 slices, every strand one atom or none
    (300, 1, 2, C.OFFSET, "unit", False, True),           # 128 slices ... and more than DYN_CHAIN atoms nowhere
    (300, 1, 256, 0.0, "unit", True, False),              # one slice: two strands of 150 atoms, one fold each
]


def _family(n, T, K, offset, wk, listed, currents):
    """inputs, reference, bound of a family; offset families take the aligned k-vectors, which put |k.r| at 1e4 rad"""
    pos, vel = C.trajectory(n, T, seed=n + K, offset=offset)
    k = C.k_list(K, seed=3, aligned=bool(offset))[:4]                       # (the model loops over k-vectors in Python)
    w = C.weights(wk, n, seed=1)
    idx = np.random.default_rng(2).permutation(n)[: n - 3].astype(np.int32) if listed else None
    ref, absum = D.project64(pos, vel, k, idx, w, currents, with_abs=True)
    return pos, vel, k, w, idx, ref, C.bound(absum, n if idx is None else idx.size)[None]


@pytest.mark.parametrize("family", FAMILIES, ids=[f"n{f[0]}_K{f[2]}_{int(f[3])}" for f in FAMILIES])
def test_bound_holds_for_the_kernels_arithmetic(family):
    n, T, K, offset, wk, listed, currents = family
    assert C.eps_term() <= C.EPS_TERM_CAP
    assert 2 * C.slices(K) == {1: 512, 2: 256, 3: 128, 256: 2}[K]
    pos, vel, k, w, idx, ref, lim = _family(*family)
    reach = C.max_abs_phase(pos, k, idx)
    assert (0.8e4 <= reach <= 1.2e4) if offset else reach < 200.0
    good = C.project_model(pos, vel, k, idx, w, currents, False, call_K=K)
    frac = float(np.max(np.abs(good - ref) / lim))
    print(f"n = {n}, K = {K}, largest |k.r| {reach:.3e} rad: the kernel's arithmetic has its worst element at {frac:.4f} of its bound")
    assert frac <= 1.0


def test_the_radians_chain_lands_over_the_bound_at_1e4_rad():
    """The proof that the bound can fail, on the one family the bound was set against: 64 atoms whose positions carry an
    offset that makes |k.r| = 1e4 rad.  The model of the kernel's arithmetic stays inside; the same model with k.r as a
    float32 FMA chain in radians does not."""
    family = FAMILIES[1]
    n, T, K, offset, wk, listed, currents = family
    assert n == 64 and offset == C.OFFSET
    pos, vel, k, w, idx, ref, lim = _family(*family)
    reach = C.max_abs_phase(pos, k, idx)
    assert 0.8e4 <= reach <= 1.2e4
    good = float(np.max(np.abs(C.project_model(pos, vel, k, idx, w, currents, False, call_K=K) - ref) / lim))
    bad = float(np.max(np.abs(C.project_model(pos, vel, k, idx, w, currents, True, call_K=K) - ref) / lim))
    print(f"64 atoms, largest |k.r| {reach:.3e} rad: the kernel's arithmetic at {good:.4f} of the bound, the float32 radians "
          f"chain at {bad:.1f} times the bound")
    assert good <= 1.0 < bad


def test_constants_mirror_the_kernels():
    """psa_amd/_hip.py holds the kernel's tile and chain sizes for the bound of the tests: the same numbers as psa_ctx.h"""
    import re
    from pathlib import Path
    text = (Path(_hip.__file__).resolve().parent / "csrc" / "psa_ctx.h").read_text()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (DYN_[A-Z]+) = (\d+);", text)}
    assert set(found) == {"DYN_THREADS", "DYN_ATOMS", "DYN_CHAIN", "DYN_FRAMES"}
    for name, value in found.items():
        assert getattr(_hip, name) == value, name


def test_turns_model_is_exact_to_its_stated_error():
    """the reduced phase of the kernel's arithmetic against k.r / 2 pi in float64: within 1.51 u turns of it, modulo 1"""
    pos, _ = C.trajectory(500, 2, seed=11, offset=C.OFFSET)
    k = C.k_list(6, seed=12, aligned=True)
    assert 0.8e4 <= C.max_abs_phase(pos, k) <= 1.2e4
    kh, kl = C.kappa_parts(k)
    for j in range(6):
        got = C.turns_model(pos, kh[j], kl[j]).astype(np.float64)
        want = (pos.astype(np.float64) @ k[j].astype(np.float64)) / (2 * np.pi)
        err = got - want
        err -= np.rint(err)
        assert np.max(np.abs(got)) <= 0.5 + 1e-3
        assert np.max(np.abs(err)) <= 1.51 * C.U, float(np.max(np.abs(err)) / C.U)


# ---- (e) the Python layer ---------------------------------------------------------------------------------------------
def _calculator(n_atoms=8, n_frames=16):
    pos, vel = C.trajectory(n_atoms, n_frames, seed=1)
    box = np.diag([C.BOX] * 3).astype(np.float32)
    tr = Trajectory(pos, vel, np.ones(n_atoms, np.int32), np.arange(n_frames, dtype=np.float32), box, np.diag(box).copy(),
                    np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, 4, 4, 4)


def test_argument_checks_need_no_device():
    calc = _calculator()
    k = C.k_list(3, seed=1)
    mags = np.linalg.norm(k, axis=1)
    with pytest.raises(TypeError, match="Segments"):
        calc.calculate_dynamic_spectra(mags, k, segments=(8, 4))
    with pytest.raises(ValueError):
        calc.calculate_dynamic_spectra(mags, k, segments=Segments(32, 16, "hann"))            # L > T
    with pytest.raises(ValueError, match="atom_weights"):
        calc.calculate_dynamic_spectra(mags, k, atom_weights=np.ones(7))
    with pytest.raises(ValueError, match=r"\(K, 3\)"):
        calc.calculate_dynamic_spectra(mags, k[:, :2])
    with pytest.raises(ValueError, match="finite"):
        calc.calculate_dynamic_spectra(mags, np.array([[0.0, np.inf, 0.0]]))
    with pytest.raises(ValueError, match="out of bounds"):
        calc.calculate_dynamic_spectra(mags, k, basis_atom_indices=[0, 8])

    class TwoRanks:
        nranks, mode, engine = 2, "k", None
    calc._shard = TwoRanks()
    with pytest.raises(NotImplementedError, match="sharded"):
        calc.calculate_dynamic_spectra(mags, k)
    calc._shard = None
    assert calc._engine is None                                            # nothing above reached for a device


def test_empty_k_list_and_the_result_type():
    calc = _calculator()
    out = calc.calculate_dynamic_spectra(np.zeros(0), np.zeros((0, 3), np.float32), segments=Segments(8, 4, "hann"), currents=False)
    assert isinstance(out, DynamicSpectra) and out.density.shape == (8, 0) and out.longitudinal is None and out.transverse is None
    assert out.freqs.shape == (8,) and calc._engine is None
    d = DynamicSpectra(np.full((4, 2), 3.0, np.float32), None, None, np.fft.fftfreq(4, 0.5), np.zeros(2), np.zeros((2, 3)), np.arange(5), 6.0)
    np.testing.assert_allclose(d.structure_factor, 3.0 * 4 * 0.5 / 6.0)     # density L dt / sum w^2, dt from freqs
    one = DynamicSpectra(np.full((1, 2), 3.0, np.float32), None, None, np.zeros(1), np.zeros(2), np.zeros((2, 3)), np.arange(5), 6.0)
    with pytest.raises(ValueError, match="dt_ps"):
        one.structure_factor                                               # one bin: no time step in freqs
    one.dt_ps = 0.5
    np.testing.assert_allclose(one.structure_factor, 3.0 * 1 * 0.5 / 6.0)
    assert out.dt_ps == 0.002
    assert _hip.OPT_DYNAMIC_WORK_BYTES == 13 and {"psa_dynamic_spectra", "psa_debug_dynamic_project"} <= set(_hip.SIGNATURES)
