"""The dynamic structure factor and the current correlations on the GPU (psa_dynamic_spectra, `calculate_dynamic_spectra`):
the kernel's projections element by element inside the bound of tests/dynamic_cases.py at every edge of its tiling, with
the same bits from a repeated call and from a call cut into blocks of k-vectors; the error of the hardware sine and
cosine the bound rests on; the cross-check with the SED projection on frozen positions; the calculator against the
float64 restatement (tests/dynamic64.py) with and without segments; Parseval and the Jacobi-Anger lines; every refusal;
no trace in a later SED calculation.

The kernel's tiles (psa_amd/_hip.py mirrors psa_amd/csrc/dynamic.hip): DYN_ATOMS = 512 atoms per staged tile, DYN_CHAIN =
128 atoms per float32 accumulator (a lane sums two strands: with one atom slice a chain is full at 256 atoms),
DYN_FRAMES = 4 frames per workgroup, DYN_THREADS = 256 lanes split into min(256, K rounded up to a power of two)
k-vectors x atom slices (one wavefront holds one slice from K = 64 on)."""
import math

import numpy as np
import pytest

import dynamic64 as D
import dynamic_cases as C
import ref64
from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _clean(engine):
    reset(engine)
    yield
    reset(engine)


@pytest.fixture(scope="module", autouse=True)
def _forget(engine):
    yield
    engine.invalidate()


def _resident(engine, pos, vel):
    from psa_amd import _hip
    engine.ensure_resident(_hip.SLOT_POSITIONS, pos)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, vel)


# ---- the sine and the cosine --------------------------------------------------------------------------------------
def test_sincos_sweep(engine):
    """v_sin_f32 / v_cos_f32 on [-2, 2] turns against float64: 2^22 + 1 evenly spaced arguments (every multiple of 2^-20:
    the quadrant edges and zero among them) and 2^20 random ones.  DYN_SINCOS_ERR is twice the measured maximum."""
    from psa_amd import _hip
    x = np.concatenate([np.linspace(-2.0, 2.0, (1 << 22) + 1), np.random.default_rng(1).uniform(-2.0, 2.0, 1 << 20)]).astype(np.float32)
    got = engine.debug_dynamic_sincos(x).astype(np.float64)
    th = 2 * np.pi * x.astype(np.float64)
    e_sin, e_cos = np.abs(got[:, 0] - np.sin(th)), np.abs(got[:, 1] - np.cos(th))
    worst = max(float(e_sin.max()), float(e_cos.max()))
    near = np.abs(x) <= 0.51                                              # where the kernel's reduced argument lies
    worst_near = max(float(e_sin[near].max()), float(e_cos[near].max()))
    print(f"sincos sweep: max |sin err| {e_sin.max():.3e} at x = {x[e_sin.argmax()]!r}, max |cos err| {e_cos.max():.3e} at "
          f"x = {x[e_cos.argmax()]!r}; on |x| <= 0.51: {worst_near:.3e}; DYN_SINCOS_ERR = {_hip.DYN_SINCOS_ERR:.3e}, "
          f"eps_term = {C.eps_term():.3e} (cap {C.EPS_TERM_CAP:.3e})")
    assert 2 * worst <= _hip.DYN_SINCOS_ERR
    assert C.eps_term() <= C.EPS_TERM_CAP


# ---- the per-element bound ------------------------------------------------------------------------------------------
# (atoms, frames, K, currents, index list, weights, offset)
_A, _CH = 512, 128
BOUND_CASES = [
    (1, 1, 1, True, False, "unit", 0.0),
    (2, 3, 2, False, False, "signed", 0.0),
    (_CH - 1, 3, 1, True, False, "unit", C.OFFSET),
    (_CH, 5, 2, True, True, "sqrt_mass", 0.0),
    (_CH + 1, 4, 63, False, False, "unit", C.OFFSET),          # two lanes per k-vector, half a wavefront idle in k
    (2 * _CH - 1, 1, 64, True, False, "signed", C.OFFSET),     # one wavefront per slice
    (2 * _CH, 3, 65, True, True, "unit", 0.0),               # 128 k-vector slots, two slices
    (2 * _CH + 1, 5, 129, False, True, "sqrt_mass", C.OFFSET), # one slice: a chain fills at 256 atoms, one atom after it
    (2 * _CH + 1, 3, 128, True, False, "unit", C.OFFSET),
    (_A - 1, 3, 257, True, False, "unit", C.OFFSET),           # two tiles of k-vectors, the second of one
    (_A, 4, 256, False, False, "signed", 0.0),
    (_A + 1, 5, 3, True, True, "signed", C.OFFSET),            # a second staged tile of one atom, 64 slices
    (_A + 1, 1, 257, True, False, "sqrt_mass", 0.0),
    (3 * _A + 7, 3, 130, True, True, "unit", C.OFFSET),        # four tiles, three folds per strand
]


@pytest.mark.parametrize("case", BOUND_CASES, ids=[f"n{c[0]}_T{c[1]}_K{c[2]}_{'j' if c[3] else 'rho'}_{'idx' if c[4] else 'all'}_{c[5]}_{int(c[6])}"
                                                   for c in BOUND_CASES])
def test_projection_within_bound_same_bits_any_blocking(engine, case):
    from psa_amd import _hip
    n, T, K, currents, listed, wk, offset = case
    n_all = n + 5 if listed else n
    pos, vel = C.trajectory(n_all, T, seed=n + K, offset=offset)
    k = C.k_list(K, seed=K, aligned=bool(offset))
    w = C.weights(wk, n_all, seed=2)
    idx = np.random.default_rng(3).permutation(n_all)[:n].astype(np.int32) if listed else None
    reach = C.max_abs_phase(pos, k, idx)
    assert (0.8e4 <= reach <= 1.2e4) if offset else reach < 200.0           # offset: |k.r| = 1e4 rad
    _resident(engine, pos, vel)
    engine.set_atom_weights(w)
    got = engine.debug_dynamic_project(k, idx, currents)
    ref, absum = D.project64(pos, vel, k, idx, w, currents, with_abs=True)
    assert got.shape == ref.shape == (K, 4 if currents else 1, T)
    frac = np.abs(got.astype(np.complex128) - ref) / C.bound(absum, n)[None]
    worst = np.unravel_index(np.argmax(frac), frac.shape)
    print(f"largest |k.r| {reach:.3e} rad: worst element {worst} at {frac[worst]:.4f} of its bound ({C.bound(absum, n)[worst[1:]]:.3e})")
    assert frac.max() <= 1.0
    if K >= 2:
        assert np.all(got[1].imag == 0)                                   # k = 0: sin(0) = 0 exactly
    again = engine.debug_dynamic_project(k, idx, currents)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))      # two identical calls: the same bits
    if K >= 2:                                                             # ... and so a call cut into blocks of k-vectors
        per_k = (4 if currents else 1) * T * 8
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, per_k * max(1, K // 3))
        blocked = engine.debug_dynamic_project(k, idx, currents)
        assert np.array_equal(got.view(np.uint32), blocked.view(np.uint32))


# ---- cross-check with the SED projection --------------------------------------------------------------------------------
def test_frozen_positions_give_the_sed_projection(engine):
    """With the positions of every frame frozen to frame 0's, q_1..3 is the SED projection of the velocities at those
    mean positions -- up to the two definitions: the SED's phase argument is BY DEFINITION the float32 FMA chain
    (tests/ref64.py), this path's the exact k.r, so "equal within the sum of both bounds" is inexact as a premise and
    the allowance has a third term, |ref_dyn - ref_sed|, the distance of the two float64 references (triangle
    inequality; computed from float64 alone).  The test prints how large that term is beside the two bounds: where it
    dominates, the check says no more than the two kernels' own bound tests do; near the origin it is of their size."""
    from psa_amd import _hip
    import dense_cases
    n, T, K = 130, 24, 9
    pos, vel = C.trajectory(n, T, seed=4)
    pos[:] = pos[0]
    k = C.k_list(K, seed=8)
    _resident(engine, pos, vel)
    q_dyn = engine.debug_dynamic_project(k, None, True)[:, 1:, :].astype(np.complex128)
    engine.set_k1(_hip.K1_MFMA32)
    q_sed = engine.debug_project_only(_hip.SLOT_VELOCITIES, pos[0], k).astype(np.complex128)
    ref_dyn, absum = D.project64(pos, vel, k, None, None, True, with_abs=True)
    ref_sed = ref64.project64(vel, pos[0], k)
    B = ref64.scale_B(vel, pos[0])
    np.testing.assert_allclose(B, absum[1:], rtol=1e-14)
    bounds = C.bound(absum[1:], n)[None] + math.sqrt(2.0) * dense_cases.bound("mfma32", n) * B[None]
    definitional = np.abs(ref_dyn[:, 1:] - ref_sed)
    allowed = bounds + definitional
    frac = np.abs(q_dyn - q_sed) / allowed
    print(f"definitional term |ref_dyn - ref_sed| over the sum of both bounds: largest {np.max(definitional / bounds):.3f}, "
          f"median {np.median(definitional / bounds):.3f}; |q_dyn - q_sed| over the sum of both bounds alone: largest "
          f"{np.max(np.abs(q_dyn - q_sed) / bounds):.3f}")
    print(f"dynamic against SED projection: worst element at {frac.max():.4f} of the allowance")
    assert frac.max() <= 1.0
    assert rel_max(q_dyn, q_sed) < 1e-5


# ---- the calculator against the restatement -------------------------------------------------------------------------------
def _calculator(engine, pos, vel, dt=0.002, cells=(4, 4, 4), box=None):
    from psa_amd import SEDCalculator, Trajectory
    T, n = pos.shape[:2]
    box = np.diag([C.BOX] * 3).astype(np.float32) if box is None else box
    tr = Trajectory(pos, vel, np.ones(n, np.int32), np.arange(T, dtype=np.float32), box, np.diag(box).copy(),
                    np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, *cells).attach(engine=engine)


@pytest.fixture(scope="module")
def thermal():
    """T = 256, N = 130, K = 9 with k = 0 and one (k, -k) pair; q in float64 once, for every segment shape"""
    pos, vel = C.trajectory(130, 256, seed=21)
    k = C.k_list(9, seed=22)
    w = C.weights("sqrt_mass", 130, seed=23)
    return dict(pos=pos, vel=vel, k=k, w=w, q=D.project64(pos, vel, k, None, w, True))


SEGMENTS = {"none": None, "hann_64_32": (64, 32, "hann"), "boxcar_64_64": (64, 64, "boxcar")}


@pytest.mark.parametrize("currents", [False, True], ids=["density", "currents"])
@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_calculator_parity_float64(engine, thermal, seg, currents):
    from psa_amd import DynamicSpectra, Segments
    s = None if SEGMENTS[seg] is None else Segments(*SEGMENTS[seg])
    calc = _calculator(engine, thermal["pos"], thermal["vel"])
    k = thermal["k"]
    out = calc.calculate_dynamic_spectra(np.linalg.norm(k, axis=1), k, atom_weights=thermal["w"], segments=s, currents=currents)
    assert isinstance(out, DynamicSpectra)
    L = 256 if s is None else s.length
    ref = D.spectra64(thermal["q"], k, *((None, None, None) if s is None else (s.window_array(), s.length, s.hop)))
    np.testing.assert_allclose(out.freqs, np.fft.fftfreq(L, 0.002))
    assert out.density.shape == (L, 9) and out.density.dtype == np.float32
    assert out.weight_norm == pytest.approx(float(np.sum(thermal["w"].astype(np.float64) ** 2)))
    errs = {"density": rel_max(out.density, ref[0])}
    if currents:
        errs["longitudinal"] = rel_max(out.longitudinal, ref[1])
        errs["transverse"] = rel_max(out.transverse, ref[2])
        assert np.all(out.longitudinal[:, 1] == 0) and np.all(out.transverse[:, 1] > 0)        # the k = 0 row
    else:
        assert out.longitudinal is None and out.transverse is None
    print(f"{seg} {'currents' if currents else 'density'}: {errs}")
    assert max(errs.values()) <= 1e-5
    np.testing.assert_allclose(out.structure_factor, out.density.astype(np.float64) * L * 0.002 / out.weight_norm, rtol=1e-12)
    if seg == "boxcar_64_64":                                              # Parseval: boxcar, H = L
        q = thermal["q"]
        np.testing.assert_allclose(out.density.sum(axis=0), np.mean(np.abs(q[:, 0]) ** 2, axis=1), rtol=1e-5)
        if currents:
            np.testing.assert_allclose((out.longitudinal + 2 * out.transverse).sum(axis=0),
                                       np.mean(np.sum(np.abs(q[:, 1:]) ** 2, axis=1), axis=1), rtol=1e-5)


def test_index_list_small_budget_and_empty_set(engine, thermal):
    """an atom subset under a budget that cuts the k-list and the segments into sub-blocks equals the one-block call;
    an empty atom set gives zeros"""
    from psa_amd import Segments, _hip
    pos, vel, k, w = thermal["pos"], thermal["vel"], thermal["k"], thermal["w"]
    idx = np.random.default_rng(5).permutation(130)[:77].astype(np.int32)
    s = Segments(64, 32, "hann")
    _resident(engine, pos, vel)
    engine.set_atom_weights(w)
    engine.set_segments(s)
    one = engine.dynamic_spectra(k, idx, True)
    ref = D.dynamic_spectra64(pos, vel, k, idx, w, True, s.window_array(), 64, 32)
    assert max(rel_max(one[i], ref[i]) for i in range(3)) <= 1e-5
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 * 8 * (4 * 256 + 3 * 64))     # 4 k-vectors of q, 3 (k, segment) units
    cut = engine.dynamic_spectra(k, idx, True)
    assert max(rel_max(cut[i], one[i]) for i in range(3)) <= 2e-6          # later sub-blocks add in float32
    assert not engine.dynamic_spectra(k, np.zeros(0, np.int32), True).any()
    assert not engine.debug_dynamic_project(k, np.zeros(0, np.int32), False).any()


# ---- Jacobi-Anger on the device ---------------------------------------------------------------------------------------------
def _wave(e_hat, cells=4, T=32, bin0=3, amp=0.07):
    R = np.stack(np.meshgrid(*[np.arange(cells)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    k0 = np.array([2 * np.pi / cells, 0.0, 0.0])
    w0 = 2 * np.pi * bin0 / T
    phase = (R @ k0)[None, :] - w0 * np.arange(T)[:, None]
    e = np.asarray(e_hat, np.float64)
    return k0, (R[None] + amp * np.cos(phase)[..., None] * e).astype(np.float32), (amp * w0 * np.sin(phase)[..., None] * e).astype(np.float32)


def test_jacobi_anger_lines_on_the_device(engine):
    from test_dynamic_host import bessel_j
    box = np.diag([4.0] * 3).astype(np.float32)
    k0, pos, vel = _wave([1.0, 0.0, 0.0])
    G = np.array([2 * np.pi, 0.0, 0.0])
    ks = np.stack([k0 + G, 2 * k0 + G]).astype(np.float32)
    out = _calculator(engine, pos, vel, box=box).calculate_dynamic_spectra(np.linalg.norm(ks, axis=1), ks)
    for col, n in ((0, 1), (1, 2)):
        want = 64 * 64 * bessel_j(n, float(ks[col, 0]) * 0.07) ** 2
        print(f"line {n}: {out.density[3 * n, col]:.6e} against N^2 J_{n}^2 = {want:.6e}")
        assert abs(out.density[3 * n, col] - want) <= 1e-4 * want
    # e parallel to k: the current's line is longitudinal; e perpendicular: transverse
    k1 = k0[None].astype(np.float32)
    par = _calculator(engine, pos, vel, box=box).calculate_dynamic_spectra(np.linalg.norm(k1, axis=1), k1)
    assert par.longitudinal[3, 0] > 0 and par.transverse[3, 0] <= 1e-5 * par.longitudinal[3, 0]
    _, pos_y, vel_y = _wave([0.0, 1.0, 0.0])
    perp = _calculator(engine, pos_y, vel_y, box=box).calculate_dynamic_spectra(np.linalg.norm(k1, axis=1), k1)
    assert perp.transverse[3, 0] > 0 and perp.longitudinal[3, 0] <= 1e-5 * perp.transverse[3, 0]
    # the same wave, turned: equal up to the Bessel factor (2 J_1(z) / z)^2 = 1 - z^2 / 4 of the longitudinal line, z = k0 A = 0.11
    assert perp.transverse[3, 0] == pytest.approx(0.5 * par.longitudinal[3, 0], rel=1e-2)


# ---- refusals, and no trace ---------------------------------------------------------------------------------------------------
def test_refusals(engine, thermal):
    import ctypes as Ct
    from psa_amd import Segments, _hip
    pos, vel, k = thermal["pos"], thermal["vel"], thermal["k"]
    _resident(engine, pos, vel)
    lib, h = engine._lib, engine._h
    f32p, i32p = Ct.POINTER(Ct.c_float), Ct.POINTER(Ct.c_int32)
    out = np.empty((3, 256, 9), np.float32)
    kp, op = k.ctypes.data_as(f32p), out.ctypes.data_as(f32p)

    def refused(rc, word):
        msg = lib.psa_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(lib.psa_dynamic_spectra(h, None, 9, None, 0, 1, op, out.nbytes), "null")
    refused(lib.psa_dynamic_spectra(h, kp, 9, None, 0, 1, None, out.nbytes), "null")
    refused(lib.psa_dynamic_spectra(h, kp, 0, None, 0, 1, op, out.nbytes), "at least one")
    refused(lib.psa_dynamic_spectra(h, kp, 9, None, 0, 1, op, out.nbytes - 4), "out_bytes")
    refused(lib.psa_dynamic_spectra(h, kp, 9, None, 0, 0, op, out.nbytes), "out_bytes")          # density only is (1, L, K)
    bad = np.array([3, 130], np.int32)
    refused(lib.psa_dynamic_spectra(h, kp, 9, bad.ctypes.data_as(i32p), 2, 1, op, out.nbytes), "out of bounds")
    k_nan = k.copy()
    k_nan[4, 1] = np.nan
    refused(lib.psa_dynamic_spectra(h, k_nan.ctypes.data_as(f32p), 9, None, 0, 1, op, out.nbytes), "finite")
    refused(lib.psa_debug_dynamic_project(h, kp, 9, None, 0, 1, None), "null")
    engine.set_atom_weights(np.ones(129, np.float32))
    refused(lib.psa_dynamic_spectra(h, kp, 9, None, 0, 1, op, out.nbytes), "weights")
    engine.set_atom_weights(None)
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 * 8 * 256 - 1)
    refused(lib.psa_dynamic_spectra(h, kp, 9, None, 0, 1, op, out.nbytes), "budget")
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
    # L > T: segments set for a longer trajectory than the one that is resident now
    engine.set_segments(Segments(512, 256, "hann"))
    big = np.empty((3, 512, 9), np.float32)
    refused(lib.psa_dynamic_spectra(h, kp, 9, None, 0, 1, big.ctypes.data_as(f32p), big.nbytes), "segment length")
    engine.set_segments(None)
    # velocities of another shape, then absent; then no positions
    engine.ensure_resident(_hip.SLOT_VELOCITIES, np.ascontiguousarray(vel[:128]))
    refused(lib.psa_dynamic_spectra(h, kp, 9, None, 0, 1, op, out.nbytes), "shape")
    engine.release(_hip.SLOT_VELOCITIES)
    refused(lib.psa_dynamic_spectra(h, kp, 9, None, 0, 1, op, out.nbytes), "velocities")
    one = np.empty((1, 256, 9), np.float32)
    assert lib.psa_dynamic_spectra(h, kp, 9, None, 0, 0, one.ctypes.data_as(f32p), one.nbytes) == 0   # the density needs none
    engine.release(_hip.SLOT_POSITIONS)
    refused(lib.psa_dynamic_spectra(h, kp, 9, None, 0, 0, one.ctypes.data_as(f32p), one.nbytes), "positions")
    with pytest.raises(_hip.PsaHipError, match="unknown option"):
        engine.set_option(14, 1)


def test_no_trace_in_the_sed_state(engine, thermal):
    """an ordinary `calculate` gives the bits it gave before a dynamic-spectra call in between"""
    from psa_amd import Segments
    calc = _calculator(engine, thermal["pos"], thermal["vel"])
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    for _ in range(2):                      # (the first call uploads and projects at once, the next builds what is cached)
        calc.calculate(mags, vecs)
    before = calc.calculate(mags, vecs)
    calc.calculate_dynamic_spectra(np.linalg.norm(thermal["k"], axis=1), thermal["k"], segments=Segments(64, 32, "hann"),
                                   atom_weights=thermal["w"])
    after = calc.calculate(mags, vecs)
    assert np.array_equal(before.sed.view(np.uint32), after.sed.view(np.uint32))
    engine.timings()                                                       # (reset)
    calc.calculate_dynamic_spectra(np.linalg.norm(thermal["k"], axis=1), thermal["k"])
    timings = engine.timings()
    assert timings["project"] > 0 and timings["fft"] > 0 and timings["epilogue"] > 0 and timings["d2h"] > 0
