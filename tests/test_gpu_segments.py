"""Segment-averaged (Welch) spectra on the GPU (psa_set_segments, `calculate(..., segments=...)`): parity with the
float64 restatement (tests/welch64.py) over modes, segment shapes and windows; the trivial case is the existing
result; Parseval; folded +-k pairs; the low-rank k-path route; the first (uploading) call; no leak into later calls;
ABI errors."""
import numpy as np
import pytest

from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu


def _trajectory(cells=(4, 4, 4), T=256, seed=3):
    """Synthetic silicon with a planted mode: 512 atoms of two types (as tests/test_gpu_weights.py)."""
    from psa_amd import Trajectory, synth
    spec = synth.SyntheticSpec(cells, T, dt_ps=0.002, seed=seed,
                               modes=[synth.Mode(3.0, 16, (2 * np.pi / synth.A_SI * 0.25, 0, 0), 0)])
    r0, types, box = synth.lattice(spec.cells)
    vel = synth.velocities_block(spec, synth.mode_tables(spec, r0), 0, T)
    pos = (r0[None] + 0.05 * np.random.default_rng(seed).standard_normal(vel.shape)).astype(np.float32)
    return Trajectory(pos, vel, types, np.arange(T, dtype=np.float32), box, np.diag(box).copy(),
                      np.zeros(3, np.float32), spec.dt_ps), spec.cells


@pytest.fixture(scope="module")
def syn(engine):
    from psa_amd import SEDCalculator
    tr, cells = _trajectory()
    calcs = {disp: SEDCalculator(tr, *cells, use_displacements=disp).attach(engine=engine) for disp in (False, True)}
    reset(engine)
    yield dict(traj=tr, calcs=calcs)
    reset(engine)
    engine.invalidate()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


MODES = ("coherent", "incoherent", "displacements", "mass")
SHAPES = [(64, 32), (100, 30), (64, 64), (48, 80), (256, 256)]


def _mode(syn, mode):
    """(calculator, calculate kwargs, data, groups, weights) of a mode for the restatement"""
    from oracle import psa_oracle as O
    from psa_amd import mass_weights
    tr = syn["traj"]
    disp = mode == "displacements"
    calc = syn["calcs"][disp]
    kw, groups, w = {}, [None], None
    if mode in ("incoherent", "mass"):
        kw = dict(basis_atom_types=[1, 2], summation_mode="incoherent")
        groups = [np.flatnonzero(tr.types == t) for t in (1, 2)]
    if mode == "mass":
        w = mass_weights(tr.types, {1: 1.0, 2: 207.0})
        kw["atom_weights"] = w
    mean = O.mean_positions(tr.positions)
    data = (tr.positions.astype(np.float64) - mean[None]) if disp else tr.velocities
    return calc, kw, data, mean, groups, w


@pytest.mark.parametrize("window", ["hann", "boxcar"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"L{L}_H{H}" for L, H in SHAPES])
@pytest.mark.parametrize("mode", MODES)
def test_parity_float64(engine, syn, mode, shape, window):
    from psa_amd import Segments
    from welch64 import welch_intensity64
    calc, kw, data, mean, groups, w = _mode(syn, mode)
    L, H = shape
    seg = Segments(L, H, window)
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    got = calc.calculate(mags, vecs, segments=seg, **kw)
    ref = welch_intensity64(data, mean, vecs, groups, seg.window_array(), L, H, w)
    assert got.sed.shape == (L, 24) and got.sed.dtype == np.float32 and not got.is_complex
    np.testing.assert_array_equal(got.freqs, np.fft.fftfreq(L, d=calc.dt_ps))
    err = rel_max(got.sed, ref)
    print(f"{mode} L={L} H={H} {window}: rel_max {err:.3e}")
    assert err <= 1e-5


def test_trivial_case_is_the_existing_result(engine, syn):
    from psa_amd import Segments
    calc = syn["calcs"][False]
    T = syn["traj"].n_frames
    seg = Segments(T, T, "boxcar")
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    kw = dict(basis_atom_types=[1, 2], summation_mode="incoherent")
    plain = calc.calculate(mags, vecs, **kw)
    trivial = calc.calculate(mags, vecs, segments=seg, **kw)
    assert np.array_equal(_bits(trivial.sed), _bits(plain.sed))
    coherent = calc.calculate(mags, vecs)
    trivial_c = calc.calculate(mags, vecs, segments=seg)
    assert rel_max(trivial_c.sed, coherent.intensity) <= 1e-6


@pytest.mark.parametrize("L", [32, 64, 128])
def test_parseval(engine, syn, L):
    """boxcar, H = L dividing T: sum over frequencies per k of the segmented and of the full spectrum agree"""
    from psa_amd import Segments
    calc = syn["calcs"][False]
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    full = calc.calculate(mags, vecs).intensity
    seg = calc.calculate(mags, vecs, segments=Segments(L, L, "boxcar")).sed
    a, b = np.sum(seg.astype(np.float64), axis=0), np.sum(full.astype(np.float64), axis=0)
    assert np.max(np.abs(a - b) / b) <= 1e-6


def test_folded_pairs(engine, syn):
    from psa_amd import Segments, _hip
    calc = syn["calcs"][False]
    _, gvecs, shape = calc.get_k_grid("xy", (-1.5, 1.5), (-1.0, 1.0), 6, 6, 0.0)
    none = np.array([], np.float32)
    seg = Segments(64, 32)
    try:
        for kw in ({}, dict(basis_atom_types=[1, 2], summation_mode="incoherent")):
            engine.set_option(_hip.OPT_FOLD_PAIRS, 1)
            folded = calc.calculate(none, gvecs, k_grid_shape=shape, segments=seg, **kw)
            engine.set_option(_hip.OPT_FOLD_PAIRS, 0)
            flat = calc.calculate(none, gvecs, k_grid_shape=shape, segments=seg, **kw)
            assert folded.sed.shape == flat.sed.shape == (64, 36)
            assert rel_max(folded.sed, flat.sed) <= 1e-6
    finally:
        reset(engine)


def test_lowrank_route(engine, syn):
    from psa_amd import Segments, _hip
    from welch64 import welch_intensity64
    calc, kw, data, mean, groups, w = _mode(syn, "coherent")
    mags, vecs = calc.get_k_path("100", 1.0, 256)
    seg = Segments(64, 32)
    try:
        engine.set_option(_hip.OPT_PLANES_EAGER, 1)
        calc.calculate(mags, vecs, segments=seg)                   # planes built: the next call takes the route
        n0 = engine.lowrank_launches()
        got = calc.calculate(mags, vecs, segments=seg)
        assert engine.lowrank_launches() > n0
        ref = welch_intensity64(data, mean, vecs, groups, seg.window_array(), 64, 32)
        assert rel_max(got.sed, ref) <= 1e-5
    finally:
        reset(engine)


def test_first_call_and_no_leak(engine, syn):
    """the uploading call equals the resident one bit for bit; an unsegmented call after a segmented one returns
    what it returned before, bit for bit"""
    from psa_amd import Segments
    calc = syn["calcs"][False]
    mags, vecs = calc.get_k_path("100", 1.0, 8)
    seg = Segments(100, 30)
    for kw in ({}, dict(basis_atom_types=[1, 2], summation_mode="incoherent")):
        engine.invalidate()
        first = calc.calculate(mags, vecs, segments=seg, **kw)     # psa_sed_project_upload
        resident = calc.calculate(mags, vecs, segments=seg, **kw)
        assert np.array_equal(_bits(first.sed), _bits(resident.sed))
        before = calc.calculate(mags, vecs, **kw)                   # (same residency state as `after`)
        calc.calculate(mags, vecs, segments=seg, **kw)
        after = calc.calculate(mags, vecs, **kw)
        assert after.sed.shape == before.sed.shape and after.sed.dtype == before.sed.dtype
        assert np.array_equal(after.sed.view(np.uint8), before.sed.view(np.uint8))
    assert engine.segment_length == 0


def test_abi_errors(engine, syn):
    from psa_amd import Segments, _hip
    calc = syn["calcs"][False]
    T, N = syn["traj"].n_frames, syn["traj"].n_atoms
    mean = calc._mean_positions()
    mags, vecs = calc.get_k_path("100", 1.0, 8)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, syn["traj"].velocities)
    lib, h = engine._lib, engine._h
    w = np.ones(4, np.float32)
    assert lib.psa_set_segments(h, 4, 0, w.ctypes.data_as(_hip._f32p)) == -1            # hop < 1
    assert lib.psa_set_segments(h, 4, 2, np.zeros(4, np.float32).ctypes.data_as(_hip._f32p)) == -1   # U = 0
    bad = np.float32([1, np.nan, 1, 1])
    assert lib.psa_set_segments(h, 4, 2, bad.ctypes.data_as(_hip._f32p)) == -1
    try:
        engine.set_segments(Segments(64, 32))
        with pytest.raises(_hip.PsaHipError, match="rc=-1"):                             # no F_INTENSITY
            engine.project(_hip.SLOT_VELOCITIES, mean, vecs)
        with pytest.raises(_hip.PsaHipError, match="rc=-1"):                             # not with frame sharding
            engine.fs_project(_hip.SLOT_VELOCITIES, mean, vecs, None, _hip.F_INTENSITY, T, 0, len(vecs))
        engine.set_segments(Segments(T + 16, 8))
        with pytest.raises(_hip.PsaHipError, match="rc=-1"):                             # L > T
            engine.project(_hip.SLOT_VELOCITIES, mean, vecs, None, _hip.F_INTENSITY)
        with pytest.raises(_hip.PsaHipError, match="rc=-1"):
            engine.calculate(_hip.SLOT_VELOCITIES, mean, vecs, None, _hip.F_INTENSITY)
    finally:
        engine.set_segments(None)
    # the context is usable afterwards, and the slab rows of a segmented result are (K, L)
    engine.set_segments(Segments(64, 32))
    try:
        engine.project(_hip.SLOT_VELOCITIES, mean, vecs, None, _hip.F_INTENSITY)
        rows = engine.slab_read(0, len(vecs), 64, True)
        out = engine.finalize(64, len(vecs), True)
    finally:
        engine.set_segments(None)
    assert np.array_equal(rows.T, out)
    ref = calc.calculate(mags, vecs, segments=Segments(64, 32))
    assert np.array_equal(_bits(ref.sed), _bits(out))
