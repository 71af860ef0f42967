"""The vibrational density of states on the GPU (psa_vdos, `calculate_vdos`): parity with the float64 restatement
(tests/vdos64.py) over modes, segment shapes and windows; the single-atom identity with the SED path; the planted mode;
Parseval; index-list and empty groups; float64 accumulation over 32768 atoms; invariance under the blocking and
determinism; no leak into later SED calls; ABI errors.  Beside rel_max the parity tests hold every element to the bound
of tests/vdos_cases.py (its edges are in tests/test_gpu_vdos_perelement.py)."""
import ctypes as C

import numpy as np
import pytest

import vdos_cases as V
from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu


def _trajectory(cells=(4, 4, 4), T=256, seed=3):
    """Synthetic silicon with a planted mode: 512 atoms of two types (the trajectory of tests/test_gpu_segments.py)."""
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


MODES = ("all", "partial", "displacements", "mass")
SHAPES = [(256, 256), (64, 32), (100, 30), (48, 80), (63, 21)]


def _mode(syn, mode):
    """(calculator, calculate_vdos kwargs, restatement kwargs) of a mode"""
    from oracle import psa_oracle as O
    from psa_amd import mass_weights
    tr = syn["traj"]
    disp = mode == "displacements"
    calc = syn["calcs"][disp]
    kw, ref = {}, dict(data=tr.positions if disp else tr.velocities, groups=[None])
    if disp:
        ref["mean"] = O.mean_positions(tr.positions)
    if mode in ("partial", "mass"):
        kw = dict(basis_atom_types=[1, 2])
        ref["groups"] = [np.flatnonzero(tr.types == t) for t in (1, 2)]
    if mode == "mass":
        kw["atom_weights"] = ref["weights"] = mass_weights(tr.types, {1: 1.0, 2: 207.0})
    return calc, kw, ref


@pytest.mark.parametrize("window", ["hann", "boxcar"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"L{L}_H{H}" for L, H in SHAPES])
@pytest.mark.parametrize("mode", MODES)
def test_parity_float64(engine, syn, mode, shape, window):
    from psa_amd import Segments
    from vdos64 import vdos64
    calc, kw, ref_kw = _mode(syn, mode)
    L, H = shape
    seg = Segments(L, H, window)
    got = calc.calculate_vdos(segments=seg, **kw)
    ref = vdos64(window=seg.window_array(), L=L, H=H, **ref_kw)
    G = len(ref_kw["groups"])
    assert got.dos.shape == (L // 2 + 1, G, 3) and got.dos.dtype == np.float32 and len(got.groups) == G
    assert np.array_equal(got.freqs, np.fft.rfftfreq(L, d=calc.dt_ps))
    err = rel_max(got.dos, ref)
    ratio = V.check(got.dos, window=seg.window_array(), L=L, H=H, ref=ref, **ref_kw)
    print(f"{mode} L={L} H={H} {window}: rel_max {err:.3e}, {ratio:.3f} x bound")
    assert err <= 1e-5
    assert ratio <= 1.0
    assert engine.segment_length == 0


def test_full_length_without_segments(engine, syn):
    """segments=None is one boxcar segment of all frames"""
    from vdos64 import vdos64
    for mode in MODES:
        calc, kw, ref_kw = _mode(syn, mode)
        got = calc.calculate_vdos(**kw)
        ref = vdos64(**ref_kw)
        err, ratio = rel_max(got.dos, ref), V.check(got.dos, ref=ref, **ref_kw)
        print(f"{mode} full length: rel_max {err:.3e}, {ratio:.3f} x bound")
        assert got.dos.shape[0] == 129 and err <= 1e-5
        assert ratio <= 1.0


@pytest.mark.parametrize("weighted", [False, True])
def test_single_atom_identity(engine, syn, weighted):
    """sum_c D of the group {a} is the SED intensity of basis_atom_indices=[a] at any k: |exp(i k.r)| = 1"""
    from psa_amd import mass_weights
    calc, tr = syn["calcs"][False], syn["traj"]
    T = tr.n_frames
    w = mass_weights(tr.types, {1: 1.0, 2: 207.0}) if weighted else None
    mags, vecs = calc.get_k_path("100", 1.0, 8)
    for a in (3, 310):
        d = calc.calculate_vdos(basis_atom_indices=[a], atom_weights=w).total[:, 0]
        sed = calc.calculate(mags, vecs, basis_atom_indices=[a], atom_weights=w).intensity
        for j in (2, 7):
            err = rel_max(d, sed[:T // 2 + 1, j])
            print(f"atom {a} k {j} weighted {weighted}: rel_max {err:.3e}")
            assert err <= 1e-5


def test_planted_mode(engine, syn):
    got = syn["calcs"][False].calculate_vdos()
    assert int(np.argmax(got.dos[:, 0, 0])) == 16


@pytest.mark.parametrize("L", [64, 63])
def test_parseval(engine, syn, L):
    from psa_amd import Segments
    from vdos64 import parseval_sum
    calc, tr = syn["calcs"][False], syn["traj"]
    got = calc.calculate_vdos(basis_atom_types=[1, 2], segments=Segments(L, L, "boxcar"))
    used = tr.velocities[:(tr.n_frames // L) * L].astype(np.float64)
    for gi, t in enumerate((1, 2)):
        ms = np.sum(np.mean(used[:, tr.types == t, :] ** 2, axis=0), axis=0)
        err = np.max(np.abs(parseval_sum(got.dos[:, gi, :], L) - ms) / ms)
        print(f"L={L} type {t}: Parseval {err:.3e}")
        assert err <= 1e-6


def test_index_list_groups(engine, syn):
    """a sparse unsorted group, an empty group and a group that skips atoms, straight through the engine"""
    from psa_amd import Segments, _hip
    from vdos64 import vdos64
    tr = syn["traj"]
    engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
    groups = [np.array([301, 5, 17, 131, 2]), np.array([], int), np.arange(9, 400, 3)]
    for seg in (None, Segments(64, 32)):
        engine.set_segments(seg)
        try:
            got = engine.vdos(_hip.SLOT_VELOCITIES, None, groups)
        finally:
            engine.set_segments(None)
        kw = {} if seg is None else dict(window=seg.window_array(), L=seg.length, H=seg.hop)
        ref = vdos64(tr.velocities, groups, **kw)
        assert got.shape == ref.shape and got.dtype == np.float32
        assert not got[:, 1, :].any()
        for gi in (0, 2):
            err = rel_max(got[:, gi, :], ref[:, gi, :])
            print(f"group {gi} segments {seg is not None}: rel_max {err:.3e}")
            assert err <= 1e-5
        ratio = V.check(got, tr.velocities, groups, ref=ref, **kw)
        print(f"segments {seg is not None}: {ratio:.3f} x bound")
        assert ratio <= 1.0
    in_order = engine.vdos(_hip.SLOT_VELOCITIES, None, [np.sort(groups[0]), groups[1], groups[2]])
    assert np.array_equal(in_order, engine.vdos(_hip.SLOT_VELOCITIES, None, groups))     # the order inside a group is free


def test_blocking_invariance_and_determinism(engine, syn):
    """a work budget that forces several atom blocks and several segment blocks gives the default-budget result"""
    from psa_amd import Segments, _hip
    calc, tr = syn["calcs"][False], syn["traj"]
    seg = Segments(64, 32)                                   # 7 segments; 256 atom pairs = 8 tiles; one unit = 768 L bytes
    kw = dict(basis_atom_types=[1, 2], segments=seg)
    # groups of 45 and 111 atoms: 23 + 56 pairs, so the first tile of 32 pairs holds rows of both groups
    kw_odd = dict(basis_atom_indices=[list(range(0, 90, 2)), list(range(1, 223, 2))], segments=seg)
    unit = 768 * 64
    try:
        whole, whole_odd = calc.calculate_vdos(**kw).dos, calc.calculate_vdos(**kw_odd).dos
        assert np.array_equal(whole, calc.calculate_vdos(**kw).dos)
        for dos, groups in ((whole, [np.flatnonzero(tr.types == t) for t in (1, 2)]),
                            (whole_odd, [np.arange(0, 90, 2), np.arange(1, 223, 2)])):
            ratio = V.check(dos, tr.velocities, groups, seg.window_array(), seg.length, seg.hop)
            print(f"default budget, groups of {[len(g) for g in groups]}: {ratio:.3f} x bound")
            assert ratio <= 1.0
        for budget in (3 * unit, 14 * unit + 5, 20 * unit):  # 8 x 3 blocks of (1 tile, 3 segments); 4 x 1 of (2, 7); 4 x 1
            engine.set_option(_hip.OPT_VDOS_WORK_BYTES, budget)
            for k, ref in ((kw, whole), (kw_odd, whole_odd)):
                a, b = calc.calculate_vdos(**k).dos, calc.calculate_vdos(**k).dos
                err = rel_max(a, ref)
                print(f"budget {budget}: rel_max {err:.3e}")
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
                assert err <= 1e-6
        engine.set_option(_hip.OPT_VDOS_WORK_BYTES, unit - 1)
        with pytest.raises(_hip.PsaHipError, match=str(unit)):
            calc.calculate_vdos(**kw)
    finally:
        reset(engine)
    assert np.array_equal(whole, calc.calculate_vdos(**kw).dos)


def test_no_leak_into_sed_calls(engine, syn):
    from psa_amd import Segments, mass_weights
    calc, tr = syn["calcs"][False], syn["traj"]
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    for kw in ({}, dict(basis_atom_types=[1, 2], summation_mode="incoherent")):
        before = calc.calculate(mags, vecs, **kw)
        calc.calculate_vdos(basis_atom_types=[1, 2], segments=Segments(100, 30),
                            atom_weights=mass_weights(tr.types, {1: 1.0, 2: 207.0}))
        after = calc.calculate(mags, vecs, **kw)
        assert after.sed.shape == before.sed.shape and after.sed.dtype == before.sed.dtype
        assert np.array_equal(after.sed.view(np.uint8), before.sed.view(np.uint8))
    assert engine.segment_length == 0


def test_uploads_when_not_resident(engine, syn):
    from psa_amd import _hip
    calc, tr = syn["calcs"][False], syn["traj"]
    resident = calc.calculate_vdos().dos
    engine.invalidate()
    first = calc.calculate_vdos().dos
    assert engine.is_resident(_hip.SLOT_VELOCITIES, tr.velocities)
    assert np.array_equal(first, resident)


def test_abi_errors(engine, syn):
    from psa_amd import Segments, _hip
    from vdos64 import vdos64
    tr = syn["traj"]
    T, N = tr.n_frames, tr.n_atoms
    engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
    lib, h = engine._lib, engine._h
    F = T // 2 + 1

    def call(idx, off, G, nbytes=None, out=None):
        out = np.zeros((G, 3, F), np.float32) if out is None else out
        ip = None if idx is None else np.ascontiguousarray(idx, np.int32)
        op = None if off is None else np.ascontiguousarray(off, np.int64)
        return lib.psa_vdos(h, _hip.SLOT_VELOCITIES, None, None if ip is None else ip.ctypes.data_as(_hip._i32p),
                            None if op is None else op.ctypes.data_as(_hip._i64p), G, 0, out.ctypes.data_as(_hip._f32p),
                            C.c_size_t(out.nbytes if nbytes is None else nbytes))

    assert call(None, None, 1, nbytes=4 * 3 * F - 4) == -1                     # out_bytes not exact
    assert b"out_bytes" in lib.psa_last_error()
    assert call([0, 1, 1, 2], [0, 2, 4], 2) == -1                              # overlapping groups
    assert b"disjoint" in lib.psa_last_error()
    assert call([0, N], [0, 2], 1) == -1                                       # index out of range
    assert call([0, -1], [0, 2], 1) == -1
    assert call(None, None, 2) == -1                                           # NULL list means one group
    engine.set_segments(Segments(T + 16, 8))
    try:
        assert call(None, None, 1, out=np.zeros((1, 3, (T + 16) // 2 + 1), np.float32)) == -1     # L > T
    finally:
        engine.set_segments(None)
    engine.set_atom_weights(np.ones(N + 1, np.float32))
    try:
        assert call(None, None, 1) == -1                                       # weights of another length
    finally:
        engine.set_atom_weights(None)
    out = np.zeros((1, 3, F), np.float32)                                      # the context is usable afterwards
    assert call(None, None, 1, out=out) == 0
    assert rel_max(out.transpose(2, 0, 1), vdos64(tr.velocities, [None])) <= 1e-5


def test_accumulation_over_32768_atoms(engine, syn):
    """16^3 cells, T = 64, one group, boxcar L = 64: the sum over 32768 atoms is held in float64 on the device"""
    from psa_amd import SEDCalculator, Segments
    from vdos64 import vdos64
    tr, cells = _trajectory(cells=(16, 16, 16), T=64, seed=5)
    assert tr.n_atoms == 32768
    calc = SEDCalculator(tr, *cells).attach(engine=engine)
    try:
        got = calc.calculate_vdos(segments=Segments(64, 64, "boxcar"))
        ref = vdos64(tr.velocities, [None], np.ones(64), 64, 64)
        err = rel_max(got.dos, ref)
        ratio = V.check(got.dos, tr.velocities, [None], np.ones(64), 64, 64, ref=ref)
        print(f"N = 32768, T = 64: rel_max {err:.3e}, {ratio:.3f} x bound")
        assert got.dos.shape == (33, 1, 3) and err <= 1e-5
        assert ratio <= 1.0
    finally:
        engine.invalidate()
