"""Per-atom weights on the GPU (psa_set_atom_weights, `calculate(..., atom_weights=...)`): exact identities on every
projection-kernel family (weights 1 and 8 against the unweighted result, bit for bit, and no leak into a later call),
parity with a float64 NumPy restatement for mass-, raw-mass- and charge-like weights through the dense kernels and the
low-rank k-path route, agreement of the folded / streamed / pipelined / frame-piece paths, the plane cache left alone,
and clean errors."""
import numpy as np
import pytest

from conftest import make_calculator, rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu


def _trajectory(cells=(4, 4, 4), T=256, seed=3):
    """Synthetic silicon with a planted mode: 512 atoms of two types, host arrays (the calculator uploads them)."""
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
    yield dict(traj=tr, calcs=calcs)
    reset(engine)
    engine.invalidate()


MODES = {"coherent": ({}, False), "incoherent": (dict(basis_atom_types=[1, 2], summation_mode="incoherent"), False),
         "displacements": ({}, True)}
# (K, options, k1 selector): the kernel family each case lands on once the group's planes exist
FAMILIES = {
    "bf16_split_K8": (8, dict(planes=0), None),
    "f16_pair_K24": (24, dict(planes=0), None),
    "planes32_K12": (12, {}, None),
    "planes64_K24": (24, {}, None),
    "planes128_K40": (40, {}, None),
    "wide256_K100": (100, {}, None),
    "wide256_K256_dense": (256, dict(lowrank=0), None),
    "lowrank_K256": (256, {}, None),
    "mfma32_K24": (24, {}, "MFMA32"),
    "wave_K24": (24, {}, "WAVE"),
}


def _configure(engine, opts, k1):
    from psa_amd import _hip
    reset(engine)
    engine.set_option(_hip.OPT_PLANES, opts.get("planes", 1))
    engine.set_option(_hip.OPT_PLANES_EAGER, 1)
    engine.set_option(_hip.OPT_K1_LOWRANK, opts.get("lowrank", 1))
    if k1:
        engine.set_k1(getattr(_hip, "K1_" + k1))


def _inten(sed):
    """sum_c |S|^2 of a complex result (`SED.intensity`, read once); an incoherent result is that already"""
    return sed.intensity if sed.is_complex else sed.sed


def _run(engine, calc, mags, vecs, kw, weights=None, direct=False):
    """(sed array, intensity) of one calculation.  direct: engine.project + finalize, where a complex result of a long
    k-path reaches the low-rank route (the calculator sends it to psa_sed_calculate, which stays on the dense kernels
    while it pipelines the copy-out)"""
    if not direct:
        sed = calc.calculate(mags, vecs, atom_weights=weights, **kw)
        return sed.sed, _inten(sed)
    assert not kw
    slot, data, flags = calc._data_slot()
    mean = calc._mean_positions()
    engine.ensure_resident(slot, data)
    engine.set_atom_weights(weights)
    try:
        engine.project(slot, mean, vecs, None, flags)
        out = engine.finalize(calc.traj.n_frames, len(vecs), False)
    finally:
        engine.set_atom_weights(None)
    return out, np.sum(np.abs(out) ** 2, axis=-1).astype(np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.float32).view(np.uint32)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("mode", list(MODES))
def test_exact_identities(engine, syn, family, mode):
    """w = 1: bit-identical to no weights; w = 8: exactly 8 x sed (complex) / 64 x intensity; then an unweighted call
    equals the first one bit for bit (the setting does not leak)."""
    K, opts, k1 = FAMILIES[family]
    kw, disp = MODES[mode]
    calc, N = syn["calcs"][disp], syn["traj"].n_atoms
    mags, vecs = calc.get_k_path("100", 1.0, K)
    lowrank = family == "lowrank_K256"
    direct = lowrank and mode != "incoherent"
    try:
        _configure(engine, opts, k1)
        _run(engine, calc, mags, vecs, kw, None, direct)           # upload, planes: later calls all take one route
        n0 = engine.lowrank_launches()
        ref, ref_i = _run(engine, calc, mags, vecs, kw, None, direct)
        taken = engine.lowrank_launches() - n0
        ones, ones_i = _run(engine, calc, mags, vecs, kw, np.ones(N, np.float32), direct)
        n1 = engine.lowrank_launches()
        eights, eights_i = _run(engine, calc, mags, vecs, kw, np.full(N, 8.0, np.float32), direct)
        if lowrank and not disp:
            assert taken >= 1 and engine.lowrank_launches() - n1 == taken
        again, _ = _run(engine, calc, mags, vecs, kw, None, direct)
        assert np.array_equal(_bits(ones), _bits(ref))
        assert np.array_equal(_bits(ones_i), _bits(ref_i))
        scale = 8.0 if ref.dtype == np.complex64 else 64.0
        assert np.array_equal(_bits(eights), _bits((ref * np.float32(scale)).astype(ref.dtype)))
        assert np.array_equal(_bits(eights_i), _bits(ref_i * np.float32(64.0)))
        assert np.array_equal(_bits(again), _bits(ref))
        assert float(np.max(ref_i)) > 0.0
    finally:
        reset(engine)


# ---------------------------------------------------------------------------------------------------------------------
def weighted_reference(traj, k_vectors, w, groups=None, disp=False, incoherent=False):
    """float64 restatement of the oracle (oracle/psa_oracle.py: sed_for_group, calculate) on w[None, :, None] * d: the
    phase from the unweighted float32 mean positions, the reference's float32 phase argument."""
    from oracle import psa_oracle as O
    pos, vel = traj.positions, traj.velocities
    mean = O.mean_positions(pos)
    d = (pos.astype(np.float64) - mean[None]) if disp else vel.astype(np.float64)
    d = d * np.asarray(w, np.float64)[None, :, None]
    T = d.shape[0]
    if groups is None:
        groups = [np.arange(d.shape[1])]
    if not incoherent:
        groups = [np.unique(np.concatenate(groups))]
    out = 0.0
    for g in groups:
        P = np.exp(1j * np.dot(k_vectors, mean[g].T).astype(np.float64))          # (K, N_g)
        q = np.einsum("tac,ka->tkc", d[:, g, :], P, optimize=True)
        S = np.fft.fft(q, axis=0) / T
        if not incoherent:
            return S
        out = out + np.sum(np.abs(S) ** 2, axis=-1)
    return out


def _weights(kind, traj):
    from psa_amd import mass_weights
    N = traj.n_atoms
    rng = np.random.default_rng(7)
    if kind == "mass":
        return mass_weights(traj.types, {1: 1.0, 2: 207.0})
    if kind == "raw_mass":
        return rng.uniform(1.0, 1000.0, N).astype(np.float32)
    w = rng.choice([-2.0, -1.0, 0.5, 1.0, 3.0], N).astype(np.float32)          # charge-like, signed
    w[rng.choice(N, 5, replace=False)] = 0.0
    return w


@pytest.mark.parametrize("kind", ["mass", "raw_mass", "charge"])
@pytest.mark.parametrize("mode", ["coherent", "incoherent", "displacements"])
def test_parity_dense_and_lowrank(engine, syn, kind, mode):
    kw, disp = MODES[mode]
    calc, traj = syn["calcs"][disp], syn["traj"]
    w = _weights(kind, traj)
    mags, vecs = calc.get_k_path("100", 1.0, 256)
    incoh = mode == "incoherent"
    groups = [np.flatnonzero(traj.types == t) for t in (1, 2)] if incoh else None
    ref = weighted_reference(traj, vecs, w, groups, disp, incoh)
    ref_i = ref if incoh else np.sum(np.abs(ref) ** 2, axis=-1)
    got = {}
    try:
        for lr in (0, 1):
            _configure(engine, {"lowrank": lr}, None)
            direct = lr == 1 and not incoh
            _run(engine, calc, mags, vecs, kw, None, direct)
            n0 = engine.lowrank_launches()
            got[lr], got_i = _run(engine, calc, mags, vecs, kw, w, direct)
            if lr == 0:
                assert engine.lowrank_launches() == n0
            elif not disp:
                assert engine.lowrank_launches() > n0                  # the weighted k-path took the route
            err = rel_max(got_i, ref_i)
            print(f"{kind} {mode} lowrank={lr}: rel_max {err:.3e}")
            assert err <= 1e-5
        assert rel_max(got[1], got[0]) <= 1e-6
    finally:
        reset(engine)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_parity_golden_trajectories(engine, trajs, name):
    d = trajs[name]
    calc = make_calculator(d).attach(engine=engine)
    traj = calc.traj
    w = np.random.default_rng(1).uniform(-3.0, 30.0, traj.n_atoms).astype(np.float32)
    types = [int(t) for t in np.unique(traj.types)]
    for n_k in (8, 40):
        mags, vecs = calc.get_k_path([1, 1, 0], 2.0, n_k)
        for kw in ({}, dict(basis_atom_types=types, summation_mode="incoherent")):
            incoh = bool(kw) and len(types) > 1
            groups = [np.flatnonzero(traj.types == t) for t in types] if incoh else None
            ref = weighted_reference(traj, vecs, w, groups, False, incoh)
            got = calc.calculate(mags, vecs, atom_weights=w, **kw)
            err = rel_max(_inten(got), ref if incoh else np.sum(np.abs(ref) ** 2, axis=-1))
            assert err <= 1e-5, (name, n_k, kw, err)
    engine.invalidate()


# ---------------------------------------------------------------------------------------------------------------------
def test_paths_agree(engine, syn):
    from psa_amd import _hip
    calc, traj = syn["calcs"][False], syn["traj"]
    w = _weights("mass", traj)
    T, N = traj.n_frames, traj.n_atoms
    try:
        reset(engine)
        # Gamma-symmetric grid: folded against every vector projected
        _, gvecs, shape = calc.get_k_grid("xy", (-1.5, 1.5), (-1.0, 1.0), 6, 6, 0.0)
        none = np.array([], np.float32)
        calc.calculate(none, gvecs, k_grid_shape=shape)
        folded = calc.calculate(none, gvecs, k_grid_shape=shape, atom_weights=w)
        engine.set_option(_hip.OPT_FOLD_PAIRS, 0)
        flat = calc.calculate(none, gvecs, k_grid_shape=shape, atom_weights=w)
        engine.set_option(_hip.OPT_FOLD_PAIRS, 1)
        assert rel_max(folded.sed, flat.sed) <= 1e-6

        # first call on a non-resident array (streamed upload) against the resident call
        mags, vecs = calc.get_k_path("100", 1.0, 200)
        engine.invalidate()
        streamed = calc.calculate(mags, vecs, atom_weights=w)
        resident = calc.calculate(mags, vecs, atom_weights=w)              # >= 192 vectors: psa_sed_calculate, pipelined
        assert rel_max(streamed.sed, resident.sed) <= 1e-6
        engine.set_atom_weights(w)                                          # project + finalize: one block
        try:
            engine.project(_hip.SLOT_VELOCITIES, calc._mean_positions(), vecs)
            blockwise = engine.finalize(T, len(vecs), False)
        finally:
            engine.set_atom_weights(None)
        assert rel_max(resident.sed, blockwise) <= 1e-6

        # only the weights change: nothing about the resident array is rebuilt
        engine.oneoff_stats()
        cache = engine.plane_cache()
        calc.calculate(mags, vecs, atom_weights=np.ones(N, np.float32))
        assert engine.plane_cache() == cache
        st = engine.oneoff_stats()
        assert st["split_planes"] == 0.0 and st["upload"] == 0.0, st

        # pre-FFT projection of frame pieces, and fs_project of the whole list, against all frames
        mean = calc._mean_positions()
        engine.set_atom_weights(w)
        try:
            whole = engine.debug_project_only(_hip.SLOT_VELOCITIES, mean, vecs)
            halves = (engine.debug_project_only(_hip.SLOT_VELOCITIES, mean, vecs, frames=(0, T // 2))
                      + engine.debug_project_only(_hip.SLOT_VELOCITIES, mean, vecs, frames=(T // 2, T - T // 2)))
            assert rel_max(halves, whole) <= 1e-6
            engine.fs_project(_hip.SLOT_VELOCITIES, mean, vecs, None, 0, T, 0, len(vecs))
            fs = engine.fs_read(0, len(vecs), T)
            assert rel_max(fs, whole) <= 1e-6
        finally:
            engine.set_atom_weights(None)
        unweighted = engine.debug_project_only(_hip.SLOT_VELOCITIES, mean, vecs)
        assert rel_max(whole, unweighted) > 1e-2                           # (the weights did something)
    finally:
        reset(engine)


def test_errors_leave_the_context_usable(engine, syn):
    from psa_amd import _hip
    calc, traj = syn["calcs"][False], syn["traj"]
    N = traj.n_atoms
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    reset(engine)
    ref = calc.calculate(mags, vecs)
    bad = np.ones(N, np.float32)
    bad[3] = np.nan
    with pytest.raises(ValueError):
        calc.calculate(mags, vecs, atom_weights=bad)
    with pytest.raises(ValueError):
        calc.calculate(mags, vecs, atom_weights=np.ones(N + 1, np.float32))
    with pytest.raises(ValueError):
        engine.set_atom_weights(bad)
    lib = engine._lib
    assert lib.psa_set_atom_weights(engine._h, bad.ctypes.data_as(_hip._f32p), N) == -1     # PSA_EINVAL
    # weights of another length than the slot's atoms: the projection refuses
    engine.set_atom_weights(np.ones(N + 8, np.float32))
    try:
        with pytest.raises(_hip.PsaHipError, match="rc=-1"):
            engine.project(_hip.SLOT_VELOCITIES, calc._mean_positions(), vecs)
    finally:
        engine.set_atom_weights(None)
    again = calc.calculate(mags, vecs)
    assert np.array_equal(_bits(again.sed), _bits(ref.sed))
    zero = calc.calculate(mags, vecs, atom_weights=np.zeros(N, np.float32))
    assert not np.any(zero.sed) and not np.any(_inten(zero))
