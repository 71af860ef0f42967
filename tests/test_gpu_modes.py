"""The mode-projected SED on the GPU (psa_sed_modes, `calculate_mode_sed`): the contraction kernel alone against its
derived per-element bound (tests/modes64.py); end to end against the float64 restatement; the identities that tie it to
`calculate` (Cartesian and union vectors, completeness, homogeneity, the planted mode, the low-rank k-path route);
blocking, determinism, isolation from the SED entry points; ABI errors.

Measured on one MI355X (each test prints its figures): kernel alone 5.3 .. 10.6 u per element against bounds of 22 .. 490 u;
end to end rel_max 8.8e-8 .. 5.0e-7 over the 32 cases, per element (reported only) 6 .. 41 u of A^2 in velocity mode and
900 .. 6100 u in displacement mode; identities <= 4.3e-7; low-rank route 8 launches, 4.0e-7 to float64; the three
blockings bit-identical."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu

B_SITES = 8
MASSES = {1: 1.0, 2: 207.0}


def _trajectory(cells=(4, 4, 4), T=256, seed=3):
    """Synthetic silicon with a planted mode: 512 atoms, 8 basis sites (the trajectory of tests/test_gpu_vdos.py)."""
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
    from oracle import psa_oracle as O
    from psa_amd import SEDCalculator, mass_weights, site_groups
    out = {}
    for T in (256, 100):
        tr, cells = _trajectory(T=T)
        calcs = {disp: SEDCalculator(tr, *cells, use_displacements=disp).attach(engine=engine) for disp in (False, True)}
        path = calcs[False].get_k_path("100", 1.0, 24)
        rng = np.random.default_rng(17)
        scattered = (rng.standard_normal((7, 3)) * 1.2).astype(np.float32)
        out[T] = dict(traj=tr, calcs=calcs, groups=site_groups(np.arange(tr.n_atoms) % B_SITES), mean=O.mean_positions(tr.positions),
                      weights=mass_weights(tr.types, MASSES),
                      klists={"path": path, "scattered": (np.linalg.norm(scattered, axis=1).astype(np.float32), scattered)})
    reset(engine)
    yield out
    reset(engine)
    engine.invalidate()


def _lists(groups):
    return [g.tolist() for g in groups]


# ------------------------------------------------------------------------------------------------- 1. the kernel alone
def test_kernel_against_the_derived_bound(engine):
    """psa_debug_mode_power on uploaded complex64 spectra: |Phi_gpu - Phi_64| <= (12 B + 10) u A^2 per element (derived in
    tests/modes64.py; the proof that this can fail is tests/test_modes_host.py)"""
    import modes64 as M64
    for B, M, T, K in M64.CASES:
        S, eig = M64.kernel_case(B, M, T, K)
        got = engine.debug_mode_power(S, eig)
        ref, A = M64.contract64(S, eig)
        assert got.shape == (T, K, M) and got.dtype == np.float32
        err = M64.per_element(got, ref, A)
        print(f"B={B} M={M} T={T} K={K}: {err / M64.U:.1f} u per element, bound {M64.bound(B) / M64.U:.0f} u, rel_max {rel_max(got, ref):.2e}")
        assert err <= M64.bound(B)


# ------------------------------------------------------------------------------------------------- 2. end to end
_S64 = {}


def _reference(syn, T, klist, weighted, disp):
    """(spectra64 of the 8 sites, cached per configuration)"""
    import modes64 as M64
    key = (T, klist, weighted, disp)
    if key not in _S64:
        s = syn[T]
        tr = s["traj"]
        _S64[key] = M64.spectra64(tr.positions if disp else tr.velocities, s["mean"], s["klists"][klist][1], s["groups"],
                                  s["weights"] if weighted else None, disp)
    return _S64[key]


def _eig(K, M, seed=5):
    import modes64 as M64
    return M64.random_unitary(np.random.default_rng(seed), K, B_SITES, M)


@pytest.mark.parametrize("disp", [False, True], ids=["velocities", "displacements"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "mass"])
@pytest.mark.parametrize("M", [24, 5])
@pytest.mark.parametrize("klist", ["path", "scattered"])
@pytest.mark.parametrize("T", [256, 100])
def test_parity_float64(engine, syn, T, klist, M, weighted, disp):
    import modes64 as M64
    s = syn[T]
    mags, vecs = s["klists"][klist]
    eig = _eig(len(vecs), M)
    got = s["calcs"][disp].calculate_mode_sed(mags, vecs, eig, s["groups"], atom_weights=s["weights"] if weighted else None)
    ref, A = M64.contract64(_reference(syn, T, klist, weighted, disp), eig)
    assert got.sed.shape == (T, len(vecs), M) and got.sed.dtype == np.float32 and len(got.groups) == B_SITES
    assert np.array_equal(got.freqs, np.fft.fftfreq(T, d=s["calcs"][disp].dt_ps))
    err = rel_max(got.sed, ref)
    print(f"T={T} {klist} M={M} mass={weighted} disp={disp}: rel_max {err:.3e}; per element (reported) "
          f"{M64.per_element(got.sed, ref, A) / M64.U:.1f} u of A^2")
    assert err <= 1e-5
    assert engine.segment_length == 0


# ------------------------------------------------------------------------------------------------- 3. identities
def test_cartesian_vectors_are_the_group_spectra(engine, syn):
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["path"], s["groups"]
    K = len(vecs)
    eig = np.zeros((K, 3 * B_SITES, B_SITES, 3), np.complex64)
    for b in range(B_SITES):
        for c in range(3):
            eig[:, 3 * b + c, b, c] = 1.0
    phi = calc.calculate_mode_sed(mags, vecs, eig, groups).sed
    for b in range(B_SITES):
        one = calc.calculate(mags, vecs, basis_atom_indices=groups[b].tolist()).sed
        err = rel_max(phi[:, :, 3 * b:3 * b + 3], np.abs(one.astype(np.complex128)) ** 2)
        print(f"Cartesian vectors, site {b}: rel_max {err:.3e}")
        assert err <= 1e-5


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "mass"])
def test_union_vectors_are_the_coherent_spectrum(engine, syn, weighted):
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["scattered"], s["groups"]
    w = s["weights"] if weighted else None
    eig = np.zeros((len(vecs), 3, B_SITES, 3), np.complex64)
    for c in range(3):
        eig[:, c, :, c] = 1.0
    phi = calc.calculate_mode_sed(mags, vecs, eig, groups, atom_weights=w).sed
    whole = calc.calculate(mags, vecs, atom_weights=w).sed
    err = rel_max(phi, np.abs(whole.astype(np.complex128)) ** 2)
    print(f"union vectors, mass={weighted}: rel_max {err:.3e}")
    assert err <= 1e-5


def test_completeness(engine, syn):
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["path"], s["groups"]
    phi = calc.calculate_mode_sed(mags, vecs, _eig(len(vecs), 24), groups).sed
    inco = calc.calculate(mags, vecs, basis_atom_indices=_lists(groups), summation_mode="incoherent").sed
    assert inco.shape == phi.shape[:2]
    err = rel_max(np.sum(phi.astype(np.float64), axis=-1), inco)
    print(f"completeness: rel_max {err:.3e}")
    assert err <= 1e-5


def test_homogeneity(engine, syn):
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["scattered"], s["groups"]
    eig = _eig(len(vecs), 24)
    base = calc.calculate_mode_sed(mags, vecs, eig, groups).sed
    rng = np.random.default_rng(8)
    phase = np.exp(2j * np.pi * rng.random((len(vecs), 24, 1, 1)))
    turned = calc.calculate_mode_sed(mags, vecs, (eig * phase).astype(np.complex64), groups).sed
    err = rel_max(turned, base)
    print(f"unit phase per (k, nu): rel_max {err:.3e}")
    assert err <= 1e-5
    assert np.isfinite(base).all() and base[base > 0].min() > 1e-30 and base.max() < 1e30
    doubled = calc.calculate_mode_sed(mags, vecs, np.complex64(2) * eig, groups).sed
    assert np.array_equal(doubled.view(np.uint32), (np.float32(4) * base).view(np.uint32))


def test_planted_mode(engine, syn):
    """the x-polarised planted wave (amplitude 3, bin 16, k* = 0.25 * 2 pi / a along x) answers to the vector x/sqrt(B)"""
    from psa_amd import synth
    s = syn[256]
    calc, groups, T = s["calcs"][False], s["groups"], 256
    vecs = np.float32([[0.1, 0.2, 0.0], [2 * np.pi / synth.A_SI * 0.25, 0, 0], [0.9, 0.0, 0.3]])
    n = 3 * B_SITES
    rng = np.random.default_rng(12)
    eig = np.empty((3, n, B_SITES, 3), np.complex64)
    for k in range(3):
        m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        m[:, 0] = 0.0
        m[0::3, 0] = 1.0                                  # x on every site: column 0 of Q is x / sqrt(B) up to a sign
        q = np.linalg.qr(m)[0]
        eig[k] = q.T.reshape(n, B_SITES, 3)
    assert np.allclose(np.abs(eig[:, 0, :, 0]), 1 / np.sqrt(B_SITES), atol=1e-6) and np.allclose(eig[:, 0, :, 1:], 0, atol=1e-6)
    phi = calc.calculate_mode_sed(np.linalg.norm(vecs, axis=1), vecs, eig, groups).sed
    w_star = int(np.argmax(phi[:, 1, 0]))
    assert w_star in (16, T - 16)
    assert int(np.argmax(phi[w_star, 1, :])) == 0


def test_lowrank_route_on_a_k_path(engine, syn):
    """256 k-vectors on [100]: every site group has a low-rank plan (checked on the host), its planes are built on
    first sight (PSA_OPT_PLANES_EAGER), the route serves all 8 projections; the result meets float64, and the dense
    route on the same list agrees with it"""
    import modes64 as M64
    from psa_amd import _hip
    s = syn[256]
    calc, groups, tr = s["calcs"][False], s["groups"], s["traj"]
    mags, vecs = calc.get_k_path("100", 1.0, 256)
    assert all(_hip.lowrank_plan(vecs, s["mean"], g) is not None for g in groups)
    eig = _eig(256, 24, seed=6)
    try:
        engine.set_option(_hip.OPT_PLANES_EAGER, 1)
        n0 = engine.lowrank_launches()
        low = calc.calculate_mode_sed(mags, vecs, eig, groups).sed
        taken = engine.lowrank_launches() - n0
        ref = M64.mode_sed64(tr.velocities, s["mean"], vecs, groups, eig)
        err = rel_max(low, ref)
        engine.set_option(_hip.OPT_K1_LOWRANK, 0)
        n0 = engine.lowrank_launches()
        dense = calc.calculate_mode_sed(mags, vecs, eig, groups).sed
        assert engine.lowrank_launches() == n0
        err_d = rel_max(dense, low)
        print(f"low-rank route: {taken} launches, rel_max to float64 {err:.3e}, dense route to it {err_d:.3e}")
        assert taken == B_SITES
        assert err <= 1e-5 and err_d <= 1e-5
    finally:
        reset(engine)


# ------------------------------------------------------------------------------------------------- 4. blocking, isolation
def test_blocking_determinism_and_budget(engine, syn):
    import modes64 as M64
    from psa_amd import _hip
    s = syn[256]
    calc, (mags, vecs), groups, tr = s["calcs"][False], s["klists"]["path"], s["groups"], s["traj"]
    eig = _eig(len(vecs), 24)
    ref = M64.contract64(_reference(syn, 256, "path", False, False), eig)[0]
    per_k = 24 * B_SITES * 256                               # bytes of one k-vector in the stacked buffer
    got = {}
    try:
        for name, budget in (("one block", 4 << 30), ("five blocks", 5 * per_k + 100), ("24 blocks", per_k)):
            engine.set_option(_hip.OPT_MODES_WORK_BYTES, budget)
            a = calc.calculate_mode_sed(mags, vecs, eig, groups).sed
            b = calc.calculate_mode_sed(mags, vecs, eig, groups).sed
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))          # two identical calls
            got[name] = (a.copy(), rel_max(a, ref))
            print(f"{name}: rel_max to float64 {got[name][1]:.3e}")
            assert got[name][1] <= 1e-5
        names = list(got)
        for i, x in enumerate(names):
            for y in names[i + 1:]:
                d = float(np.max(np.abs(got[x][0].astype(np.float64) - got[y][0]))) / float(np.max(np.abs(ref)))
                same = np.array_equal(got[x][0].view(np.uint32), got[y][0].view(np.uint32))
                print(f"{x} vs {y}: distance {d:.3e} (bit-identical: {same})")
                assert d <= got[x][1] + got[y][1]
        engine.set_option(_hip.OPT_MODES_WORK_BYTES, per_k - 1)
        with pytest.raises(_hip.PsaHipError, match=str(per_k)):
            calc.calculate_mode_sed(mags, vecs, eig, groups)
    finally:
        reset(engine)
    assert np.array_equal(calc.calculate_mode_sed(mags, vecs, eig, groups).sed.view(np.uint32), got["one block"][0].view(np.uint32))


def test_no_leak_into_sed_calls(engine, syn):
    from psa_amd import _hip
    s = syn[256]
    calc, (mags, vecs), groups, tr = s["calcs"][False], s["klists"]["path"], s["groups"], s["traj"]
    eig = _eig(len(vecs), 5)
    for kw in ({}, dict(basis_atom_types=[1, 2], summation_mode="incoherent")):
        before = calc.calculate(mags, vecs, **kw)
        calc.calculate_mode_sed(mags, vecs, eig, groups, atom_weights=s["weights"])
        after = calc.calculate(mags, vecs, **kw)
        assert after.sed.shape == before.sed.shape and after.sed.dtype == before.sed.dtype
        assert np.array_equal(after.sed.view(np.uint8), before.sed.view(np.uint8))
    # a projection that has not been finalized yet survives a mode call
    engine.project(_hip.SLOT_VELOCITIES, s["mean"], vecs, None, 0)
    whole = np.array(engine.finalize(tr.n_frames, len(vecs), False))
    engine.project(_hip.SLOT_VELOCITIES, s["mean"], vecs, None, 0)
    calc.calculate_mode_sed(mags, vecs, eig, groups)
    later = engine.finalize(tr.n_frames, len(vecs), False)
    assert np.array_equal(np.asarray(later).view(np.uint8), whole.view(np.uint8))
    assert engine.segment_length == 0
    # the weights of the mode call are gone: an unweighted call gives the unweighted bits
    plain = calc.calculate_mode_sed(mags, vecs, eig, groups).sed
    calc.calculate_mode_sed(mags, vecs, eig, groups, atom_weights=s["weights"])
    assert np.array_equal(calc.calculate_mode_sed(mags, vecs, eig, groups).sed.view(np.uint32), plain.view(np.uint32))


def test_empty_group_and_all_atoms(engine, syn):
    """straight through the engine: an empty group contributes nothing; NULL groups with B = 1 are all atoms"""
    import modes64 as M64
    from psa_amd import _hip
    s = syn[256]
    tr, (mags, vecs) = s["traj"], s["klists"]["scattered"]
    engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
    rng = np.random.default_rng(21)
    groups = [np.array([301, 5, 17, 131, 2]), np.array([], int), np.arange(9, 400, 3)]
    eig = M64.random_unitary(rng, len(vecs), 3, 4)
    got = engine.sed_modes(_hip.SLOT_VELOCITIES, s["mean"], vecs, groups, eig)
    err = rel_max(got, M64.mode_sed64(tr.velocities, s["mean"], vecs, groups, eig))
    e1 = M64.random_unitary(rng, len(vecs), 1)
    err1 = rel_max(engine.sed_modes(_hip.SLOT_VELOCITIES, s["mean"], vecs, None, e1),
                   M64.mode_sed64(tr.velocities, s["mean"], vecs, [None], e1))
    print(f"index lists with an empty group: rel_max {err:.3e}; all atoms: {err1:.3e}")
    assert err <= 1e-5 and err1 <= 1e-5


def test_abi_errors(engine, syn):
    import modes64 as M64
    from psa_amd import Segments, _hip
    s = syn[256]
    tr, (mags, vecs) = s["traj"], s["klists"]["scattered"]
    T, N, K, M = tr.n_frames, tr.n_atoms, len(vecs), 4
    engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
    lib, h = engine._lib, engine._h
    mean = np.ascontiguousarray(s["mean"], np.float32)
    kv = np.ascontiguousarray(vecs, np.float32)
    good_eig = M64.random_unitary(np.random.default_rng(1), K, 2, M)
    two = ([0, 1, 2, 3], [0, 2, 4])

    def call(idx=two[0], off=two[1], B=2, eig=good_eig, M=M, nbytes=None, out="alloc"):
        o = np.zeros((T, K, max(M, 1)), np.float32) if isinstance(out, str) else out
        ip = None if idx is None else np.ascontiguousarray(idx, np.int32)
        op = None if off is None else np.ascontiguousarray(off, np.int64)
        rc = lib.psa_sed_modes(h, _hip.SLOT_VELOCITIES, mean.ctypes.data_as(_hip._f32p), kv.ctypes.data_as(_hip._f32p), K,
                               None if ip is None else ip.ctypes.data_as(_hip._i32p),
                               None if op is None else op.ctypes.data_as(_hip._i64p), B,
                               None if eig is None else eig.ctypes.data_as(C.c_void_p), M, 0,
                               None if o is None else o.ctypes.data_as(_hip._f32p),
                               C.c_size_t((0 if o is None else o.nbytes) if nbytes is None else nbytes))
        return rc, lib.psa_last_error()

    def refused(what, **kw):
        rc, msg = call(**kw)
        assert rc == -1 and len(msg) > 0, (what, rc, msg)
        return msg

    assert b"eig" in refused("eig null", eig=None)
    refused("out_host null", out=None, nbytes=4 * T * K * M)
    refused("M < 1", M=0)
    bad = good_eig.copy()
    bad[2, 1, 1, 0] = np.inf
    assert b"finite" in refused("non-finite eig", eig=bad)
    assert b"disjoint" in refused("an atom in two groups", idx=[0, 1, 1, 2])
    refused("index out of range", idx=[0, 1, 2, N])
    refused("negative index", idx=[0, -1, 2, 3])
    assert b"out_bytes" in refused("out_bytes not exact", nbytes=4 * T * K * M - 4)
    refused("NULL list means one group", idx=None, off=None)
    engine.set_segments(Segments(64, 32))
    try:
        assert b"segment" in refused("segments set")
    finally:
        engine.set_segments(None)
    engine.set_atom_weights(np.ones(N + 1, np.float32))
    try:
        assert b"weights" in refused("weights of another length")
    finally:
        engine.set_atom_weights(None)
    engine.set_option(_hip.OPT_MODES_WORK_BYTES, 24 * 2 * T - 1)
    try:
        assert str(24 * 2 * T).encode() in refused("budget below one k-vector")
    finally:
        reset(engine)
    out = np.zeros((T, K, M), np.float32)                                     # the context is usable afterwards
    rc, _ = call(out=out)
    assert rc == 0
    groups = [np.array([0, 1]), np.array([2, 3])]
    assert rel_max(out, M64.mode_sed64(tr.velocities, s["mean"], vecs, groups, good_eig)) <= 1e-5
