"""The spectral covariance and the mode vectors on the GPU (psa_sed_covariance, `calculate_spectral_covariance`,
`calculate_mode_vectors`): the covariance kernels alone on exact integer data (the operand lane map of the fp32 matrix
core, every tile shape, every boundary of the summation structure) and against their derived per-component bound
(tests/cov64.py); end to end against the float64 restatement; the identities that tie it to `calculate` and
`calculate_mode_sed`; planted modes recovered from a trajectory; blocking, determinism, isolation; ABI errors.

Measured on one MI355X (each test prints its figures): exact data bit-equal for all 540 shapes; kernel alone 11.3 .. 23.3 u per
component against the bound of 292 u; end to end rel_max per k-point matrix 4.7e-7 .. 1.2e-6 over the 16 cases (per component,
reported only: 9 .. 53 u of A); identities <= 8.6e-7; planted modes |f - f_bin| <= 0.0066 df, overlap >= 0.999896,
sin(angle) to the float64 vectors 4.3e-7 .. 1.2e-5 against Davis-Kahan bounds of 1.5e-5 .. 2.0e-4; the three blockings
bit-identical."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu

B_SITES = 8
MASSES = {1: 1.0, 2: 207.0}


# ------------------------------------------------------------------------------------------------- 1. exact data
def _boundary_lengths():
    from psa_amd import _hip
    marks = (4, _hip.COV_TILE, _hip.COV_CHAIN, _hip.COV_CHAIN * _hip.COV_FOLDS, _hip.COV_CHUNK, 2 * _hip.COV_CHUNK)
    return sorted({t + d for t in marks for d in (-1, 0, 1)})


def _exact64(S, g):
    """(n_w, K, n, n) complex128 of integer spectra and weights: float64 matrix products, exact below 2^53"""
    B, K, _, T = S.shape
    X = S.transpose(1, 0, 2, 3).reshape(K, 3 * B, T)
    xr, xi = X.real.astype(np.float64), X.imag.astype(np.float64)
    out = np.empty((g.shape[0], K, 3 * B, 3 * B), np.complex128)
    for m in range(g.shape[0]):
        gr, gi = xr * g[m].astype(np.float64), xi * g[m].astype(np.float64)
        out[m] = (xr @ gr.transpose(0, 2, 1) + xi @ gi.transpose(0, 2, 1)) + 1j * (xi @ gr.transpose(0, 2, 1) - xr @ gi.transpose(0, 2, 1))
    return out


@pytest.mark.parametrize("T", _boundary_lengths())
def test_exact_integer_data(engine, T):
    """Integer real and imaginary parts in [-8, 8], weights in {0, 1, 2, 4}, scale 1: every partial and total sum stays
    below 2^24 (2 x 8 x 8 x 4 x 8193 < 2^22.1), so float32 sums are exact and the float64 reference must be matched bit for
    bit -- real and imaginary part, every (i, j): a wrong lane map, tile pair, sign, weight row or boundary cannot hide.
    n = 3, 6, 15, 24, 33, 96 covers partial and full 16-row blocks and the cap; K = 1, 3, 5; n_w = 1, 2."""
    rng = np.random.default_rng(T)
    assert 2 * 8 * 8 * 4 * T < 2 ** 24
    for B in (1, 2, 5, 8, 11, 32):
        S5 = (rng.integers(-8, 9, (B, 5, 3, T)) + 1j * rng.integers(-8, 9, (B, 5, 3, T))).astype(np.complex64)
        g2 = rng.choice(np.float32([0, 1, 2, 4]), (2, T))
        for K in (1, 3, 5):
            S = np.ascontiguousarray(S5[:, 5 - K:])
            for n_w in (1, 2):
                g = np.ascontiguousarray(g2[2 - n_w:])
                got = engine.debug_covariance(S, g, 1.0)
                ref = _exact64(S, g)
                assert got.shape == ref.shape == (n_w, K, 3 * B, 3 * B) and got.dtype == np.complex128
                assert np.array_equal(got.real, ref.real) and np.array_equal(got.imag, ref.imag), (B, K, n_w, T)
                up, low = got.transpose(0, 1, 3, 2), got
                assert np.array_equal(up.real.view(np.uint64), low.real.view(np.uint64))               # G[j,i] = conj G[i,j] ...
                assert np.array_equal(up.imag, -low.imag)                                              # ... bit for bit
                d = np.einsum("mkii->mki", got)
                assert not d.imag.any() and not np.signbit(d.imag).any()                               # Im G[i,i] = +0
    # the scale is applied in float64: a power of two, and 1/T^2
    got = engine.debug_covariance(S, g, 1.0 / (T * T))
    assert np.array_equal(got, ref * (1.0 / (T * T)))


# ------------------------------------------------------------------------------------------------- 2. the bound
@pytest.mark.parametrize("B,T,K", [(1, 192, 3), (2, 300, 5), (8, 4097, 3), (11, 8200, 3), (32, 200, 3)])
def test_kernel_against_the_derived_bound(engine, B, T, K):
    """psa_debug_covariance on the generator's complex64 spectra: per real component |G_gpu - G_64| <= bound() A (derived
    in tests/cov64.py; the proof that this can fail is tests/test_cov_host.py)"""
    import cov64 as C64
    S, g = C64.kernel_case(B, T, K, 2)
    got = engine.debug_covariance(S, g, 1.0 / (T * T))
    ref, A = C64.cov64(S, g, 1.0 / (T * T))
    err = C64.per_component(got, ref, A)
    print(f"B={B} T={T} K={K}: {err / C64.U:.1f} u per component, bound {C64.bound() / C64.U:.0f} u, rel_max {rel_max(got, ref):.2e}")
    assert err <= C64.bound()


# ------------------------------------------------------------------------------------------------- 3. end to end
def _trajectory(cells=(4, 4, 4), T=256, seed=3):
    """Synthetic silicon with a planted mode: 512 atoms, 8 basis sites (the trajectory of tests/test_gpu_modes.py)."""
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


_S64 = {}


def _reference(syn, T, klist, weighted, disp):
    """(spectra64 of the 8 sites, cached per configuration and left unchanged)"""
    import modes64 as M64
    key = (T, klist, weighted, disp)
    if key not in _S64:
        s = syn[T]
        tr = s["traj"]
        _S64[key] = M64.spectra64(tr.positions if disp else tr.velocities, s["mean"], s["klists"][klist][1], s["groups"],
                                  s["weights"] if weighted else None, disp)
    return _S64[key]


def _moment_rows(calc, T, disp):
    from psa_amd import spectral_weights
    return np.stack([spectral_weights(T, calc.dt_ps, m) for m in ((0, 2) if disp else (-2, 0))])


@pytest.mark.parametrize("disp", [False, True], ids=["velocities", "displacements"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "mass"])
@pytest.mark.parametrize("klist", ["path", "scattered"])
@pytest.mark.parametrize("T", [256, 100])
def test_parity_float64(engine, syn, T, klist, weighted, disp):
    """both moments of the calculator's kind in one call, rel_max <= 1e-5 per k-point matrix"""
    import cov64 as C64
    s = syn[T]
    mags, vecs = s["klists"][klist]
    calc = s["calcs"][disp]
    g = _moment_rows(calc, T, disp)
    got = calc.calculate_spectral_covariance(mags, vecs, s["groups"], atom_weights=s["weights"] if weighted else None, freq_weights=g)
    ref, A = C64.cov64(_reference(syn, T, klist, weighted, disp), g)
    n = 3 * B_SITES
    assert got.shape == (2, len(vecs), n, n) and got.dtype == np.complex128
    worst = max(rel_max(got[m, k], ref[m, k]) for m in range(2) for k in range(len(vecs)))
    print(f"T={T} {klist} mass={weighted} disp={disp}: worst k-point matrix rel_max {worst:.3e}; per component (reported) "
          f"{C64.per_component(got, ref, A) / C64.U:.1f} u of A")
    assert worst <= 1e-5
    assert engine.segment_length == 0


# ------------------------------------------------------------------------------------------------- 4. identities
def test_trace_is_the_group_intensity(engine, syn):
    """g = 1: sum_c G[(b,c),(b,c)] is the frequency sum of the complex `calculate` intensity of group b"""
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["path"], s["groups"]
    G = calc.calculate_spectral_covariance(mags, vecs, groups, freq_weights=np.ones(256))[0]
    for b in range(B_SITES):
        one = calc.calculate(mags, vecs, basis_atom_indices=groups[b].tolist()).sed.astype(np.complex128)    # (T, K, 3)
        want = np.sum(np.abs(one) ** 2, axis=(0, 2))
        have = np.real(sum(G[:, 3 * b + c, 3 * b + c] for c in range(3)))
        err = rel_max(have, want)
        print(f"site {b}: rel_max {err:.3e}")
        assert err <= 1e-5


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "mass"])
def test_quadratic_form_is_the_weighted_mode_sed(engine, syn, weighted):
    """sum_w g calculate_mode_sed(...)[w,k,nu] = e_nu^+ G e_nu for random unitary vectors"""
    import modes64 as M64
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["scattered"], s["groups"]
    w = s["weights"] if weighted else None
    g = _moment_rows(calc, 256, False)
    e = M64.random_unitary(np.random.default_rng(5), len(vecs), B_SITES)
    G = calc.calculate_spectral_covariance(mags, vecs, groups, atom_weights=w, freq_weights=g)
    phi = calc.calculate_mode_sed(mags, vecs, e, groups, atom_weights=w).sed.astype(np.float64)
    v = e.reshape(len(vecs), 3 * B_SITES, 3 * B_SITES).astype(np.complex128)
    for m in range(2):
        quad = np.real(np.einsum("kni,kij,knj->kn", np.conj(v), G[m], v))
        err = rel_max(quad, np.einsum("w,wkn->kn", g[m].astype(np.float64), phi))
        print(f"moment row {m}, mass={weighted}: rel_max {err:.3e}")
        assert err <= 1e-5


# ------------------------------------------------------------------------------------------------- 5. planted modes
PLANTED_BINS = (20, 33, 47, 60, 81, 100)


def _planted():
    """cells (4,4,2), two sites per cell at (0,0,0) and (1/4,1/4,1/4) a, a = 5, masses 1 and 4, T = 512, dt = 0.002 ps;
    three commensurate k-vectors with 2k no reciprocal lattice vector; six modes per k with random unitary vectors on
    exact FFT bins, amplitudes 1.0 .. 4.6; v_a = Re[A e_b exp(-i k.r_a) exp(i w t + i phi)] / sqrt(m_b) plus Gaussian
    noise 0.01; positions constant"""
    from psa_amd import Trajectory
    cells, a, T, dt = (4, 4, 2), 5.0, 512, 0.002
    rng = np.random.default_rng(42)
    ii, jj, kk = np.meshgrid(*(np.arange(c) for c in cells), indexing="ij")
    origin = np.stack([ii, jj, kk], axis=-1).reshape(-1, 1, 3).astype(np.float64)
    r0 = ((origin + np.array([[0, 0, 0], [.25, .25, .25]])[None]) * a).reshape(-1, 3)      # cell-major, basis-minor
    N = len(r0)
    site = np.arange(N) % 2
    types = (site + 1).astype(np.int32)
    mass = np.where(site == 0, 1.0, 4.0)
    kv = np.array([[1, 0, 0], [1, 2, 0], [3, 1, 1]], np.float64) * 2 * np.pi / (a * np.array(cells))
    amps = np.linspace(1.0, 4.6, 6)
    t = np.arange(T)
    vel = 0.01 * rng.standard_normal((T, N, 3))
    vectors = np.empty((3, 6, 2, 3), np.complex128)
    for k in range(3):
        z = rng.standard_normal((6, 6)) + 1j * rng.standard_normal((6, 6))
        vectors[k] = np.linalg.qr(z)[0].T.reshape(6, 2, 3)                                  # rows: modes
        for nu in range(6):
            wave = amps[nu] * np.exp(2j * np.pi * PLANTED_BINS[nu] * t / T + 2j * np.pi * rng.random())            # (T,)
            per_atom = vectors[k, nu][site] * np.exp(-1j * (r0 @ kv[k]))[:, None] / np.sqrt(mass)[:, None]         # (N, 3)
            vel += np.real(wave[:, None, None] * per_atom[None])
    pos = np.broadcast_to(r0.astype(np.float32)[None], (T, N, 3)).copy()
    box = np.diag([c * a for c in cells]).astype(np.float32)
    tr = Trajectory(pos, vel.astype(np.float32), types, np.arange(T, dtype=np.float32), box, np.diag(box).copy(),
                    np.zeros(3, np.float32), dt)
    return tr, cells, kv.astype(np.float32), vectors, site


def test_planted_modes_are_recovered(engine):
    import cov64 as C64
    from psa_amd import SEDCalculator, mass_weights, mode_vectors, site_groups, spectral_weights
    tr, cells, kv, planted, site = _planted()
    T, df = tr.n_frames, 1.0 / (tr.n_frames * 0.002)
    calc = SEDCalculator(tr, *cells).attach(engine=engine)
    groups = site_groups(site)
    w = mass_weights(tr.types, {1: 1.0, 2: 4.0})
    mags = np.linalg.norm(kv, axis=1).astype(np.float32)
    try:
        mv = calc.calculate_mode_vectors(mags, kv, groups, atom_weights=w)
        assert mv.eigenvectors.shape == (3, 6, 2, 3) and mv.ok.all()
        want_f = np.array(PLANTED_BINS) * df
        e = mv.eigenvectors.reshape(3, 6, 6).astype(np.complex128)
        overlap = np.abs(np.einsum("kni,kni->kn", np.conj(planted.reshape(3, 6, 6)), e))
        print(f"planted modes: max |f - f_bin| = {np.max(np.abs(mv.frequency - want_f)) / df:.4f} df, min overlap {overlap.min():.6f}")
        assert np.all(np.abs(mv.frequency - want_f[None]) <= df / 10)
        assert overlap.min() >= 0.999
        phi = calc.calculate_mode_sed(mags, kv, mv.eigenvectors, groups, atom_weights=w).sed
        assert np.array_equal(np.argmax(phi, axis=0), np.broadcast_to(np.array(PLANTED_BINS), (3, 6)))
        # against the float64 covariance of the same trajectory: Davis-Kahan, sin(angle) <= 2 ||G_gpu - G_64||_2 / gap
        g = np.stack([spectral_weights(T, 0.002, -2), spectral_weights(T, 0.002, 0)])
        mean = np.mean(tr.positions, axis=0, dtype=np.float32)
        G64 = C64.covariance64(tr.velocities, mean, kv, groups, g, w)[0]
        ref = mode_vectors(G64[0], G64[1])
        r = ref.eigenvectors.reshape(3, 6, 6).astype(np.complex128)
        for k in range(3):
            dist = np.linalg.norm(mv.displacement_covariance[k] - G64[0, k], 2)
            lam = ref.eigenvalues[k]
            for nu in range(6):
                gap = np.min(np.abs(np.delete(lam, nu) - lam[nu]))
                rn, en = r[k, nu] / np.linalg.norm(r[k, nu]), e[k, nu] / np.linalg.norm(e[k, nu])
                sin = np.linalg.norm(en - np.vdot(rn, en) * rn)
                print(f"k {k} mode {nu}: sin(angle) {sin:.2e}, Davis-Kahan {2 * dist / gap:.2e} (||dG|| {dist:.2e}, gap {gap:.2e})")
                assert sin <= 2 * dist / gap + 1e-6
        print(f"frequencies against mode_vectors(cov64): max difference {np.max(np.abs(mv.frequency - ref.frequency)) / df:.2e} df")
    finally:
        reset(engine)
        engine.invalidate()


# ------------------------------------------------------------------------------------------------- 6. blocking, isolation
def test_blocking_determinism_and_isolation(engine, syn):
    from psa_amd import _hip
    import modes64 as M64
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["path"], s["groups"]
    g = _moment_rows(calc, 256, False)
    e = M64.random_unitary(np.random.default_rng(5), len(vecs), B_SITES, 5)
    run = lambda: calc.calculate_spectral_covariance(mags, vecs, groups, atom_weights=s["weights"], freq_weights=g)   # noqa: E731
    for _ in range(2):      # the plane cache settles on a group's second sight: what follows runs on the cached planes
        calc.calculate(mags, vecs), calc.calculate_mode_sed(mags, vecs, e, groups)
    sed0 = calc.calculate(mags, vecs).sed.copy()
    phi0 = calc.calculate_mode_sed(mags, vecs, e, groups).sed.copy()
    assert np.array_equal(calc.calculate(mags, vecs).sed.view(np.uint8), sed0.view(np.uint8))      # ... and repeats its bits
    one = run()
    assert np.array_equal(one.view(np.uint64), run().view(np.uint64))                    # two identical calls
    per_k = 24 * B_SITES * 256 + 2 * 3 * 2 * 256 * 4                                      # q and the slabs of one k-vector
    try:
        engine.set_option(_hip.OPT_MODES_WORK_BYTES, 8 * per_k + 100)                     # 24 k-vectors in three blocks
        blocked = run()
        assert np.array_equal(blocked.view(np.uint64), one.view(np.uint64))
        engine.set_option(_hip.OPT_MODES_WORK_BYTES, per_k)                               # one k-vector per block
        assert np.array_equal(run().view(np.uint64), one.view(np.uint64))
        engine.set_option(_hip.OPT_MODES_WORK_BYTES, per_k - 1)
        with pytest.raises(_hip.PsaHipError, match=str(per_k)):
            run()
    finally:
        reset(engine)
    # the SED entry points and the mode projection give the bits they gave before the covariance calls
    assert np.array_equal(calc.calculate(mags, vecs).sed.view(np.uint8), sed0.view(np.uint8))
    assert np.array_equal(calc.calculate_mode_sed(mags, vecs, e, groups).sed.view(np.uint32), phi0.view(np.uint32))
    assert engine.segment_length == 0


# ------------------------------------------------------------------------------------------------- 7. ABI errors
def test_abi_errors(engine, syn):
    import cov64 as C64
    from psa_amd import Segments, _hip
    s = syn[256]
    tr, (mags, vecs) = s["traj"], s["klists"]["scattered"]
    T, N, K = tr.n_frames, tr.n_atoms, len(vecs)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
    lib, h = engine._lib, engine._h
    mean = np.ascontiguousarray(s["mean"], np.float32)
    kv = np.ascontiguousarray(vecs, np.float32)
    good_g = np.ascontiguousarray(np.random.default_rng(1).random((2, T)), np.float32)
    two = ([0, 1, 2, 3], [0, 2, 4])

    def call(idx=two[0], off=two[1], B=2, g=good_g, n_w=2, nbytes=None, out="alloc", mean_=mean, kv_=kv):
        o = np.zeros((max(n_w, 1), K, 3 * B, 3 * B), np.complex128) if isinstance(out, str) else out
        ip = None if idx is None else np.ascontiguousarray(idx, np.int32)
        op = None if off is None else np.ascontiguousarray(off, np.int64)
        rc = lib.psa_sed_covariance(h, _hip.SLOT_VELOCITIES, None if mean_ is None else mean_.ctypes.data_as(_hip._f32p),
                                    None if kv_ is None else kv_.ctypes.data_as(_hip._f32p), K,
                                    None if ip is None else ip.ctypes.data_as(_hip._i32p),
                                    None if op is None else op.ctypes.data_as(_hip._i64p), B,
                                    None if g is None else g.ctypes.data_as(_hip._f32p), n_w, 0,
                                    None if o is None else o.ctypes.data_as(C.c_void_p),
                                    C.c_size_t((0 if o is None else o.nbytes) if nbytes is None else nbytes))
        return rc, lib.psa_last_error()

    def refused(what, **kw):
        rc, msg = call(**kw)
        assert rc == -1 and len(msg) > 0, (what, rc, msg)
        return msg

    assert b"n_w" in refused("n_w = 0", n_w=0)
    assert b"n_w" in refused("n_w = 3", n_w=3, g=np.ones((3, T), np.float32))
    bad = good_g.copy()
    bad[1, 7] = np.nan
    assert b"finite" in refused("non-finite weight", g=bad)
    many = np.arange(33 * 2, dtype=np.int32)
    assert b"96" in refused("3 B > 96", idx=many, off=np.arange(0, 67, 2), B=33)
    assert b"disjoint" in refused("overlapping groups", idx=[0, 1, 1, 2])
    refused("index out of range", idx=[0, 1, 2, N])
    assert b"out_bytes" in refused("out_bytes not exact", nbytes=16 * 2 * K * 36 - 16)
    assert b"freq_weights" in refused("null weights", g=None)
    assert b"output" in refused("null output", out=None, nbytes=16 * 2 * K * 36)
    assert b"mean" in refused("null mean", mean_=None)
    assert b"k_vectors" in refused("null k_vectors", kv_=None)
    engine.set_segments(Segments(64, 32))
    try:
        assert b"clear psa_set_segments first" in refused("segments set")
    finally:
        engine.set_segments(None)
    out = np.zeros((2, K, 6, 6), np.complex128)                                # the context is usable afterwards
    rc, _ = call(out=out)
    assert rc == 0
    groups = [np.array([0, 1]), np.array([2, 3])]
    ref = C64.covariance64(tr.velocities, s["mean"], vecs, groups, good_g)[0]
    assert max(rel_max(out[m, k], ref[m, k]) for m in range(2) for k in range(K)) <= 1e-5
    # the debug entry refuses what its kernels do not serve
    S = np.zeros((33, 1, 3, 8), np.complex64)
    o = np.zeros((1, 1, 99, 99), np.complex128)
    rc = lib.psa_debug_covariance(h, S.ctypes.data_as(C.c_void_p), 33, 1, 8, good_g.ctypes.data_as(_hip._f32p), 1, 1.0,
                                  o.ctypes.data_as(C.c_void_p))
    assert rc == -1 and b"96" in lib.psa_last_error()
