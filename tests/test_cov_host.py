"""The spectral covariance and the mode vectors without a GPU: the float64 restatement (tests/cov64.py) against the
identities that tie it to the projected series and to the mode-projected SED; the proof that the kernel's bound can
fail; `mode_vectors` on constructed covariances; `spectral_weights`; the binding; what `calculate_spectral_covariance`
and `calculate_mode_vectors` validate, resolve and hand to the engine (a small stand-in defined here that answers
`sed_covariance` with the restatement)."""
import sys
import threading
import types
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
for p in (str(HERE.parent), str(HERE), str(HERE / "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cov64 as C64                                                                    # noqa: E402
import modes64 as M64                                                                  # noqa: E402
from psa_amd import ModeVectors, _hip, mass_weights, mode_vectors, site_groups, spectral_weights   # noqa: E402
from ref64 import project64                                                            # noqa: E402


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _case64(seed=4, N=64, T=32, K=5, B=4):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((T, N, 3)).astype(np.float32)
    mean = (rng.random((N, 3)) * 11.0).astype(np.float32)
    k = (rng.standard_normal((K, 3)) * 0.8).astype(np.float32)
    groups = site_groups(np.arange(N) % B)
    w = (0.5 + rng.random(N)).astype(np.float32)
    return data, mean, k, groups, w


# --------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_identities(weighted):
    data, mean, k, groups, w = _case64()
    w = w if weighted else None
    T, B, K = data.shape[0], len(groups), len(k)
    n = 3 * B
    # Parseval: g = 1 gives the equal-time covariance (1/T) sum_t q q^+ of the projected series
    q = np.stack([project64(data, mean, k, g, w) for g in groups]).transpose(1, 0, 2, 3).reshape(K, n, T)
    G1, A1 = C64.covariance64(data, mean, k, groups, np.ones(T), w)
    assert G1.shape == A1.shape == (1, K, n, n)
    assert _rel(G1[0], np.einsum("kit,kjt->kij", q, np.conj(q)) / T) <= 1e-12
    # Hermitian, positive semidefinite for g >= 0, |G| <= A
    rng = np.random.default_rng(11)
    g = np.stack([rng.random(T), spectral_weights(T, 0.002, -2)])
    G, A = C64.covariance64(data, mean, k, groups, g, w)
    assert np.array_equal(G, np.conj(G.transpose(0, 1, 3, 2)))
    assert np.all(np.abs(G) <= A * (1 + 1e-12))
    for m in range(2):
        for kk in range(K):
            ev = np.linalg.eigvalsh(G[m, kk])
            assert ev.min() >= -1e-12 * ev.max()
    # sum_w g Phi[w,k,nu] = e_nu^+ G e_nu for random vectors (not normalised, M free)
    e = M64.random_unitary(rng, K, B, 7) * np.complex64(1.5)
    phi = M64.mode_sed64(data, mean, k, groups, e, w)
    v = e.reshape(K, 7, n).astype(np.complex128)
    for m in range(2):
        quad = np.real(np.einsum("kmi,kij,kmj->km", np.conj(v), G[m], v))
        assert _rel(quad, np.einsum("w,wkm->km", g[m], phi)) <= 1e-12
    # the scale, and one row of weights given as (T,)
    S = M64.spectra64(data, mean, k, groups, w)
    assert np.allclose(C64.cov64(S, g[0], scale=0.25)[0], 0.25 * G[:1], rtol=1e-14, atol=0)


def test_metric_bound_and_constants():
    S, g = C64.kernel_case(2, 40, 3, 2)
    G, A = C64.cov64(S, g)
    assert S.dtype == np.complex64 and g.dtype == np.float32 and g.shape == (2, 40) and not g[:, 0].any()
    assert C64.per_component(G, G, A) == 0.0
    off = G.copy()
    off[1, 2, 3, 1] += 5j * C64.U * A[1, 2, 3, 1]
    assert C64.per_component(off, G, A) == pytest.approx(5 * C64.U, rel=1e-6)
    with pytest.raises(AssertionError):
        C64.per_component(np.ones_like(G), G, np.zeros_like(A))
    # the constants the bound is built from are those of the kernel's text, and its header comment states them
    k = C64.kernel_constants()
    assert (k["COV_CHAIN"], k["COV_FOLDS"], k["COV_TILE"], k["COV_CHUNK"]) == (_hip.COV_CHAIN, _hip.COV_FOLDS, _hip.COV_TILE,
                                                                               _hip.COV_CHUNK)
    assert 16 * k["COV_MAX_BLOCKS"] == _hip.COV_MAX_ROWS == 96
    assert _hip.COV_CHAIN <= 256 and _hip.COV_CHUNK == _hip.COV_CHAIN * _hip.COV_FOLDS and _hip.COV_CHAIN % _hip.COV_TILE == 0
    text = C64.KERNEL_SOURCE.read_text()
    assert f"COV_CHAIN = {_hip.COV_CHAIN} frequencies" in text and f"COV_FOLDS = {_hip.COV_FOLDS} times" in text
    assert C64.bound() == (2 * _hip.COV_CHAIN + _hip.COV_FOLDS + 4) * C64.U == 292 * C64.U


@pytest.mark.parametrize("B,T,K", [(2, 300, 3), (5, 200, 3)])
def test_bound_can_fail(B, T, K):
    """On the generator's inputs: the float32 chain in the kernel's structure (without FMA) is inside the bound; the same
    chain with the loud frequency dropped at one k-point, or with ONE row truncated to bfloat16, is far outside it"""
    S, g = C64.kernel_case(B, T, K, 2)
    ref, A = C64.cov64(S, g)
    k = K - 1                                              # the quietest k-point
    i = C64.loudest_row(S, k)
    good = C64.per_component(C64.chain32(S, g), ref, A)
    drop = C64.per_component(C64.chain32(S, g, drop=(k, T // 3)), ref, A)
    trunc = C64.per_component(C64.chain32(S, g, truncate=(k, i)), ref, A)
    print(f"B={B} T={T} K={K}: bound {C64.bound() / C64.U:.0f} u, chain {good / C64.U:.1f} u, dropped frequency "
          f"{drop / C64.bound():.0f} x bound, truncated row {trunc / C64.bound():.0f} x bound")
    assert good <= C64.bound()
    assert drop >= 100 * C64.bound()
    assert trunc >= 10 * C64.bound()


# --------------------------------------------------------------------------------------------------- mode vectors
def _planted(rng, K, B, freqs_thz, kT=0.7):
    """(G_u, G_v, vectors (K, n, n) rows = modes) of k_B T D^-1 and k_B T 1 in a random unitary basis"""
    n = 3 * B
    z = rng.standard_normal((K, n, n)) + 1j * rng.standard_normal((K, n, n))
    V = np.stack([np.linalg.qr(zk)[0] for zk in z])                        # columns: modes
    om2 = (2 * np.pi * np.asarray(freqs_thz, np.float64)) ** 2
    G_u = np.einsum("kin,kn,kjn->kij", V, kT / om2, np.conj(V))
    G_v = np.einsum("kin,kn,kjn->kij", V, np.full_like(om2, kT), np.conj(V))
    return G_u, G_v, V.transpose(0, 2, 1)


def test_mode_vectors_recovery_order_gauge():
    rng = np.random.default_rng(3)
    K, B = 4, 2
    f = np.sort(rng.uniform(1.0, 15.0, (K, 6)), axis=1)[:, ::-1]          # planted in DEscending order
    G_u, G_v, V = _planted(rng, K, B, f)
    mv = mode_vectors(G_u, G_v)
    assert isinstance(mv, ModeVectors) and mv.eigenvectors.shape == (K, 6, B, 3) and mv.eigenvectors.dtype == np.complex64
    assert mv.frequency.shape == mv.eigenvalues.shape == mv.ok.shape == (K, 6) and mv.ok.all()
    assert np.all(np.diff(mv.frequency, axis=1) > 0)                     # ascending
    assert np.allclose(mv.frequency, f[:, ::-1], rtol=1e-10)
    assert np.allclose(mv.eigenvalues, 0.7 / (2 * np.pi * mv.frequency) ** 2, rtol=1e-10)
    e = mv.eigenvectors.reshape(K, 6, 6).astype(np.complex128)
    overlap = np.abs(np.einsum("kni,kni->kn", np.conj(V[:, ::-1]), e))
    assert overlap.min() >= 1 - 1e-6
    top = np.argmax(np.abs(e), axis=2)                                     # gauge: the largest component real, positive
    pivot = np.take_along_axis(e, top[:, :, None], axis=2)[:, :, 0]
    assert np.all(np.abs(pivot.imag) <= 1e-7) and np.all(pivot.real > 0)
    assert mv.displacement_covariance is not None and np.array_equal(mv.velocity_covariance, G_v)
    # the vectors are the convention of the contraction: e^+ G_u e is the eigenvalue
    assert np.allclose(np.real(np.einsum("kni,kij,knj->kn", np.conj(e), G_u, e)), mv.eigenvalues, rtol=1e-5)


def test_mode_vectors_degenerate_pair_and_bad_modes():
    rng = np.random.default_rng(5)
    f = np.array([[2.0, 5.0, 5.0, 7.0, 9.0, 11.0]])
    G_u, G_v, V = _planted(rng, 1, 2, f)
    mv = mode_vectors(G_u, G_v)
    e = mv.eigenvectors.reshape(6, 6).astype(np.complex128)
    assert np.allclose(mv.frequency[0], f[0], rtol=1e-7)
    P = np.einsum("ni,nj->ij", V[0, 1:3].conj(), V[0, 1:3])               # projector on the planted pair's subspace
    for nu in (1, 2):
        assert abs(np.vdot(e[nu], P.T @ e[nu]).real - 1.0) <= 1e-5        # some basis of the right subspace
    assert abs(np.vdot(e[1], e[2])) <= 1e-5
    # a non-positive eigenvalue of G_u, and a non-positive quotient: NaN, ok False, sorted last, the rest untouched
    lam = np.array([0.05, 0.04, 0.03, 0.02, 0.01, -0.01])
    Gu = np.einsum("in,n,jn->ij", V[0].T, lam, np.conj(V[0].T))[None]
    Gv = np.einsum("in,n,jn->ij", V[0].T, np.array([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]), np.conj(V[0].T))[None]
    bad = mode_vectors(Gu, Gv)
    assert bad.ok[0].tolist() == [True] * 4 + [False] * 2 and np.isnan(bad.frequency[0, 4:]).all()
    assert np.allclose(bad.frequency[0, :4], np.sqrt(1.0 / np.array([0.05, 0.04, 0.02, 0.01])) / (2 * np.pi), rtol=1e-9)
    with pytest.raises(ValueError):
        mode_vectors(np.zeros((1, 4, 4)), np.zeros((1, 4, 4)))           # 3B
    with pytest.raises(ValueError):
        mode_vectors(np.zeros((1, 6, 6)), np.zeros((2, 6, 6)))


def test_spectral_weights():
    T, dt = 16, 0.01
    f = np.fft.fftfreq(T, dt)
    for moment in (0, -2, 2):
        g = spectral_weights(T, dt, moment)
        assert g.dtype == np.float32 and g.shape == (T,) and g[0] == 0.0
        want = np.where(f != 0, (2 * np.pi * np.where(f == 0, 1, f)) ** moment, 0.0)
        assert np.array_equal(g, want.astype(np.float32))
    g = spectral_weights(T, dt, 0, band=(10.0, 30.0))
    assert np.array_equal(g != 0, (np.abs(f) >= 10.0) & (np.abs(f) < 30.0)) and g.max() == 1.0
    assert spectral_weights(T, dt, -2, band=(0.0, 50.0))[0] == 0.0       # Nyquist = 50 THz
    assert spectral_weights(5, dt, 2)[0] == 0.0 and np.all(spectral_weights(5, dt, 2)[1:] > 0)
    for bad in ((30.0, 10.0), (10.0, 10.0), (-1.0, 10.0), (10.0, 60.0), (1.0, 2.0)):   # the last holds no bin (df = 6.25)
        with pytest.raises(ValueError):
            spectral_weights(T, dt, 0, band=bad)
    for moment in (1, -1, 4, None):
        with pytest.raises(ValueError):
            spectral_weights(T, dt, moment)


# --------------------------------------------------------------------------------------------------- package surface
def test_binding_declares_the_entry_points():
    assert len(_hip.SIGNATURES["psa_sed_covariance"][1]) == 13 and len(_hip.SIGNATURES["psa_debug_covariance"][1]) == 9
    assert _hip.ABI_VERSION == 6
    assert hasattr(_hip.Engine, "sed_covariance") and hasattr(_hip.Engine, "debug_covariance")
    lib = _hip.load_library()
    assert lib.psa_abi_version() == 6 and lib.psa_sed_covariance and lib.psa_debug_covariance
    header = (HERE.parent / "include" / "psa_hip.h").read_text()
    assert "int psa_sed_covariance(" in header and "int psa_debug_covariance(" in header
    assert "#define PSA_HIP_ABI_VERSION 6" in header
    import psa_amd
    assert all(name in psa_amd.__all__ for name in ("ModeVectors", "mode_vectors", "spectral_weights"))


# --------------------------------------------------------------------------------------------------- the calculator
class CovStandIn:
    """What the two methods need of an engine: residency, weights, `sed_covariance` (the float64 restatement), and a
    log of the calls in order."""

    def __init__(self, fail=False):
        self.lock = threading.RLock()
        self.slots, self.held, self.log = {}, {}, []
        self.weights, self.segment_length, self.fail = None, 0, fail
        self.rank, self.nranks = 0, 1

    def is_resident(self, slot, array):
        return self.held.get(slot) is array

    def ensure_resident(self, slot, array):
        if not self.is_resident(slot, array):
            self.log.append(("upload", slot))
            self.slots[slot], self.held[slot] = np.asarray(array, np.float32), array

    def mean_positions(self, slot):
        return np.mean(self.slots[slot], axis=0, dtype=np.float32)

    def set_atom_weights(self, w):
        self.log.append(("weights", None if w is None else w.copy()))
        self.weights = w

    def sed_covariance(self, slot, mean_pos_all, k_vectors, groups, freq_weights, flags=0):
        self.log.append(("covariance", slot, flags, groups, freq_weights.dtype, freq_weights.shape, freq_weights.copy()))
        if self.fail:
            raise _hip.PsaHipError("injected failure")
        n = self.slots[slot].shape[1]
        g = [np.arange(n)] if groups is None else groups
        return C64.covariance64(self.slots[slot], mean_pos_all, k_vectors, g, freq_weights, self.weights,
                                bool(flags & _hip.F_DISPLACEMENTS))[0]


def _golden(name="a"):
    import conftest
    with np.load(conftest.GOLDEN / f"traj_{name}.npz") as z:
        d = {k: z[k] for k in z.files}
    d["dt_ps"], d["cells"] = float(d["dt_ps"]), tuple(int(v) for v in d["cells"])
    return d


def test_calculator_results_and_engine_calls():
    import conftest
    d = _golden()
    eng = CovStandIn()
    calc = conftest.make_calculator(d).attach(engine=eng)
    tr = calc.traj
    T, N = tr.n_frames, tr.n_atoms
    mags, vecs = calc.get_k_path("100", 1.0, 4)
    groups = site_groups(np.arange(N) % 2)
    mean = np.mean(tr.positions, axis=0, dtype=np.float32)
    rng = np.random.default_rng(2)
    g2 = rng.random((2, T))

    G = calc.calculate_spectral_covariance(mags, vecs, basis_atom_indices=groups, freq_weights=g2)
    assert G.shape == (2, 4, 6, 6) and G.dtype == np.complex128
    assert [e[0] for e in eng.log] == ["upload", "covariance"]
    assert eng.log[-1][1:3] == (_hip.SLOT_VELOCITIES, 0) and eng.log[-1][4:6] == (np.float32, (2, T))
    assert _rel(G, C64.covariance64(tr.velocities, mean, vecs, groups, g2.astype(np.float32))[0]) <= 1e-12

    # one row as (T,), lists of lists, weights set for the call only
    w = mass_weights(tr.types, {int(t): 1.0 + 3.0 * i for i, t in enumerate(np.unique(tr.types))})
    eng.log.clear()
    G1 = calc.calculate_spectral_covariance(mags, vecs, [g.tolist() for g in groups], atom_weights=w, freq_weights=g2[1])
    assert G1.shape == (1, 4, 6, 6) and eng.log[-2][5] == (1, T)
    assert [e[0] for e in eng.log] == ["weights", "covariance", "weights"] and eng.weights is None
    assert _rel(G1, C64.covariance64(tr.velocities, mean, vecs, groups, g2[1].astype(np.float32), w)[0]) <= 1e-12

    # no basis: all atoms as one group, the NULL group of the ABI
    eng.log.clear()
    one = calc.calculate_spectral_covariance(mags, vecs, freq_weights=np.ones(T))
    assert eng.log[-1][3] is None and one.shape == (1, 4, 3, 3)

    # mode vectors: one engine call with two rows, the moments (-2, 0) of a velocity calculator, the band in both
    eng.log.clear()
    band = (0.5 / (T * d["dt_ps"]), 0.4 / d["dt_ps"])
    mv = calc.calculate_mode_vectors(mags, vecs, groups, atom_weights=w, band=band)
    calls = [e for e in eng.log if e[0] == "covariance"]
    assert len(calls) == 1 and calls[0][5] == (2, T)
    assert np.array_equal(calls[0][6], np.stack([spectral_weights(T, d["dt_ps"], -2, band), spectral_weights(T, d["dt_ps"], 0, band)]))
    assert isinstance(mv, ModeVectors) and mv.eigenvectors.shape == (4, 6, 2, 3) and mv.eigenvectors.dtype == np.complex64
    assert mv.frequency.shape == (4, 6) and mv.k_points is mags and mv.k_vectors is vecs
    assert len(mv.groups) == 2 and all(np.array_equal(a, b) for a, b in zip(mv.groups, groups)) and eng.weights is None
    ref = mode_vectors(*C64.covariance64(tr.velocities, mean, vecs, groups, calls[0][6], w)[0])
    assert np.array_equal(mv.frequency, ref.frequency) and np.array_equal(mv.eigenvectors, ref.eigenvectors)
    assert np.array_equal(mv.displacement_covariance, ref.displacement_covariance)

    # a displacement calculator: positions slot, the displacement flag, the moments (0, +2)
    disp = conftest.make_calculator(d, use_displacements=True).attach(engine=CovStandIn())
    types_ = [int(t) for t in np.unique(tr.types)]
    md = disp.calculate_mode_vectors(mags, vecs, basis_atom_types=types_)
    call = [e for e in disp.engine.log if e[0] == "covariance"][0]
    assert call[1:3] == (_hip.SLOT_POSITIONS, _hip.F_DISPLACEMENTS)
    assert np.array_equal(call[6], np.stack([spectral_weights(T, d["dt_ps"], 0), spectral_weights(T, d["dt_ps"], 2)]))
    assert md.eigenvectors.shape == (4, 3 * len(types_), len(types_), 3)


def test_validation():
    import conftest
    d = _golden()
    eng = CovStandIn()
    calc = conftest.make_calculator(d).attach(engine=eng)
    T, N = calc.traj.n_frames, calc.traj.n_atoms
    mags, vecs = calc.get_k_path("100", 1.0, 4)
    two = [[0, 1, 2], [3, 4]]
    ones = np.ones(T)
    with pytest.raises(ValueError, match="freq_weights"):
        calc.calculate_spectral_covariance(mags, vecs, two, freq_weights=np.ones(T + 1))
    with pytest.raises(ValueError, match="freq_weights"):
        calc.calculate_spectral_covariance(mags, vecs, two, freq_weights=np.ones((3, T)))
    with pytest.raises(ValueError, match="freq_weights"):
        calc.calculate_spectral_covariance(mags, vecs, two, freq_weights=np.ones((0, T)))
    bad = ones.copy()
    bad[3] = np.inf
    with pytest.raises(ValueError, match="finite"):
        calc.calculate_spectral_covariance(mags, vecs, two, freq_weights=bad)
    with pytest.raises(ValueError, match="disjoint"):
        calc.calculate_spectral_covariance(mags, vecs, [[0, 1], [1, 2]], freq_weights=ones)
    with pytest.raises(ValueError, match="out of bounds"):
        calc.calculate_spectral_covariance(mags, vecs, [[0, N], [1]], freq_weights=ones)
    with pytest.raises(ValueError, match="32 atom groups"):
        calc.calculate_spectral_covariance(mags, vecs, [[i] for i in range(33)], freq_weights=ones)
    with pytest.raises(ValueError):
        calc.calculate_spectral_covariance(mags, vecs, two, atom_weights=np.ones(N + 1), freq_weights=ones)
    with pytest.raises(TypeError):                                                    # keyword only, and required
        calc.calculate_spectral_covariance(mags, vecs, two, None, None, ones)
    with pytest.raises(TypeError):
        calc.calculate_spectral_covariance(mags, vecs, two)
    with pytest.raises(ValueError):
        calc.calculate_mode_vectors(mags, vecs, two, band=(5.0, 1.0))
    assert eng.log == []                                                              # refused before the engine hears of it

    none = (np.zeros(0, np.float32), np.zeros((0, 3), np.float32))
    empty_k = calc.calculate_spectral_covariance(*none, two, freq_weights=np.ones((2, T)))
    assert empty_k.shape == (2, 0, 6, 6) and empty_k.dtype == np.complex128 and eng.log == []
    mv0 = calc.calculate_mode_vectors(*none, two)                                       # empty inputs as `calculate_mode_sed`
    assert isinstance(mv0, ModeVectors) and mv0.eigenvectors.shape == (0, 6, 2, 3) and mv0.eigenvectors.dtype == np.complex64
    assert mv0.frequency.shape == mv0.ok.shape == (0, 6) and len(mv0.groups) == 2 and eng.log == []

    stub = types.SimpleNamespace(nranks=2, mode="k", engine=CovStandIn(), run=None)
    sharded = conftest.make_calculator(d).attach(shard_group=stub)
    with pytest.raises(NotImplementedError):
        sharded.calculate_spectral_covariance(mags, vecs, two, freq_weights=ones)
    with pytest.raises(NotImplementedError):
        sharded.calculate_mode_vectors(mags, vecs, two)
    assert stub.engine.log == []

    from psa_amd import SEDCalculator, Trajectory
    empty = Trajectory(np.zeros((0, 4, 3), np.float32), np.zeros((0, 4, 3), np.float32), np.ones(4, int),
                       np.zeros(0, np.float32), np.eye(3, dtype=np.float32) * 10, np.full(3, 10, np.float32),
                       np.zeros(3, np.float32), 0.001)
    got = SEDCalculator(empty, 1, 1, 1).attach(engine=eng).calculate_spectral_covariance(mags, vecs, two, freq_weights=np.zeros(0))
    assert got.shape == (1, 0, 0, 0) and eng.log == []
    mv0 = SEDCalculator(empty, 1, 1, 1).attach(engine=eng).calculate_mode_vectors(mags, vecs, two)
    assert mv0.eigenvectors.shape == (0, 0, 0, 3) and mv0.frequency.shape == (0, 0) and mv0.groups == [] and eng.log == []


def test_weights_cleared_after_a_failure():
    import conftest
    d = _golden()
    eng = CovStandIn(fail=True)
    calc = conftest.make_calculator(d).attach(engine=eng)
    mags, vecs = calc.get_k_path("100", 1.0, 2)
    with pytest.raises(_hip.PsaHipError):
        calc.calculate_mode_vectors(mags, vecs, atom_weights=np.ones(calc.traj.n_atoms, np.float32))
    assert eng.weights is None
