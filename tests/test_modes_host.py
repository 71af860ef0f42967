"""The mode-projected SED without a GPU: the float64 restatement (tests/modes64.py) against the identities that tie it
to the plain SED; the proof that the contraction kernel's per-element bound can fail where rel_max cannot; `site_groups`
and the `ModeSED` container; the binding; what `calculate_mode_sed` validates, resolves and hands to the engine (the
engine is a small stand-in defined here that answers `sed_modes` with the restatement)."""
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

import modes64 as M64                                             # noqa: E402
from psa_amd import ModeSED, _hip, mass_weights, site_groups      # noqa: E402
from ref64 import project64                                       # noqa: E402


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# --------------------------------------------------------------------------------------------------- the restatement
def _case64(seed=4, N=64, T=32, K=5, B=4):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((T, N, 3)).astype(np.float32)
    mean = (rng.random((N, 3)) * 11.0).astype(np.float32)
    k = (rng.standard_normal((K, 3)) * 0.8).astype(np.float32)
    groups = site_groups(np.arange(N) % B)
    w = (0.5 + rng.random(N)).astype(np.float32)
    return data, mean, k, groups, w


def _spectrum(data, mean, k, g, w):
    """(T, K, 3) complex128 of one group, straight from tests/ref64.py"""
    return (np.fft.fft(project64(data, mean, k, g, w), axis=-1) / data.shape[0]).transpose(2, 0, 1)


@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_identities(weighted):
    data, mean, k, groups, w = _case64()
    w = w if weighted else None
    B, K = len(groups), len(k)
    per_group = [_spectrum(data, mean, k, g, w) for g in groups]
    # Cartesian vectors: column 3b + c is |S_b[.., c]|^2
    cart = np.zeros((K, 3 * B, B, 3), np.complex64)
    for b in range(B):
        for c in range(3):
            cart[:, 3 * b + c, b, c] = 1.0
    phi = M64.mode_sed64(data, mean, k, groups, cart, w)
    for b in range(B):
        assert _rel(phi[:, :, 3 * b:3 * b + 3], np.abs(per_group[b]) ** 2) <= 1e-12
    # union vectors: the coherent spectrum of all atoms
    union = np.zeros((K, 3, B, 3), np.complex64)
    for c in range(3):
        union[:, c, :, c] = 1.0
    whole = _spectrum(data, mean, k, np.arange(data.shape[1]), w)
    assert _rel(M64.mode_sed64(data, mean, k, groups, union, w), np.abs(whole) ** 2) <= 1e-12
    # completeness: unitary vectors sum to the incoherent intensity (complex64 vectors are unitary to 1e-7 only:
    # the float64 matrix is used here)
    rng = np.random.default_rng(9)
    z = rng.standard_normal((K, 3 * B, 3 * B)) + 1j * rng.standard_normal((K, 3 * B, 3 * B))
    uni = np.stack([np.linalg.qr(zk)[0] for zk in z]).reshape(K, 3 * B, B, 3)
    inco = sum(np.sum(np.abs(s) ** 2, axis=-1) for s in per_group)
    S = M64.spectra64(data, mean, k, groups, w)
    Q = np.einsum("kmbc,bkcw->wkm", np.conj(uni), S)
    assert _rel(np.sum(np.abs(Q) ** 2, axis=-1), inco) <= 1e-12
    assert _rel(np.sum(M64.mode_sed64(data, mean, k, groups, uni.astype(np.complex64), w), axis=-1), inco) <= 1e-6
    # homogeneity, and an empty group contributes nothing
    e5 = M64.random_unitary(rng, K, B, 5)
    base = M64.mode_sed64(data, mean, k, groups, e5, w)
    assert _rel(M64.mode_sed64(data, mean, k, groups, np.complex64(2) * e5, w), 4 * base) <= 1e-12
    g5 = groups + [np.zeros(0, int)]
    e6 = np.concatenate([e5, np.ones((K, 5, 1, 3), np.complex64)], axis=2)
    assert np.array_equal(M64.mode_sed64(data, mean, k, g5, e6, w), base)


def test_scale_and_metric():
    S, e = M64.kernel_case(2, 6, 40, 3)
    phi, A = M64.contract64(S, e)
    assert phi.shape == A.shape == (40, 3, 6) and np.all(phi <= A ** 2 * (1 + 1e-12))
    assert M64.per_element(phi, phi, A) == 0.0
    off = phi.copy()
    off[3, 1, 2] += 5 * M64.U * A[3, 1, 2] ** 2
    assert M64.per_element(off, phi, A) == pytest.approx(5 * M64.U, rel=1e-6)
    with pytest.raises(AssertionError):
        M64.per_element(np.ones_like(phi), phi, np.zeros_like(A))
    assert M64.bound(8) == 106 * M64.U and M64.bound(1) == 22 * M64.U and M64.bound(40) == 490 * M64.U
    assert (8, 24) in [c[:2] for c in M64.CASES] and (40, 7) in [c[:2] for c in M64.CASES]
    assert any(c[2] % 64 for c in M64.CASES) and all(c[3] >= 3 for c in M64.CASES)


@pytest.mark.parametrize("case", M64.CASES, ids=[f"B{c[0]}_M{c[1]}" for c in M64.CASES])
def test_bound_can_fail_where_rel_max_cannot(case):
    """On the inputs of the GPU test: a float32 chain without FMA is under the bound; the same chain with ONE term's
    spectrum truncated to bfloat16 is at least 10 x over it (1000 x at B = 8, M = 24) while its rel_max stays under
    the project's 1e-5 bar; with one term dropped it is at least 1000 x over."""
    B, Mv, T, K = case
    S, e = M64.kernel_case(B, Mv, T, K)
    ref, A = M64.contract64(S, e)
    k = K - 1                                              # the quietest k-point: rel_max looks at the loudest
    b, c = M64.loudest_term(S, k)
    good, trunc, drop = M64.chain32(S, e), M64.chain32(S, e, truncate=(k, b, c)), M64.chain32(S, e, drop=(k, b, c))
    g, t, d = (M64.per_element(x, ref, A) for x in (good, trunc, drop))
    print(f"B={B} M={Mv} T={T} K={K}: bound {M64.bound(B) / M64.U:.0f} u, chain {g / M64.U:.1f} u, truncated term "
          f"{t / M64.bound(B):.0f} x bound at rel_max {_rel(trunc, ref):.2e}, dropped term {d / M64.bound(B):.0f} x bound")
    assert g <= M64.bound(B)
    assert t >= 10 * M64.bound(B) and _rel(trunc, ref) < 1e-5
    assert d >= 1000 * M64.bound(B)
    if (B, Mv) == (8, 24):
        assert t >= 1000 * M64.bound(B)


# --------------------------------------------------------------------------------------------------- package surface
def test_site_groups_and_container():
    g = site_groups(np.arange(16) % 8)
    assert len(g) == 8 and all(np.array_equal(g[b], [b, b + 8]) for b in range(8))
    g = site_groups(["b", "a", "b", "c"])
    assert [x.tolist() for x in g] == [[1], [0, 2], [3]]
    with pytest.raises(ValueError):
        site_groups(np.zeros((2, 2)))
    sed = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    m = ModeSED(sed, np.fft.fftfreq(2, 0.5), np.zeros(3), np.zeros((3, 3)), g)
    assert m.sed is sed and np.array_equal(m.total, sed.sum(axis=-1)) and len(m.groups) == 3
    import psa_amd
    assert "ModeSED" in psa_amd.__all__ and "site_groups" in psa_amd.__all__


def test_binding_declares_the_entry_points():
    assert "psa_sed_modes" in _hip.SIGNATURES and "psa_debug_mode_power" in _hip.SIGNATURES
    assert _hip.OPT_MODES_WORK_BYTES == 12 and _hip.ABI_VERSION == 6
    assert hasattr(_hip.Engine, "sed_modes") and hasattr(_hip.Engine, "debug_mode_power")
    lib = _hip.load_library()
    assert lib.psa_abi_version() == 6 and lib.psa_sed_modes and lib.psa_debug_mode_power
    header = (HERE.parent / "include" / "psa_hip.h").read_text()
    assert "#define PSA_OPT_MODES_WORK_BYTES 12" in header and "#define PSA_HIP_ABI_VERSION 6" in header


# --------------------------------------------------------------------------------------------------- the calculator
class ModesStandIn:
    """What `calculate_mode_sed` needs of an engine: residency, weights, `sed_modes` (the float64 restatement as
    float32), and a log of the calls in order."""

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

    def sed_modes(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, flags=0):
        self.log.append(("modes", slot, flags, groups, eigenvectors.dtype, eigenvectors.shape))
        if self.fail:
            raise _hip.PsaHipError("injected failure")
        n = self.slots[slot].shape[1]
        g = [np.arange(n)] if groups is None else groups
        return M64.mode_sed64(self.slots[slot], mean_pos_all, k_vectors, g, eigenvectors, self.weights,
                              bool(flags & _hip.F_DISPLACEMENTS)).astype(np.float32)


def _golden(name="a"):
    import conftest
    with np.load(conftest.GOLDEN / f"traj_{name}.npz") as z:
        d = {k: z[k] for k in z.files}
    d["dt_ps"], d["cells"] = float(d["dt_ps"]), tuple(int(v) for v in d["cells"])
    return d


def test_calculator_results_and_engine_calls():
    import conftest
    d = _golden()
    eng = ModesStandIn()
    calc = conftest.make_calculator(d).attach(engine=eng)
    tr = calc.traj
    T, N = tr.n_frames, tr.n_atoms
    mags, vecs = calc.get_k_path("100", 1.0, 4)
    labels = np.arange(N) % 2
    groups = site_groups(labels)
    rng = np.random.default_rng(2)
    eig = M64.random_unitary(rng, 4, 2, 5)
    mean = np.mean(tr.positions, axis=0, dtype=np.float32)

    got = calc.calculate_mode_sed(mags, vecs, eig, basis_atom_indices=groups)
    assert isinstance(got, ModeSED) and got.sed.shape == (T, 4, 5) and got.sed.dtype == np.float32
    assert np.array_equal(got.freqs, np.fft.fftfreq(T, d=d["dt_ps"]))
    assert got.k_points is mags and got.k_vectors is vecs
    assert len(got.groups) == 2 and all(np.array_equal(a, b) for a, b in zip(got.groups, groups))
    assert [e[0] for e in eng.log] == ["upload", "modes"]                    # no weights: never heard of
    assert eng.log[-1][1:3] == (_hip.SLOT_VELOCITIES, 0) and eng.log[-1][4:] == (np.complex64, (4, 5, 2, 3))
    ref = M64.mode_sed64(tr.velocities, mean, vecs, groups, eig)
    assert _rel(got.sed, ref) <= 1e-6

    # lists of lists, complex128 vectors, weights set for the call only
    w = mass_weights(tr.types, {int(t): 1.0 + 3.0 * i for i, t in enumerate(np.unique(tr.types))})
    eng.log.clear()
    got = calc.calculate_mode_sed(mags, vecs, eig.astype(np.complex128), [g.tolist() for g in groups], atom_weights=w)
    assert [e[0] for e in eng.log] == ["weights", "modes", "weights"] and eng.weights is None
    assert _rel(got.sed, M64.mode_sed64(tr.velocities, mean, vecs, groups, eig, w)) <= 1e-6

    # no basis: all atoms as one group, the NULL group of the ABI
    e1 = M64.random_unitary(rng, 4, 1)
    eng.log.clear()
    one = calc.calculate_mode_sed(mags, vecs, e1)
    assert eng.log[-1][3] is None and one.sed.shape == (T, 4, 3)

    # types as groups; displacement mode
    types_ = [int(t) for t in np.unique(tr.types)]
    et = M64.random_unitary(rng, 4, len(types_), 2)
    disp = conftest.make_calculator(d, use_displacements=True).attach(engine=ModesStandIn())
    dd = disp.calculate_mode_sed(mags, vecs, et, basis_atom_types=types_)
    assert disp.engine.log[-1][1:3] == (_hip.SLOT_POSITIONS, _hip.F_DISPLACEMENTS)
    members = [np.flatnonzero(tr.types == t) for t in types_]
    assert _rel(dd.sed, M64.mode_sed64(tr.positions, mean, vecs, members, et, displacements=True)) <= 1e-6


def test_validation():
    import conftest
    d = _golden()
    eng = ModesStandIn()
    calc = conftest.make_calculator(d).attach(engine=eng)
    T, N = calc.traj.n_frames, calc.traj.n_atoms
    mags, vecs = calc.get_k_path("100", 1.0, 4)
    two = [[0, 1, 2], [3, 4]]
    eig = np.ones((4, 5, 2, 3), np.complex64)
    with pytest.raises(ValueError, match=r"\(4, 5, 3, 3\).*\(4, M, 2, 3\)"):         # both shapes are named
        calc.calculate_mode_sed(mags, vecs, np.ones((4, 5, 3, 3), np.complex64), two)
    with pytest.raises(ValueError, match="expected"):
        calc.calculate_mode_sed(mags, vecs, eig[:3], two)                            # K mismatch
    with pytest.raises(ValueError, match="expected"):
        calc.calculate_mode_sed(mags, vecs, eig[:, :, :, :2], two)
    with pytest.raises(ValueError, match="expected"):
        calc.calculate_mode_sed(mags, vecs, eig[:, :0], two)                         # M = 0
    with pytest.raises(ValueError, match="expected"):
        calc.calculate_mode_sed(mags, vecs, eig)                                     # one group of all atoms, B = 2 given
    with pytest.raises(ValueError, match="disjoint"):
        calc.calculate_mode_sed(mags, vecs, eig, [[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="out of bounds"):
        calc.calculate_mode_sed(mags, vecs, eig, [[0, N], [1]])
    bad = eig.copy()
    bad[1, 2, 0, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        calc.calculate_mode_sed(mags, vecs, bad, two)
    with pytest.raises(ValueError):
        calc.calculate_mode_sed(mags, vecs, eig, two, atom_weights=np.ones(N + 1))
    with pytest.raises(TypeError):                                                    # keyword only
        calc.calculate_mode_sed(mags, vecs, eig, two, None, np.ones(N))
    assert eng.log == []                                                              # refused before the engine hears of it

    empty_k = calc.calculate_mode_sed(np.zeros(0, np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 5, 2, 3), np.complex64), two)
    assert isinstance(empty_k, ModeSED) and empty_k.sed.shape == (T, 0, 5) and empty_k.sed.dtype == np.float32
    assert empty_k.freqs.shape == (T,) and len(empty_k.groups) == 2 and eng.log == []

    stub = types.SimpleNamespace(nranks=2, mode="k", engine=ModesStandIn(), run=None)
    sharded = conftest.make_calculator(d).attach(shard_group=stub)
    with pytest.raises(NotImplementedError):
        sharded.calculate_mode_sed(mags, vecs, eig, two)
    assert stub.engine.log == []

    from psa_amd import SEDCalculator, Trajectory
    empty = Trajectory(np.zeros((0, 4, 3), np.float32), np.zeros((0, 4, 3), np.float32), np.ones(4, int),
                       np.zeros(0, np.float32), np.eye(3, dtype=np.float32) * 10, np.full(3, 10, np.float32),
                       np.zeros(3, np.float32), 0.001)
    got = SEDCalculator(empty, 1, 1, 1).attach(engine=eng).calculate_mode_sed(mags, vecs, eig, two)
    assert isinstance(got, ModeSED) and got.sed.shape == (0, 0, 0) and got.freqs.size == 0 and got.groups == []
    assert eng.log == []


def test_weights_cleared_after_a_failure():
    import conftest
    d = _golden()
    eng = ModesStandIn(fail=True)
    calc = conftest.make_calculator(d).attach(engine=eng)
    mags, vecs = calc.get_k_path("100", 1.0, 2)
    with pytest.raises(_hip.PsaHipError):
        calc.calculate_mode_sed(mags, vecs, np.ones((2, 1, 1, 3), np.complex64), atom_weights=np.ones(calc.traj.n_atoms, np.float32))
    assert eng.weights is None
