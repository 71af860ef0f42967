"""The vibrational density of states without a GPU: the float64 restatement (tests/vdos64.py) against
scipy.signal.welch and Parseval; the `VDOS` container; what `calculate_vdos` validates, resolves and hands to the
engine (weights and segments set for the call only, the array made resident first).  The engine is a small stand-in
defined here that answers `vdos` with the restatement."""
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

from psa_amd import VDOS, Segments, _hip, mass_weights          # noqa: E402
from vdos64 import parseval_sum, scipy_factor, vdos64            # noqa: E402


class VdosStandIn:
    """What `calculate_vdos` needs of an engine: residency, weights, segments, `vdos` (the float64 restatement as
    float32), and a log of the calls in order."""

    def __init__(self, fail=False):
        self.lock = threading.RLock()
        self.slots, self.held, self.log = {}, {}, []
        self.weights = self.segments = None
        self.segment_length, self.fail = 0, fail
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

    def set_segments(self, s):
        self.log.append(("segments", s))
        self.segments, self.segment_length = s, (0 if s is None else s.length)

    def vdos(self, slot, mean_pos_all, groups=None, flags=0):
        self.log.append(("vdos", slot, flags, groups))
        if self.fail:
            raise _hip.PsaHipError("injected failure")
        s, data = self.segments, self.slots[slot]
        kw = {} if s is None else dict(window=s.window_array(), L=s.length, H=s.hop)
        mean = mean_pos_all if flags & _hip.F_DISPLACEMENTS else None
        return vdos64(data, [None] if groups is None else groups, weights=self.weights, mean=mean, **kw).astype(np.float32)


def _golden(name="a"):
    import conftest
    with np.load(conftest.GOLDEN / f"traj_{name}.npz") as z:
        d = {k: z[k] for k in z.files}
    d["dt_ps"], d["cells"] = float(d["dt_ps"]), tuple(int(v) for v in d["cells"])
    return d


def _series(T, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, N, 3))
    x[:, 0, 0] += 3.0 * np.cos(2 * np.pi * 0.1 * np.arange(T))          # a line, and a mean
    x[:, 1, :] += 2.0
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", ["hann", "boxcar", "ramp"])
@pytest.mark.parametrize("T,L,H", [(256, 64, 32), (256, 100, 30), (256, 63, 21), (256, 256, 256), (300, 37, 5)])
def test_restatement_is_scipys_welch(window, T, L, H):
    """per atom and component: scipy.signal.welch(scaling="spectrum", two-sided, no detrending), rows 0 .. L//2, times
    (sum w)^2 / (L sum w^2) is the restatement (scipy needs H <= L); groups sum the atoms, weights enter squared"""
    scipy_signal = pytest.importorskip("scipy.signal")
    x = _series(T, 6, T + L + H)
    w = np.linspace(0.1, 1.0, L) if window == "ramp" else Segments(L, H, window).window_array()
    wf = np.asarray(w, np.float32).astype(np.float64)
    _, pxx = scipy_signal.welch(x.astype(np.float64), fs=1.0, window=wf, nperseg=L, noverlap=L - H, detrend=False,
                                return_onesided=False, scaling="spectrum", axis=0)
    theirs = scipy_factor(w, L) * pxx[:L // 2 + 1]                                     # (F, N, 3)
    per_atom = vdos64(x, [[a] for a in range(6)], w, L, H)
    assert per_atom.shape == theirs.shape == (L // 2 + 1, 6, 3)
    assert np.max(np.abs(per_atom - theirs)) <= 1e-12 * np.max(np.abs(theirs))
    aw = np.float32([1.0, 2.0, 0.5, 3.0, 1.5, 0.0])
    grouped = vdos64(x, [[4, 0], [1, 2, 3], []], w, L, H, weights=aw)
    ref = np.stack([np.sum(theirs[:, g, :] * aw.astype(np.float64)[g][None, :, None] ** 2, axis=1)
                    for g in ([4, 0], [1, 2, 3])], axis=1)
    assert np.max(np.abs(grouped[:, :2] - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert not grouped[:, 2].any()                                                    # an empty group gives zeros


@pytest.mark.parametrize("L", [64, 63])
def test_parseval(L):
    """boxcar, H = L: D[0] + 2 sum_{0<o<L/2} D[o] (+ D[L/2] once for even L) is the mean square of the frames used"""
    T = 200
    x = _series(T, 5, L)
    D = vdos64(x, [None, [1, 3]], np.ones(L), L, L)
    used = x[:(T // L) * L].astype(np.float64)
    for gi, g in enumerate((np.arange(5), np.array([1, 3]))):
        ms = np.sum(np.mean(used[:, g, :] ** 2, axis=0), axis=0)                     # (3,)
        got = parseval_sum(D[:, gi, :], L)
        print(f"L={L} group {gi}: {np.max(np.abs(got - ms) / ms):.2e}")
        assert np.max(np.abs(got - ms) / ms) <= 1e-12


def test_restatement_displacements_and_default_segment():
    x = _series(50, 4, 9)
    mean = np.mean(x, axis=0, dtype=np.float32)
    D = vdos64(x, [None], mean=mean)
    ref = vdos64((x.astype(np.float64) - mean[None].astype(np.float64)), [None])
    assert D.shape == (26, 1, 3) and np.max(np.abs(D - ref)) <= 1e-12 * np.max(ref)
    X = np.fft.rfft(x.astype(np.float64), axis=0) / 50
    np.testing.assert_allclose(vdos64(x, [None])[:, 0, :], np.sum(np.abs(X) ** 2, axis=1), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
def test_vdos_container():
    dos = np.arange(24, dtype=np.float32).reshape(4, 2, 3)
    v = VDOS(dos, np.fft.rfftfreq(6, 0.5), [np.array([0]), np.array([1, 2])])
    assert v.total.shape == (4, 2) and np.array_equal(v.total, dos.sum(axis=-1))
    assert v.dos is dos and len(v.groups) == 2 and v.freqs.shape == (4,)
    import psa_amd
    assert "VDOS" in psa_amd.__all__


def test_binding_declares_psa_vdos():
    assert "psa_vdos" in _hip.SIGNATURES and _hip.ABI_VERSION == 6 and _hip.OPT_VDOS_WORK_BYTES == 11
    assert hasattr(_hip.Engine, "vdos")


def test_calculator_results_and_engine_calls():
    import conftest
    d = _golden()
    eng = VdosStandIn()
    calc = conftest.make_calculator(d).attach(engine=eng)
    tr = calc.traj
    T, N = tr.n_frames, tr.n_atoms
    types_ = [int(t) for t in np.unique(tr.types)]
    members = [np.flatnonzero(tr.types == t) for t in types_]

    got = calc.calculate_vdos()
    assert isinstance(got, VDOS) and got.dos.shape == (T // 2 + 1, 1, 3) and got.dos.dtype == np.float32
    assert np.array_equal(got.freqs, np.fft.rfftfreq(T, d=d["dt_ps"]))
    assert len(got.groups) == 1 and np.array_equal(got.groups[0], np.arange(N))
    assert [e[0] for e in eng.log] == ["upload", "vdos"]                   # no weights, no segments: never heard of
    assert eng.log[-1][1:] == (_hip.SLOT_VELOCITIES, 0, None)               # all atoms in order: the NULL group
    ref = vdos64(tr.velocities, [None])
    assert np.max(np.abs(got.dos - ref)) <= 1e-6 * np.max(ref)

    seg = Segments(16, 8)
    w = mass_weights(tr.types, {t: 1.0 + 3.0 * i for i, t in enumerate(types_)})
    eng.log.clear()
    part = calc.calculate_vdos(basis_atom_types=types_, atom_weights=w, segments=seg)
    assert part.dos.shape == (9, len(types_), 3) and np.array_equal(part.freqs, np.fft.rfftfreq(16, d=d["dt_ps"]))
    assert all(np.array_equal(a, b) for a, b in zip(part.groups, members))
    assert [e[0] for e in eng.log] == ["weights", "segments", "vdos", "weights", "segments"]     # resident already
    assert eng.weights is None and eng.segments is None and eng.segment_length == 0
    ref = vdos64(tr.velocities, members, seg.window_array(), 16, 8, weights=w)
    assert np.max(np.abs(part.dos - ref)) <= 1e-6 * np.max(ref)
    assert np.allclose(part.total, ref.sum(axis=-1), rtol=1e-5)

    lists = calc.calculate_vdos(basis_atom_indices=[[5, 1], [2]])
    assert lists.dos.shape == (T // 2 + 1, 2, 3)
    assert np.max(np.abs(lists.dos - vdos64(tr.velocities, [[5, 1], [2]]))) <= 1e-6 * np.max(lists.dos)

    disp = conftest.make_calculator(d, use_displacements=True).attach(engine=VdosStandIn())
    dd = disp.calculate_vdos()
    assert disp.engine.log[-1][1:3] == (_hip.SLOT_POSITIONS, _hip.F_DISPLACEMENTS)
    mean = np.mean(tr.positions, axis=0, dtype=np.float32)
    ref = vdos64(tr.positions, [None], mean=mean)
    assert np.max(np.abs(dd.dos - ref)) <= 1e-6 * np.max(ref)


def test_validation():
    import conftest
    d = _golden()
    eng = VdosStandIn()
    calc = conftest.make_calculator(d).attach(engine=eng)
    T, N = calc.traj.n_frames, calc.traj.n_atoms
    with pytest.raises(ValueError, match="disjoint"):
        calc.calculate_vdos(basis_atom_indices=[[0, 1], [1, 2]])                     # overlapping groups
    with pytest.raises(ValueError, match="disjoint"):
        calc.calculate_vdos(basis_atom_indices=[0, 3, 0])
    with pytest.raises(ValueError, match="out of bounds"):
        calc.calculate_vdos(basis_atom_indices=[0, N])
    with pytest.raises(TypeError):
        calc.calculate_vdos(segments=16)                                              # bad segments type
    with pytest.raises(ValueError):
        calc.calculate_vdos(segments=Segments(T + 1))                                 # L > T
    with pytest.raises(ValueError):
        calc.calculate_vdos(atom_weights=np.ones(N + 1))                              # weights shape
    with pytest.raises(ValueError):
        calc.calculate_vdos(atom_weights=np.full(N, np.nan))
    with pytest.raises(TypeError):                                                    # keyword only
        calc.calculate_vdos(None, None, np.ones(N))
    assert eng.log == []                                                              # refused before the engine hears of it

    stub = types.SimpleNamespace(nranks=2, mode="k", engine=VdosStandIn(), run=None)
    sharded = conftest.make_calculator(d).attach(shard_group=stub)
    with pytest.raises(NotImplementedError):
        sharded.calculate_vdos()
    assert stub.engine.log == []

    from psa_amd import SEDCalculator, Trajectory
    empty = Trajectory(np.zeros((0, 4, 3), np.float32), np.zeros((0, 4, 3), np.float32), np.ones(4, int),
                       np.zeros(0, np.float32), np.eye(3, dtype=np.float32) * 10, np.full(3, 10, np.float32),
                       np.zeros(3, np.float32), 0.001)
    got = SEDCalculator(empty, 1, 1, 1).attach(engine=eng).calculate_vdos()
    assert isinstance(got, VDOS) and got.dos.shape == (0, 0, 3) and got.freqs.size == 0 and got.groups == []
    assert eng.log == []


def test_cleared_after_a_failure():
    import conftest
    d = _golden()
    eng = VdosStandIn(fail=True)
    calc = conftest.make_calculator(d).attach(engine=eng)
    w = np.ones(calc.traj.n_atoms, np.float32)
    with pytest.raises(_hip.PsaHipError):
        calc.calculate_vdos(atom_weights=w, segments=Segments(8))
    assert eng.weights is None and eng.segments is None and eng.segment_length == 0
