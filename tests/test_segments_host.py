"""Segment-averaged (Welch) spectra without a GPU: `Segments` validation, `count`, the hann window against scipy, the
float64 restatement (tests/welch64.py) against scipy.signal.welch, the calculator's refusals (chiral, sharded), and the
rule that the engine hears of segments only for the call that asks (cleared afterwards, whatever happens).  The engine
is the CPU test double with segments."""
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import scipy.signal

HERE = Path(__file__).resolve().parent
for p in (str(HERE.parent), str(HERE), str(HERE / "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle_engine import OracleEngine          # noqa: E402
from psa_amd import Segments, _hip               # noqa: E402
from welch64 import project64, scipy_factor, segment_intensity64, welch_intensity64   # noqa: E402


class SegmentOracleEngine(OracleEngine):
    """The oracle double with psa_set_segments: a velocity-mode intensity call while segments are set returns the
    float64 restatement as float32 (L, K)."""

    def __init__(self, *args, fail=False, **kw):
        super().__init__(*args, **kw)
        self.segments, self.segment_calls, self.fail, self._pending = None, [], fail, None

    def set_segments(self, s):
        self.segment_calls.append(s)
        self.segments = s

    def _welch(self, slot, mean_pos_all, k_vectors, groups, flags):
        assert flags & _hip.F_INTENSITY and not flags & _hip.F_DISPLACEMENTS
        if self.fail:
            raise _hip.PsaHipError("injected failure")
        s = self.segments
        gs = [None] if groups is None else list(groups)
        return welch_intensity64(self.slots[slot], mean_pos_all, k_vectors, gs, s.window_array(), s.length,
                                 s.hop).astype(np.float32)

    def calculate(self, slot, mean_pos_all, k_vectors, groups=None, flags=0, with_intensity=False):
        if self.segments is None:
            return super().calculate(slot, mean_pos_all, k_vectors, groups, flags, with_intensity)
        return self._welch(slot, mean_pos_all, k_vectors, groups, flags)

    def project_upload(self, slot, array, mean_pos_all, k_vectors, groups=None, flags=0):
        if self.segments is None:
            return super().project_upload(slot, array, mean_pos_all, k_vectors, groups, flags)
        self.ensure_resident(slot, array)
        self._pending = self._welch(slot, mean_pos_all, k_vectors, groups, flags)

    def finalize(self, T, K, intensity, fetch=True, with_intensity=False):
        if self._pending is None:
            return super().finalize(T, K, intensity, fetch, with_intensity)
        out, self._pending = self._pending, None
        assert out.shape == (T, K) and intensity and not with_intensity
        return out


def _golden(name="a"):
    import conftest
    with np.load(conftest.GOLDEN / f"traj_{name}.npz") as z:
        d = {k: z[k] for k in z.files}
    d["dt_ps"], d["cells"] = float(d["dt_ps"]), tuple(int(v) for v in d["cells"])
    return d


# ---------------------------------------------------------------------------------------------------------------------
def test_segments_validation():
    s = Segments(64)
    assert (s.length, s.hop, s.window) == (64, 32, "hann")
    assert Segments(5).hop == 2 and Segments(2).hop == 1
    with pytest.raises(ValueError):
        Segments(64).count(63)                                   # L > T
    for bad in (dict(length=1), dict(length=0), dict(length=-4), dict(length=2.5), dict(length=64, hop=0),
                dict(length=64, hop=-3), dict(length=64, window="hamming"), dict(length=64, window="HANN"),
                dict(length=64, window=np.ones(63)), dict(length=64, window=np.ones((64, 1))),
                dict(length=4, window=[1.0, np.nan, 1.0, 1.0]), dict(length=4, window=[1.0, np.inf, 1.0, 1.0]),
                dict(length=4, window=np.zeros(4)), dict(length=4, window=[1e300, 1, 1, 1]),
                dict(length=4, window=np.ones(4, np.complex64))):
        with pytest.raises(ValueError):
            Segments(**bad)
    w = np.linspace(0.0, 1.0, 16)
    a, b = Segments(16, 4, w), Segments(16, 4, list(w))
    assert a == b and hash(a) == hash(b)                         # frozen, array windows kept as tuples
    np.testing.assert_array_equal(a.window_array(), w.astype(np.float32))
    with pytest.raises(Exception):
        a.length = 8


@pytest.mark.parametrize("T,L,H,n", [(256, 64, 32, 7), (256, 100, 30, 6), (256, 64, 64, 4), (256, 48, 80, 3),
                                     (256, 256, 256, 1), (256, 256, 1, 1), (257, 64, 64, 4), (65536, 4096, 2048, 31),
                                     (10, 2, 1, 9), (10, 3, 100, 1)])
def test_count(T, L, H, n):
    assert Segments(L, H).count(T) == n
    used = (n - 1) * H + L
    assert used <= T and used + H > T                            # the last segment is the last that fits


@pytest.mark.parametrize("L", [2, 3, 48, 64, 100, 256, 4096])
def test_hann_is_scipys(L):
    w = Segments(L).window_array()
    assert w.dtype == np.float32 and w.shape == (L,)
    assert np.array_equal(w, scipy.signal.get_window("hann", L).astype(np.float32))
    assert np.array_equal(Segments(L, window="boxcar").window_array(), np.ones(L, np.float32))


@pytest.mark.parametrize("window", ["hann", "boxcar", "ramp"])
@pytest.mark.parametrize("T,L,H", [(256, 64, 32), (256, 100, 30), (256, 64, 64), (256, 256, 256), (300, 37, 5)])
def test_restatement_is_scipys_welch(window, T, L, H):
    """sum over components of scipy.signal.welch(scaling="spectrum", two-sided, no detrending) times the documented
    factor (sum w)^2 / (L sum w^2) is the float64 restatement (scipy needs H <= L)"""
    rng = np.random.default_rng(T + L + H)
    q = rng.standard_normal((T, 5, 3)) + 1j * rng.standard_normal((T, 5, 3))
    q[:, 0] += 3.0 * np.exp(2j * np.pi * 0.1 * np.arange(T))[:, None]          # a line, and a mean
    q[:, 1] += 2.0
    w = np.linspace(0.1, 1.0, L) if window == "ramp" else Segments(L, H, window).window_array()
    ours = segment_intensity64(q, w, L, H)
    wf = np.asarray(w, np.float32).astype(np.float64)
    _, pxx = scipy.signal.welch(q, fs=1.0, window=wf, nperseg=L, noverlap=L - H, detrend=False,
                                return_onesided=False, scaling="spectrum", axis=0)
    theirs = scipy_factor(w, L) * np.sum(pxx, axis=-1)
    assert theirs.shape == ours.shape == (L, 5)
    assert np.max(np.abs(ours - theirs)) <= 1e-12 * np.max(np.abs(theirs))


def test_restatement_identities():
    """boxcar, one segment of every frame: the full intensity; boxcar, H = L dividing T: Parseval"""
    rng = np.random.default_rng(1)
    q = rng.standard_normal((240, 4, 3)) + 1j * rng.standard_normal((240, 4, 3))
    full = np.sum(np.abs(np.fft.fft(q, axis=0) / 240) ** 2, axis=-1)
    np.testing.assert_allclose(segment_intensity64(q, np.ones(240), 240, 240), full, rtol=1e-13)
    seg = segment_intensity64(q, np.ones(60), 60, 60)
    np.testing.assert_allclose(np.sum(seg, axis=0), np.sum(full, axis=0), rtol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------
def test_calculator_results_and_engine_calls():
    """through the calculator: (L, K) float32, fftfreq(L), not complex; coherent = the union as one group,
    incoherent = summed over the groups; set on the engine for the call only"""
    import conftest
    d = _golden()
    eng = SegmentOracleEngine()
    calc = conftest.make_calculator(d).attach(engine=eng)
    tr = calc.traj
    mags, vecs = calc.get_k_path("x", 1.0, 6)
    plain = calc.calculate(mags, vecs)
    assert eng.segment_calls == []                               # not asked: never heard of
    seg = Segments(16, 8)
    mean = np.mean(tr.positions, axis=0, dtype=np.float32)
    w = seg.window_array()
    types_ = [int(t) for t in np.unique(tr.types)]
    groups = [np.flatnonzero(tr.types == t) for t in types_]
    for kw, ref_groups in (({}, [None]), (dict(basis_atom_types=types_, summation_mode="incoherent"), groups),
                           (dict(basis_atom_indices=[list(g[:3]) for g in groups]),
                            [np.unique(np.concatenate([g[:3] for g in groups]))])):
        got = calc.calculate(mags, vecs, segments=seg, **kw)
        ref = welch_intensity64(tr.velocities, mean, vecs, ref_groups, w, 16, 8)
        assert got.sed.dtype == np.float32 and got.sed.shape == (16, 6) and not got.is_complex
        np.testing.assert_array_equal(got.freqs, np.fft.fftfreq(16, d=d["dt_ps"]))
        assert np.max(np.abs(got.sed - ref)) <= 1e-6 * np.max(ref)
        assert eng.segments is None and eng.segment_calls[-2:] == [seg, None]
    empty = calc.calculate(np.zeros(0, np.float32), np.zeros((0, 3), np.float32), segments=seg)
    assert empty.sed.shape == (16, 0) and empty.sed.dtype == np.float32
    again = calc.calculate(mags, vecs)
    np.testing.assert_array_equal(again.sed, plain.sed)
    kp = calc.calculate_kpath_sed("x", 1.0, 6, segments=seg)
    kg = calc.calculate_kgrid_sed("xy", (-1, 1, -1, 1), 2, 3, segments=seg)
    assert kp.sed.shape == (16, 6) and kg.sed.shape == (16, 6) and kg.k_grid_shape == (2, 3)


def test_cleared_after_a_failure_and_validated_first():
    import conftest
    d = _golden()
    eng = SegmentOracleEngine(fail=True)
    calc = conftest.make_calculator(d).attach(engine=eng)
    mags, vecs = calc.get_k_path("x", 1.0, 4)
    calc.calculate(mags, vecs)                                   # resident: the next call goes to engine.calculate
    with pytest.raises(_hip.PsaHipError):
        calc.calculate(mags, vecs, segments=Segments(8))
    assert eng.segments is None and eng.segment_calls[-1] is None
    n = len(eng.segment_calls)
    T = calc.traj.n_frames
    with pytest.raises(ValueError):
        calc.calculate(mags, vecs, segments=Segments(T + 1))     # L > T: refused before the engine hears of it
    with pytest.raises(TypeError):
        calc.calculate(mags, vecs, segments=16)
    with pytest.raises(TypeError):                               # keyword only
        calc.calculate(mags, vecs, None, None, "coherent", None, 500, None, Segments(8))
    assert len(eng.segment_calls) == n


def test_refusals_without_a_gpu():
    import conftest
    d = _golden()
    eng = SegmentOracleEngine()
    calc = conftest.make_calculator(d).attach(engine=eng)
    seg = Segments(8)
    with pytest.raises(ValueError, match="chiral"):
        calc.calculate_kpath_sed("x", 1.0, 4, chiral=True, segments=seg)
    with pytest.raises(ValueError, match="chiral"):
        calc.calculate_kgrid_sed("xy", (-1, 1, -1, 1), 2, 2, chiral=True, segments=seg)
    with pytest.raises(ValueError, match="chiral"):
        calc.calculate_chiral_sed("x", 1.0, 4, segments=seg)
    stub = types.SimpleNamespace(nranks=2, mode="k", engine=SegmentOracleEngine(), run=None)
    sharded = conftest.make_calculator(d).attach(shard_group=stub)
    mags, vecs = sharded.get_k_path("x", 1.0, 4)
    with pytest.raises(NotImplementedError):
        sharded.calculate(mags, vecs, segments=seg)
    with pytest.raises(NotImplementedError):
        sharded.calculate_kpath_sed("x", 1.0, 4, segments=seg)
    assert eng.segment_calls == [] and stub.engine.segment_calls == []


def test_project64_matches_ref64():
    """the restatement's q is ref64's SED before its FFT"""
    from ref64 import sed64
    d = _golden()
    mean = np.mean(d["positions"], axis=0, dtype=np.float32)
    k = np.float32([[0.1, 0.2, 0.0], [0.5, 0.0, 0.3]])
    q = project64(d["velocities"], mean, k)
    s = sed64(d["velocities"], mean, k)
    np.testing.assert_allclose(np.fft.fft(q, axis=0) / q.shape[0], s, rtol=0, atol=1e-12 * np.max(np.abs(s)))
