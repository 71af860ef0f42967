"""Welch-averaged mode spectra without a GPU: the float64 restatement (tests/modes_welch64.py) against the identities
that tie it to the mode-projected SED and to the segment-averaged SED; the proof that the contraction kernel's
per-element bound can fail; what `calculate_mode_sed(segments=...)` and `calculate_mode_peaks(segments=...)` validate and
hand to the engine (a small stand-in defined here); the binding, header and Makefile entries; and a planted stationary
Lorentzian mode whose frequency and width the float64 fit of the float64 restatement recovers.

Figures this file prints.  The bound's proof on the six kernel cases: float32 chain 4.1 .. 7.6 u against bounds of
25 .. 495 u; one dropped term 2238 .. 670646 x the bound; one term truncated to bfloat16 8.4 .. 10099 x the bound at a
global rel_max of 6e-8 .. 1.5e-6.  The planted mode (float64, 8 seeds of the planted AR(1) mode, T = 4096, Segments(512, 256, "hann")): status 0 on
every seed, |f0 - planted| 0.03 .. 0.27 planted half widths, fitted / planted half width 0.73 .. 1.35."""
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

import fit64                                                      # noqa: E402
import modes64 as M64                                             # noqa: E402
import modes_welch64 as W64                                       # noqa: E402
import welch64                                                    # noqa: E402
from psa_amd import ModeSED, PeakFit, Segments, _hip, site_groups  # noqa: E402


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _case64(seed=4, N=48, T=40, K=4, B=4):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((T, N, 3)).astype(np.float32)
    mean = (rng.random((N, 3)) * 11.0).astype(np.float32)
    k = (rng.standard_normal((K, 3)) * 0.8).astype(np.float32)
    return data, mean, k, site_groups(np.arange(N) % B), (0.5 + rng.random(N)).astype(np.float32)


# --------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("weighted", [False, True])
def test_one_boxcar_segment_is_the_mode_sed(weighted):
    data, mean, k, groups, w = _case64()
    w = w if weighted else None
    T = data.shape[0]
    eig = M64.random_unitary(np.random.default_rng(3), len(k), len(groups), 5)
    phi, a2 = W64.mode_welch64(data, mean, k, groups, eig, Segments(T, T, "boxcar"), w)
    ref, A = M64.contract64(M64.spectra64(data, mean, k, groups, w), eig)
    assert phi.shape == (T, len(k), 5)
    assert _rel(phi, ref) <= 1e-12 and _rel(a2, A * A) <= 1e-12
    assert np.all(phi <= a2 * (1 + 1e-12))


@pytest.mark.parametrize("seg", [Segments(16, 8, "hann"), Segments(12, 16, "boxcar"), Segments(40, 40, "hann")],
                         ids=["hann_16_8", "boxcar_12_16", "hann_40_40"])
def test_cartesian_vectors_sum_to_the_welch_intensity(seg):
    data, mean, k, groups, w = _case64()
    B, K = len(groups), len(k)
    for b in range(B):
        eig = np.zeros((K, 3, B, 3), np.complex64)
        for c in range(3):
            eig[:, c, b, c] = 1.0
        phi, _ = W64.mode_welch64(data, mean, k, groups, eig, seg, w)
        ref = welch64.welch_intensity64(data, mean, k, [groups[b]], seg.window_array(), seg.length, seg.hop, w)
        assert phi.shape == (seg.length, K, 3)
        # welch64 projects with NumPy's cos/sin of the float32 argument, ref64 with the chain form of the same argument:
        # the two agree to the rounding of float64, not to the last bit
        assert _rel(phi.sum(axis=-1), ref) <= 1e-12


def test_bound_and_cases():
    assert W64.bound(8, 7) == (96 + 11 + 14) * W64.U and W64.bound(1, 1) == 25 * W64.U
    assert [c[:4] for c in W64.CASES] == [tuple(c) for c in M64.CASES]             # the parent's shapes, L for T
    assert sorted({c[4] for c in W64.CASES}) == [1, 2, 3, 7]
    S, e = W64.kernel_case(2, 6, 40, 3, 3)
    phi, a2 = W64.contract_welch64(S, e, 0.5)
    assert S.shape == (2, 3, 3, 3, 40) and phi.shape == a2.shape == (40, 3, 6)
    assert W64.per_element(phi, phi, a2) == 0.0
    off = phi.copy()
    off[3, 1, 2] += 5 * W64.U * a2[3, 1, 2]
    assert W64.per_element(off, phi, a2) == pytest.approx(5 * W64.U, rel=1e-6)


@pytest.mark.parametrize("case", W64.CASES, ids=[f"B{c[0]}_M{c[1]}_ns{c[4]}" for c in W64.CASES])
def test_bound_can_fail(case):
    """On the inputs of the GPU test: the float32 chain without FMA is under the bound; with ONE term of ONE segment
    dropped, or that term truncated to bfloat16, it is over it -- the truncated output's global rel_max is printed
    beside it"""
    B, Mv, L, K, ns = case
    S, e = W64.kernel_case(B, Mv, L, K, ns)
    scale = W64.kernel_scale(ns)
    ref, a2 = W64.contract_welch64(S, e, float(scale))
    k, s = K - 1, ns - 1                                   # the quietest k-point (rel_max looks at the loudest), the last segment
    b, c = M64.loudest_term(S[:, :, :, s, :], k)
    good = W64.chain32(S, e, scale)
    trunc = W64.chain32(S, e, scale, truncate=(s, k, b, c))
    drop = W64.chain32(S, e, scale, drop=(s, k, b, c))
    g, t, d = (W64.per_element(x, ref, a2) for x in (good, trunc, drop))
    bnd = W64.bound(B, ns)
    print(f"B={B} M={Mv} L={L} K={K} ns={ns}: bound {bnd / W64.U:.0f} u, chain {g / W64.U:.1f} u, truncated term "
          f"{t / bnd:.1f} x bound at rel_max {_rel(trunc, ref):.2e}, dropped term {d / bnd:.0f} x bound")
    assert g <= bnd
    assert d > bnd
    assert t > bnd


# --------------------------------------------------------------------------------------------------- the calculator
class WelchStandIn:
    """What the mode methods need of an engine: residency, weights, segments, the four mode entry points (the float64
    restatements as float32; the fits by tests/fit64.py), and a log of the calls in order."""

    def __init__(self, fail=False):
        self.lock = threading.RLock()
        self.slots, self.held, self.log = {}, {}, []
        self.weights, self.segments, self.segment_length, self.fail = None, None, 0, fail
        self.rank, self.nranks = 0, 1

    def is_resident(self, slot, array):
        return self.held.get(slot) is array

    def ensure_resident(self, slot, array):
        if not self.is_resident(slot, array):
            self.log.append(("upload", slot, self.segment_length))
            self.slots[slot], self.held[slot] = np.asarray(array, np.float32), array

    def mean_positions(self, slot):
        return np.mean(self.slots[slot], axis=0, dtype=np.float32)

    def set_atom_weights(self, w):
        self.log.append(("weights", None if w is None else w.copy()))
        self.weights = w

    def set_segments(self, segments):
        self.log.append(("segments", segments))
        self.segments, self.segment_length = segments, 0 if segments is None else segments.length

    def _groups(self, slot, groups):
        return [np.arange(self.slots[slot].shape[1])] if groups is None else groups

    def sed_modes(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, flags=0):
        self.log.append(("modes", slot, flags))
        return M64.mode_sed64(self.slots[slot], mean_pos_all, k_vectors, self._groups(slot, groups), eigenvectors, self.weights,
                              bool(flags & _hip.F_DISPLACEMENTS)).astype(np.float32)

    def sed_modes_welch(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, flags=0):
        self.log.append(("modes_welch", slot, flags, self.segments))
        if self.fail:
            raise _hip.PsaHipError("injected failure")
        return W64.mode_welch64(self.slots[slot], mean_pos_all, k_vectors, self._groups(slot, groups), eigenvectors, self.segments,
                                self.weights, bool(flags & _hip.F_DISPLACEMENTS))[0].astype(np.float32)

    def _fit(self, phi, df):
        F, K, M = phi.shape
        fit, info = fit64.fit(phi.reshape(F, K * M), df)
        return PeakFit.from_arrays(fit.astype(np.float32), info.astype(np.int32), (K, M))

    def sed_modes_fit(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, df, flags=0, *, return_sed=False, **kw):
        self.log.append(("modes_fit", df))
        phi = self.sed_modes(slot, mean_pos_all, k_vectors, groups, eigenvectors, flags)
        return self._fit(phi, df), (phi if return_sed else None)

    def sed_modes_welch_fit(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, df, flags=0, *, return_sed=False, **kw):
        self.log.append(("modes_welch_fit", df, self.segments))
        phi = self.sed_modes_welch(slot, mean_pos_all, k_vectors, groups, eigenvectors, flags)
        return self._fit(phi, df), (phi if return_sed else None)


def _golden(name="a"):
    import conftest
    with np.load(conftest.GOLDEN / f"traj_{name}.npz") as z:
        d = {k: z[k] for k in z.files}
    d["dt_ps"], d["cells"] = float(d["dt_ps"]), tuple(int(v) for v in d["cells"])
    return d


def _setup(fail=False):
    import conftest
    d = _golden()
    eng = WelchStandIn(fail)
    calc = conftest.make_calculator(d).attach(engine=eng)
    mags, vecs = calc.get_k_path("100", 1.0, 3)
    groups = site_groups(np.arange(calc.traj.n_atoms) % 2)
    eig = M64.random_unitary(np.random.default_rng(2), 3, 2, 4)
    return d, eng, calc, mags, vecs, groups, eig


def test_segments_reach_the_engine_and_are_cleared():
    d, eng, calc, mags, vecs, groups, eig = _setup()
    tr = calc.traj
    T = tr.n_frames
    L = max(12, T // 2)
    seg = Segments(L, max(1, L // 2), "hann")
    mean = np.mean(tr.positions, axis=0, dtype=np.float32)
    got = calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg)
    assert isinstance(got, ModeSED) and got.sed.shape == (L, 3, 4) and got.sed.dtype == np.float32
    assert np.array_equal(got.freqs, np.fft.fftfreq(L, d=d["dt_ps"]))
    # set inside the lock and before the upload (its FFT primer then builds length L), cleared afterwards
    assert [e[0] for e in eng.log] == ["segments", "upload", "modes_welch", "segments"]
    assert eng.log[0][1] is seg and eng.log[1][2] == L and eng.log[2][3] is seg and eng.log[3][1] is None
    assert eng.segment_length == 0
    assert _rel(got.sed, W64.mode_welch64(tr.velocities, mean, vecs, groups, eig, seg)[0]) <= 1e-6

    # without segments: exactly the calls of before
    eng.log.clear()
    plain = calc.calculate_mode_sed(mags, vecs, eig, groups)
    assert [e[0] for e in eng.log] == ["modes"] and plain.sed.shape == (T, 3, 4)
    eng.log.clear()
    fit = calc.calculate_mode_peaks(mags, vecs, eig, groups)
    assert [e[0] for e in eng.log] == ["modes_fit", "modes"] and eng.log[0][1] == 1.0 / (T * d["dt_ps"])
    assert isinstance(fit, PeakFit)

    # the fit: df of the segment transform, spectra with L rows
    eng.log.clear()
    fit, sed = calc.calculate_mode_peaks(mags, vecs, eig, groups, segments=seg, return_sed=True, atom_weights=np.ones(tr.n_atoms))
    assert [e[0] for e in eng.log] == ["weights", "segments", "modes_welch_fit", "modes_welch", "weights", "segments"]
    assert eng.log[2][1] == 1.0 / (L * d["dt_ps"]) and eng.log[2][2] is seg
    assert eng.segment_length == 0 and eng.weights is None
    assert fit.frequency.shape == (3, 4) and sed.sed.shape == (L, 3, 4)
    assert np.array_equal(sed.freqs, np.fft.fftfreq(L, d=d["dt_ps"]))


def test_segments_cleared_after_a_failure():
    d, eng, calc, mags, vecs, groups, eig = _setup(fail=True)
    seg = Segments(12, 6)
    with pytest.raises(_hip.PsaHipError):
        calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg, atom_weights=np.ones(calc.traj.n_atoms, np.float32))
    assert eng.segment_length == 0 and eng.segments is None and eng.weights is None
    with pytest.raises(_hip.PsaHipError):
        calc.calculate_mode_peaks(mags, vecs, eig, groups, segments=seg)
    assert eng.segment_length == 0 and eng.segments is None


def test_segment_validation():
    import conftest
    d, eng, calc, mags, vecs, groups, eig = _setup()
    T = calc.traj.n_frames
    for method in (calc.calculate_mode_sed, calc.calculate_mode_peaks):
        with pytest.raises(TypeError, match="Segments"):
            method(mags, vecs, eig, groups, segments=(12, 6))
        with pytest.raises(ValueError, match="exceeds"):
            method(mags, vecs, eig, groups, segments=Segments(T + 1))
        with pytest.raises(TypeError):                                                # keyword only
            method(mags, vecs, eig, groups, None, Segments(12))
    assert eng.log == []                                                              # refused before the engine hears of it
    empty_k = calc.calculate_mode_sed(np.zeros(0, np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 5, 2, 3), np.complex64),
                                      groups, segments=Segments(12, 6))
    assert empty_k.sed.shape == (12, 0, 5) and empty_k.freqs.shape == (12,) and eng.log == []
    stub = types.SimpleNamespace(nranks=2, mode="k", engine=WelchStandIn(), run=None)
    sharded = conftest.make_calculator(d).attach(shard_group=stub)
    with pytest.raises(NotImplementedError):
        sharded.calculate_mode_sed(mags, vecs, eig, groups, segments=Segments(12, 6))
    assert stub.engine.log == []


# --------------------------------------------------------------------------------------------------- package surface
def test_binding_header_and_makefile():
    new = ("psa_sed_modes_welch", "psa_sed_modes_welch_fit", "psa_debug_mode_power_welch")
    assert all(n in _hip.SIGNATURES for n in new) and _hip.ABI_VERSION == 6
    assert len(_hip.SIGNATURES["psa_sed_modes_welch"][1]) == len(_hip.SIGNATURES["psa_sed_modes"][1])
    assert len(_hip.SIGNATURES["psa_sed_modes_welch_fit"][1]) == len(_hip.SIGNATURES["psa_sed_modes_fit"][1])
    assert len(_hip.SIGNATURES["psa_debug_mode_power_welch"][1]) == 11
    for name in ("sed_modes_welch", "sed_modes_welch_fit", "debug_mode_power_welch"):
        assert hasattr(_hip.Engine, name)
    lib = _hip.load_library()
    assert lib.psa_abi_version() == 6 and all(getattr(lib, n) for n in new)
    header = (HERE.parent / "include" / "psa_hip.h").read_text()
    assert all(f"int {n}(" in header for n in new) and "#define PSA_HIP_ABI_VERSION 6" in header
    mk = (HERE.parent / "psa_amd" / "csrc" / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " modes.hip" in srcs and " api_modes.hip" in srcs
    import re
    assert re.search(r"for f in [^;]*\bmodes\b[^;]*; do", mk)                         # the asm list
    assert all((HERE.parent / "psa_amd" / "csrc" / f).is_file() for f in srcs.split(":=")[1].split())


def test_debug_binding_checks_its_arguments():
    eng = object.__new__(_hip.Engine)                                                  # no context: refused before any call
    e = np.zeros((3, 2, 2, 3), np.complex64)
    with pytest.raises(ValueError, match="do not fit"):
        _hip.Engine.debug_mode_power_welch(eng, np.zeros((2, 3, 3, 8), np.complex64), e)          # no segment axis
    with pytest.raises(ValueError, match="do not fit"):
        _hip.Engine.debug_mode_power_welch(eng, np.zeros((2, 4, 3, 2, 8), np.complex64), e)       # K mismatch
    with pytest.raises(ValueError, match="do not fit"):
        _hip.Engine.debug_mode_power_welch(eng, np.zeros((1, 3, 3, 2, 8), np.complex64), e)       # B mismatch
    with pytest.raises(ValueError, match="seg_block"):
        _hip.Engine.debug_mode_power_welch(eng, np.zeros((2, 3, 3, 2, 8), np.complex64), e, seg_block=-1)


# --------------------------------------------------------------------------------------------------- a planted mode
def test_planted_lorentzian_mode_is_recovered():
    """T = 4096, Segments(512, 256, "hann"): 15 segments; peak near bin 60.3 of 512, half width 6 bins.  Conditions, not
    measurements: status 0, f0 within one planted half width, hwhm within a factor 2."""
    assert 1 + (W64.PLANTED_T - W64.PLANTED_L) // W64.PLANTED_H == 15
    f0, hw = W64.planted_truth()
    for seed in range(8):
        fit, info, _ = W64.planted_fit64(seed)
        print(f"seed {seed}: status {info[0]}, {info[1]} iterations, window {info[3]} bins, f0 off by {(fit[0] - f0) / hw:+.3f} "
              f"half widths, hwhm {fit[1] / hw:.3f} of the planted")
        assert info[0] == 0
        assert abs(fit[0] - f0) <= hw
        assert 0.5 * hw <= fit[1] <= 2.0 * hw
