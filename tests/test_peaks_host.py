"""The Lorentzian peak fit without a GPU: the float64 restatement (tests/fit64.py) recovers planted parameters and holds
every case the GPU tests assert against its own float32-arithmetic copy at the bound; the comparison can fail; the window
rule and the band arithmetic on hand-written inputs; validation, `PeakFit`, the calculator's call into the engine; the ABI
and the build list."""
import re
import threading
import types
from pathlib import Path

import numpy as np
import pytest

import fit64 as F64
from psa_amd import PeakFit, _hip, peaks

HERE = Path(__file__).resolve().parent
DT = 0.002


def _df(F):
    return 1.0 / (F * DT)


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", F64.SHAPES, ids=str)
def test_fit64_recovers_planted_parameters(shape):
    """one Lorentzian on a constant: the model itself, known to the rounding of the float32 samples"""
    phi, truth = F64.clean_case(*shape, mirror_height=0.0)
    df = _df(shape[0])
    fit, info = F64.fit(phi, df)
    assert (info[:, 0] == 0).all()
    planted = truth.copy()
    planted[:, :2] *= df
    m = F64.compare(fit[:, :4], planted)
    print(f"{shape}: planted parameters recovered to {max(m):.2e} (f0, hwhm, height, baseline: {m})")
    assert max(m) <= 1e-4
    assert np.array_equal(fit[:, 5], np.round(truth[:, 0]))                       # the peak bin


def test_fit64_recovers_a_ringdown():
    """|FFT|^2 of exp(-Gamma t + i omega0 t): omega0 at bin 100.3, hwhm 6 bins of 1024"""
    T, bin0, w = 1024, 100.3, 6.0
    phi = F64.ringdown(T, bin0, w).astype(np.float32)[:, None]
    df = _df(T)
    fit, info = F64.fit(phi, df)
    e_f0, e_w = abs(fit[0, 0] / df - bin0) / w, abs(fit[0, 1] / df / w - 1)
    print(f"ring-down: |f0 - truth| / hwhm = {e_f0:.2e}, |hwhm / truth - 1| = {e_w:.2e}, status {info[0, 0]}, window {info[0, 2:]}")
    assert info[0, 0] == 0 and e_f0 < 1e-4 and e_w < 1e-4


def _asserted_cases():
    for shape in F64.SHAPES:
        yield f"clean{shape}", F64.clean_case(*shape)[0], _df(shape[0])
    yield "noisy(1024, 130)", F64.noisy_case(1024, 130)[0], _df(1024)


@pytest.mark.parametrize("name,phi,df", list(_asserted_cases()), ids=[c[0] for c in _asserted_cases()])
def test_float32_copy_meets_the_bound(name, phi, df):
    """every case of tests/test_gpu_peaks.py, float32 arithmetic against float64 on the CPU: same windows, the four
    measures within BOUND, rss within its tolerance"""
    ref, ref_info = F64.fit(phi, df)
    got, got_info = F64.fit32(phi, df)
    assert (ref_info[:, 0] == 0).all() and (got_info[:, 0] == 0).all()
    assert np.array_equal(ref_info[:, 2:], got_info[:, 2:]) and np.array_equal(ref[:, 5], got[:, 5])
    m = F64.compare(got, ref)
    print(f"{name}: float32 copy against float64 {m}, iterations {ref_info[:, 1].max()} / {got_info[:, 1].max()}, "
          f"windows {ref_info[:, 3].min()} .. {ref_info[:, 3].max()}")
    assert max(m) <= F64.BOUND
    assert F64.rss_agrees(got, ref, ref_info).all()


def test_cases_reach_the_window_sizes():
    """windows below, at and above one 64-bin chunk, and the 4095-bin cap"""
    sizes = set()
    for shape in F64.SHAPES:
        sizes |= set(F64.fit(F64.clean_case(*shape)[0], _df(shape[0]), max_iter=1)[1][:, 3].tolist())
    assert min(sizes) < 64 and 64 in sizes and 4095 in sizes and any(64 < s < 4095 for s in sizes)


def test_comparison_can_fail():
    phi, _ = F64.clean_case(256, 15)
    ref, _ = F64.fit(phi, _df(256))
    assert F64.within(ref, ref)
    for i in range(4):
        off = ref.copy()
        off[7, i] += 1e-3 * (ref[7, 1] if i < 2 else ref[7, 2])
        m = F64.compare(off, ref)
        assert not F64.within(off, ref) and m[i] == pytest.approx(1e-3, rel=1e-6) and max(m[:i] + m[i + 1:]) == 0.0
    with pytest.raises(AssertionError):
        F64.compare(np.full_like(ref, np.nan), ref)


# ------------------------------------------------------------------------------------------------- window and status
def test_window_rule():
    z = np.zeros(64, np.float32)
    # a tie: the lowest bin wins; its right neighbour (equal) counts into the run
    a = z.copy()
    a[[20, 21]] = 4.0
    a[22] = 2.0                                     # exactly half: inside (>=)
    a[19] = 1.9
    assert F64.window(a, 1, 32) == (20, 1.5, 8, 32)               # l = 0, r = 2: h0 = 1.5, n = 12 -> [8, 33) cut at the band's end
    assert F64.window(a, 1, 32, window_hwhm=1.0) == (20, 1.5, 16, 25)  # n = ceil(1.5) = 2 -> the clamp at 4
    # a plateau up to the band's upper end, a band that starts on the peak
    b = z.copy()
    b[10:30] = 1.0
    assert F64.window(b, 10, 30) == (10, 10.0, 10, 30)            # l = 0, r = 19, h0 = 10, n = 80: both ends clipped
    assert F64.window(b, 5, 32) == (10, 10.0, 5, 32)
    assert F64.window(b, 5, 32, half_window_bins=6) == (10, 10.0, 5, 17)
    assert F64.window(b, 5, 32, half_window_bins=1) == (10, 10.0, 6, 15)       # clamp at 4
    # the clamp at 2047
    c = np.ones(8192, np.float32)
    c[3000] = 1.5
    assert F64.window(c, 1, 4096) == (3000, 2047.5, 953, 4096)
    assert F64.window(c, 1, 4096, half_window_bins=5000) == (3000, 2047.5, 953, 4096)
    c[2048] = 2.5
    p, h0, lo, hi = F64.window(c, 1, 4096, window_hwhm=3000.0)
    assert (p, h0, lo, hi) == (2048, 1.0, 1, 4096) and hi - lo == 4095
    # nothing to fit
    assert F64.window(z, 1, 32) is None and F64.window(a, 18, 22) is None       # no positive value; 4 bins
    d = a.copy()
    d[40] = np.nan
    assert F64.window(d, 1, 32) is not None and F64.window(d, 1, 41) is None    # NaN outside / inside the band
    d[40] = np.inf
    assert F64.window(d, 1, 41) is None


def test_statuses_of_the_restatement():
    phi, _ = F64.clean_case(256, 15)
    df = _df(256)
    col = phi[:, 3]
    fit, info = F64.fit_column(np.zeros(256, np.float32), 1, 128, df)
    assert info.tolist() == [2, 0, 0, 0] and np.isnan(fit).all()
    fit, info = F64.fit_column(col, 1, 128, df, max_iter=1)
    assert info[0] == 1 and info[1] == 1 and np.isfinite(fit).all()
    fit, info = F64.fit_column(np.full(256, 3.0, np.float32), 1, 128, df)
    assert info[0] in (0, 3) and np.isfinite(fit).all() and fit[3] == pytest.approx(3.0) and fit[2] == 0.0


# ------------------------------------------------------------------------------------------------- bands
def test_band_arithmetic():
    F, df = 100, 0.5
    assert peaks.positive_half(100) == (1, 50) and peaks.positive_half(101) == (1, 51) == F64.positive_half(101)
    assert peaks.peak_bands(F, df, 3).tolist() == [[1, 50]] * 3
    assert peaks.peak_bands(F, df, 2, band=(2.0, 10.0)).tolist() == [[4, 21]] * 2            # ceil(4), floor(20) + 1
    assert peaks.peak_bands(F, df, 1, band=(2.1, 9.9)).tolist() == [[5, 20]]
    assert peaks.peak_bands(F, df, 1, band=(0.0, 25.0)).tolist() == [[1, 50]]                # clipped: no DC, no Nyquist
    got = peaks.peak_bands(F, df, 3, band=(2.0, 20.0), centers=[3.0, 10.2, 19.5], search=1.5)
    assert got.tolist() == [[4, 10], [18, 24], [36, 41]] and got.dtype == np.int32           # cut to the band at both ends
    rng = np.random.default_rng(0)
    for _ in range(20):
        Fr, dfr = int(rng.integers(12, 500)), float(rng.uniform(0.01, 2.0))
        ny = 0.5 * Fr * dfr
        lo, hi = sorted(rng.uniform(0, ny, 2))
        c = rng.uniform(lo, hi, 7)
        kw = dict(band=(lo, hi), centers=c, search=0.2 * ny)
        try:
            mine = peaks.peak_bands(Fr, dfr, 7, **kw)
        except ValueError:
            continue
        assert np.array_equal(mine, F64.bands(Fr, dfr, 7, **kw))
    assert peaks.half_window_bins(None, df) == 0 and peaks.half_window_bins(5.2, df) == 10
    assert peaks.half_window_bins(0.1, df) == 4 and peaks.half_window_bins(1e6, df) == 2047


def test_python_validation():
    with pytest.raises(ValueError, match="search"):
        peaks.peak_bands(100, 0.5, 2, centers=[3.0, 4.0])
    with pytest.raises(ValueError, match="search"):
        peaks.peak_bands(100, 0.5, 2, search=1.0)
    with pytest.raises(ValueError, match="Nyquist"):
        peaks.peak_bands(100, 0.5, 2, band=(1.0, 25.1))
    with pytest.raises(ValueError, match="Nyquist"):
        peaks.peak_bands(100, 0.5, 2, band=(-0.1, 5.0))
    with pytest.raises(ValueError, match="Nyquist"):
        peaks.peak_bands(100, 0.5, 2, band=(5.0, 5.0))
    with pytest.raises(ValueError, match="no frequency bin"):
        peaks.peak_bands(100, 0.5, 2, band=(5.1, 5.4))
    with pytest.raises(ValueError, match="3 values for 2"):
        peaks.peak_bands(100, 0.5, 2, centers=[1.0, 2.0, 3.0], search=1.0)
    with pytest.raises(ValueError, match="column 1"):
        peaks.peak_bands(100, 0.5, 2, band=(2.0, 10.0), centers=[3.0, 15.0], search=1.0)
    with pytest.raises(ValueError, match="at least 12"):
        peaks.peak_bands(11, 0.5, 2)
    with pytest.raises(ValueError, match="df"):
        peaks.peak_bands(100, 0.0, 2)
    for bad in (np.zeros((11, 3), np.float32), np.zeros((20, 0), np.float32), np.zeros((20, 2, 2, 2), np.float32),
                np.zeros((20, 2), np.complex64)):
        with pytest.raises(ValueError):
            peaks.spectrum_columns(bad)
    spec, shape = peaks.spectrum_columns(np.ones((20, 3, 2), np.float64)[:, ::-1])
    assert spec.shape == (20, 6) and spec.dtype == np.float32 and spec.flags.c_contiguous and shape == (3, 2)
    assert peaks.spectrum_columns(np.ones(20))[1] == ()
    with pytest.raises(ValueError, match="window_hwhm"):
        peaks.check_fit_options(0.0, 50)
    with pytest.raises(ValueError, match="max_iter"):
        peaks.check_fit_options(8.0, 0)
    with pytest.raises(ValueError, match="half_window"):
        peaks.half_window_bins(-1.0, 0.5)
    with pytest.raises(ValueError, match="dt_ps or freqs"):
        peaks.fit_peaks(np.ones((20, 2), np.float32))
    with pytest.raises(ValueError, match="dt_ps or freqs"):
        peaks.fit_peaks(np.ones((20, 2), np.float32), dt_ps=0.1, freqs=np.fft.fftfreq(20, 0.1))
    with pytest.raises(ValueError, match="freqs has shape"):
        peaks.fit_peaks(np.ones((20, 2), np.float32), freqs=np.fft.fftfreq(21, 0.1))


def test_peakfit_container():
    fit = np.array([[2.0, 0.25, 3.0, 0.1, 1e-3, 17.0], [np.nan] * 6], np.float32)
    info = np.array([[0, 7, 9, 17], [2, 0, 0, 0]], np.int32)
    pf = PeakFit.from_arrays(np.tile(fit, (3, 1)), np.tile(info, (3, 1)), (3, 2))
    assert pf.frequency.shape == pf.status.shape == (3, 2) and pf.window.shape == (3, 2, 2)
    assert pf.window[0, 0].tolist() == [9, 26] and pf.window[0, 1].tolist() == [0, 0]
    assert pf.peak_bin.tolist() == [[17, 0]] * 3 and pf.iterations[1, 0] == 7
    assert pf.ok.tolist() == [[True, False]] * 3
    assert pf.lifetime[0, 0] == pytest.approx(1.0 / (4.0 * np.pi * 0.25)) and np.isnan(pf.lifetime[0, 1])
    assert pf.fwhm[0, 0] == 0.5
    flat = PeakFit.from_arrays(fit, info, (2,))
    assert flat.hwhm.shape == (2,) and flat.window.shape == (2, 2)
    import psa_amd
    assert "PeakFit" in psa_amd.__all__ and "fit_peaks" in psa_amd.__all__ and psa_amd.fit_peaks is peaks.fit_peaks


# ------------------------------------------------------------------------------------------------- the calculator
class PeaksStandIn:
    """What `calculate_mode_peaks` needs of an engine, with a log of the calls in order"""

    def __init__(self, fail=False):
        self.lock = threading.RLock()
        self.held, self.log, self.weights, self.fail = {}, [], None, fail
        self.rank, self.nranks, self.segment_length = 0, 1, 0

    def is_resident(self, slot, array):
        return self.held.get(slot) is array

    def ensure_resident(self, slot, array):
        self.held[slot] = array

    def mean_positions(self, slot):
        return np.mean(np.asarray(self.held[slot], np.float32), axis=0, dtype=np.float32)

    def set_atom_weights(self, w):
        self.log.append(("weights", w is not None))
        self.weights = w

    def sed_modes_fit(self, slot, mean_pos_all, k_vectors, groups, eigenvectors, df, flags=0, **kw):
        self.log.append(("fit", slot, flags, df, eigenvectors.shape, kw))
        if self.fail:
            raise _hip.PsaHipError("injected failure")
        K, M = eigenvectors.shape[:2]
        T = self.held[slot].shape[0]
        pf = PeakFit.from_arrays(np.ones((K * M, 6), np.float32), np.zeros((K * M, 4), np.int32), (K, M))
        return pf, (np.ones((T, K, M), np.float32) if kw["return_sed"] else None)


def _golden(name="a"):
    import conftest
    with np.load(conftest.GOLDEN / f"traj_{name}.npz") as z:
        d = {k: z[k] for k in z.files}
    d["dt_ps"], d["cells"] = float(d["dt_ps"]), tuple(int(v) for v in d["cells"])
    return d


def test_calculator_passes_the_call_on():
    import conftest
    from psa_amd import ModeSED
    d = _golden()
    eng = PeaksStandIn()
    calc = conftest.make_calculator(d).attach(engine=eng)
    T, N = calc.traj.n_frames, calc.traj.n_atoms
    mags, vecs = calc.get_k_path("100", 1.0, 4)
    two = [[0, 1, 2], [3, 4]]
    eig = np.ones((4, 5, 2, 3), np.complex128)
    pf = calc.calculate_mode_peaks(mags, vecs, eig, two)
    assert isinstance(pf, PeakFit) and pf.frequency.shape == (4, 5)
    call = eng.log[-1]
    assert call[:3] == ("fit", _hip.SLOT_VELOCITIES, 0) and call[3] == pytest.approx(1.0 / (T * d["dt_ps"])) and call[4] == (4, 5, 2, 3)
    assert call[5] == dict(return_sed=False, band=None, centers=None, search=None, window_hwhm=8.0, half_window=None, max_iter=50)
    eng.log.clear()
    pf, sed = calc.calculate_mode_peaks(mags, vecs, eig, two, atom_weights=np.ones(N), return_sed=True, band=(1.0, 2.0),
                                        centers=np.ones((4, 5)), search=0.5, window_hwhm=6.0, half_window=0.3, max_iter=9)
    assert isinstance(sed, ModeSED) and sed.sed.shape == (T, 4, 5) and np.array_equal(sed.freqs, np.fft.fftfreq(T, d=d["dt_ps"]))
    assert [e[0] for e in eng.log] == ["weights", "fit", "weights"] and eng.weights is None
    kw = eng.log[1][5]
    assert kw["return_sed"] and kw["band"] == (1.0, 2.0) and kw["search"] == 0.5 and kw["window_hwhm"] == 6.0
    assert kw["half_window"] == 0.3 and kw["max_iter"] == 9 and kw["centers"].shape == (4, 5)

    # the checks of calculate_mode_sed, before the engine hears of anything
    eng.log.clear()
    with pytest.raises(ValueError, match="expected"):
        calc.calculate_mode_peaks(mags, vecs, eig[:3], two)
    with pytest.raises(ValueError, match="disjoint"):
        calc.calculate_mode_peaks(mags, vecs, eig, [[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="nothing to fit"):
        calc.calculate_mode_peaks(np.zeros(0, np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 5, 2, 3), np.complex64), two)
    with pytest.raises(TypeError):
        calc.calculate_mode_peaks(mags, vecs, eig, two, None, np.ones(N))                 # keyword only
    stub = types.SimpleNamespace(nranks=2, mode="k", engine=PeaksStandIn(), run=None)
    with pytest.raises(NotImplementedError):
        conftest.make_calculator(d).attach(shard_group=stub).calculate_mode_peaks(mags, vecs, eig, two)
    assert eng.log == [] and stub.engine.log == []

    failing = PeaksStandIn(fail=True)
    calc2 = conftest.make_calculator(d).attach(engine=failing)
    with pytest.raises(_hip.PsaHipError):
        calc2.calculate_mode_peaks(mags, vecs, eig, two, atom_weights=np.ones(N))
    assert failing.weights is None


# ------------------------------------------------------------------------------------------------- ABI and build
def test_abi_declares_the_entry_points():
    header = (HERE.parent / "include" / "psa_hip.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+psa_fit_peaks\s*\(", body) and re.search(r"\bint\s+psa_sed_modes_fit\s*\(", body)
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*psa_peak_opts\s*;", body)
    assert struct and re.findall(r"(float|int32_t)\s+(\w+)\s*;", struct.group(1)) == [
        ("float", "window_hwhm"), ("int32_t", "half_window_bins"), ("int32_t", "max_iter")]
    assert [f[0] for f in _hip.PeakOpts._fields_] == ["window_hwhm", "half_window_bins", "max_iter"]
    import ctypes as C
    assert C.sizeof(_hip.PeakOpts) == 12
    assert "#define PSA_HIP_ABI_VERSION 6" in header and _hip.ABI_VERSION == 6
    assert len(_hip.SIGNATURES["psa_fit_peaks"][1]) == 11 and len(_hip.SIGNATURES["psa_sed_modes_fit"][1]) == 20
    assert hasattr(_hip.Engine, "fit_peaks") and hasattr(_hip.Engine, "sed_modes_fit")
    lib = _hip.load_library()
    assert lib.psa_abi_version() == 6 and lib.psa_fit_peaks and lib.psa_sed_modes_fit


def test_makefile_lists_the_sources():
    mk = (HERE.parent / "psa_amd" / "csrc" / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " peaks.hip" in srcs and " api_peaks.hip" in srcs
    assert re.search(r"for f in [^;]*\bpeaks\b[^;]*; do", mk)                 # the asm list
