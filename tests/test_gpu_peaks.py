"""The Lorentzian peak fit on the GPU (psa_fit_peaks, psa_sed_modes_fit; `Engine.fit_peaks`, `calculate_mode_peaks`)
against the float64 restatement tests/fit64.py: windows and peak bins exactly, the four measures of `fit64.compare`
within fit64.BOUND = 1e-4, rss within 1e-3 rss_ref + 1e-10 height^2 (b - a); the statuses and that a bad column leaves its
neighbours' bits alone; per-column bands; determinism; the mode projection end to end; a planted damped mode;
isolation from the SED entry points; ABI errors.  Each test prints its figures.

Measured on one MI355X (|df0|/hwhm, |dhwhm|/hwhm, |dheight|/height, |dbaseline|/height): clean (256, 15) 1.9e-6 / 5.2e-8 /
3.7e-8 / 2.4e-9; (100, 70) 1.1e-6 / 1.0e-7 / 5.5e-8 / 1.4e-8; (1024, 130) 7.8e-6 / 5.2e-8 / 5.4e-8 / 2.3e-9; (8192, 3) 2.8e-6 /
4.0e-8 / 3.5e-8 / 1.4e-9; 64-segment noise 1.0e-5 / 3.6e-7 / 9.8e-8 / 6.0e-8 (the first figure is the float32 rounding of f0
itself); rss within 5.4e-5 of its tolerance; centres on main and mirror peaks <= 7.8e-6; mode spectra (raw periodograms:
the float64 fit converges on 0 and 1 of 30 columns, the GPU's statuses are the same) 3.8e-6; planted damped mode f0
1.3e-6 hwhm, hwhm 5.4e-7 off."""
import ctypes as C

import numpy as np
import pytest

import fit64 as F64
from engine_state import reset

pytestmark = pytest.mark.gpu

DT = 0.002
B_SITES = 8


def _df(F):
    return 1.0 / (F * DT)


def _raw(engine, spec, df, bands=None, lo=0, hi=0, opts=(8.0, 0, 50), F=None, ncol=None, fit="alloc", info="alloc"):
    """psa_fit_peaks as the ABI has it: (rc, message, fit (C, 6), info (C, 4))"""
    from psa_amd import _hip
    spec = None if spec is None else np.ascontiguousarray(spec, np.float32)
    F = spec.shape[0] if F is None else F
    ncol = spec.shape[1] if ncol is None else ncol
    fit = np.full((max(ncol, 1), 6), -7.0, np.float32) if isinstance(fit, str) else fit
    info = np.full((max(ncol, 1), 4), -7, np.int32) if isinstance(info, str) else info
    b = None if bands is None else np.ascontiguousarray(bands, np.int32)
    o = None if opts is None else _hip.PeakOpts(*opts)
    rc = engine._lib.psa_fit_peaks(engine._h, None if spec is None else spec.ctypes.data_as(_hip._f32p), F, ncol, float(df),
                                   None if b is None else b.ctypes.data_as(_hip._i32p), lo, hi, None if o is None else C.byref(o),
                                   None if fit is None else fit.ctypes.data_as(_hip._f32p),
                                   None if info is None else info.ctypes.data_as(_hip._i32p))
    return rc, engine._lib.psa_last_error(), fit, info


def _half(F):
    return dict(lo=1, hi=(F + 1) // 2)


def _arrays(pf):
    """a PeakFit back as the (C, 6) and (C, 4) arrays of the ABI"""
    fit = np.stack([np.ravel(x) for x in (pf.frequency, pf.hwhm, pf.height, pf.baseline, pf.rss, pf.peak_bin.astype(np.float32))], axis=1)
    w = pf.window.reshape(-1, 2)
    return fit, np.stack([np.ravel(pf.status), np.ravel(pf.iterations), w[:, 0], w[:, 1] - w[:, 0]], axis=1)


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _hold(label, fit, info, ref, ref_info, statuses=(0,)):
    """the kernel's results against the restatement's on the columns the restatement fitted"""
    live = ref_info[:, 0] != 2
    assert np.array_equal(info[:, 0] == 2, ~live), (label, info[:, 0], ref_info[:, 0])
    assert np.array_equal(info[live][:, 2:], ref_info[live][:, 2:]), label                     # windows, exactly
    assert np.array_equal(fit[live][:, 5], ref[live][:, 5]), label                             # peak bins, exactly
    sel = np.isin(ref_info[:, 0], statuses)
    assert np.array_equal(info[sel][:, 0], ref_info[sel][:, 0]), (label, info[:, 0], ref_info[:, 0])
    if not sel.any():
        print(f"{label}: the float64 fit has no column of status {statuses} to compare")
        return None
    m = F64.compare(fit[sel], ref[sel])
    rss = np.abs(fit[sel][:, 4] - ref[sel][:, 4]) / (1e-3 * ref[sel][:, 4] + 1e-10 * ref[sel][:, 2] ** 2 * ref_info[sel][:, 3])
    print(f"{label}: {int(sel.sum())} columns, |df0|/hwhm {m[0]:.2e}, |dhwhm|/hwhm {m[1]:.2e}, |dheight|/height {m[2]:.2e}, "
          f"|dbaseline|/height {m[3]:.2e} (bound {F64.BOUND:.0e}); rss error / tolerance {rss.max():.2e}; "
          f"iterations {info[sel][:, 1].min()} .. {info[sel][:, 1].max()}, windows {info[sel][:, 3].min()} .. {info[sel][:, 3].max()}")
    assert max(m) <= F64.BOUND
    assert rss.max() <= 1.0
    return m


# ------------------------------------------------------------------------------------------------- 1, 2. against float64
_REF = {}


def _reference(name, shape):
    if (name, shape) not in _REF:
        phi = (F64.clean_case(*shape) if name == "clean" else F64.noisy_case(*shape))[0]
        _REF[name, shape] = (phi,) + F64.fit(phi, _df(shape[0]))
    return _REF[name, shape]


@pytest.mark.parametrize("shape", F64.SHAPES, ids=str)
def test_kernel_against_float64(engine, shape):
    phi, ref, ref_info = _reference("clean", shape)
    assert (ref_info[:, 0] == 0).all()
    rc, msg, fit, info = _raw(engine, phi, _df(shape[0]), **_half(shape[0]))
    assert rc == 0, msg
    _hold(f"clean {shape}", fit, info, ref, ref_info)
    pf = engine.fit_peaks(phi, _df(shape[0]))                                 # the Python door: the same bits
    assert pf.frequency.shape == (shape[1],) and pf.window.shape == (shape[1], 2) and pf.status.dtype == np.int32
    f2, i2 = _arrays(pf)
    assert _bits(f2, i2.astype(np.int32)) == _bits(fit, info) and pf.ok.all()
    assert np.allclose(pf.lifetime, 1.0 / (4.0 * np.pi * fit[:, 1]))


def test_kernel_against_float64_with_noise(engine):
    """64-segment chi-square noise on the (1024, 130) case"""
    phi, ref, ref_info = _reference("noisy", (1024, 130))
    assert (ref_info[:, 0] == 0).all()
    rc, msg, fit, info = _raw(engine, phi, _df(1024), **_half(1024))
    assert rc == 0, msg
    _hold("64-segment noise (1024, 130)", fit, info, ref, ref_info)


# ------------------------------------------------------------------------------------------------- 3. statuses
def test_statuses_and_their_neighbours(engine):
    """one bad column at a time in the (256, 15) case: its status, and the other 14 columns bit for bit as without it"""
    F, ncol, df = 256, 15, _df(256)
    phi, truth = F64.clean_case(F, ncol)
    top = (F + 1) // 2
    whole = np.tile(np.array([[1, top]], np.int32), (ncol, 1))
    rc, msg, base_fit, base_info = _raw(engine, phi, df, bands=whole)
    assert rc == 0, msg
    j = 5
    p = int(round(truth[j, 0]))

    def run(label, column=None, band=None, opts=(8.0, 0, 50), expect=None):
        spec, bands = phi.copy(), whole.copy()
        if column is not None:
            spec[:, j] = column
        if band is not None:
            bands[j] = band
        rc, msg, fit, info = _raw(engine, spec, df, bands=bands, opts=opts)
        assert rc == 0, (label, msg)
        if opts == (8.0, 0, 50):
            others = np.arange(ncol) != j
            assert _bits(fit[others], info[others]) == _bits(base_fit[others], base_info[others]), label
        ref, ref_info = F64.fit_column(spec[:, j], int(bands[j, 0]), int(bands[j, 1]), df, window_hwhm=opts[0],
                                       half_window_bins=opts[1], max_iter=opts[2])
        print(f"{label}: status {info[j, 0]} (float64: {ref_info[0]}), iterations {info[j, 1]}, window [{info[j, 2]}, +{info[j, 3]}), "
              f"fit {fit[j]}")
        if expect is not None:
            assert info[j, 0] == expect == ref_info[0], label
        if info[j, 0] == 2:
            assert np.isnan(fit[j]).all() and info[j].tolist() == [2, 0, 0, 0], label
        return fit, info, ref, ref_info

    run("a zero column", column=np.zeros(F, np.float32), expect=2)
    run("a negative column", column=np.full(F, -1.0, np.float32), expect=2)
    nan_in = phi[:, j].copy()
    nan_in[100] = np.nan
    run("NaN inside the band", column=nan_in, expect=2)
    inf_in = phi[:, j].copy()
    inf_in[p + 1] = np.inf
    run("infinity inside the band", column=inf_in, expect=2)
    fit_out, info_out, _, _ = run("NaN outside the band", column=nan_in, band=(1, 100), expect=0)
    fit_cl, info_cl, ref, ref_info = run("the same band without the NaN", band=(1, 100), expect=0)
    assert _bits(fit_out, info_out) == _bits(fit_cl, info_cl)
    _hold("band [1, 100)", fit_cl[j:j + 1], info_cl[j:j + 1], ref[None], ref_info[None])
    fit_c, info_c, _, _ = run("a constant column", column=np.full(F, 3.0, np.float32))
    fit_c2, info_c2, _, _ = run("a constant column again", column=np.full(F, 3.0, np.float32))
    assert info_c[j, 0] in (0, 3) and np.isfinite(fit_c[j]).all() and _bits(fit_c, info_c) == _bits(fit_c2, info_c2)
    run("a band of 4 bins", band=(p - 2, p + 2), expect=2)
    fit5, info5, ref, ref_info = run("a band of 5 bins", band=(p - 2, p + 3))
    assert info5[j, 0] != 2 and info5[j, 2:].tolist() == [p - 2, 5] == ref_info[2:].tolist()
    fit_e, info_e, ref, ref_info = run("the peak at the band's lower edge", band=(p, p + 60), expect=0)
    assert info_e[j, 2] == p and fit_e[j, 5] == p
    _hold("peak at the edge", fit_e[j:j + 1], info_e[j:j + 1], ref[None], ref_info[None])
    fit_s, info_s, ref, ref_info = run("a narrow band on the shoulder", band=(p + 2, p + 12), expect=3)
    assert fit_s[j, 5] == p + 2 and fit_s[j, 0] / df < p + 2                    # the maximum at the edge, the fitted centre outside
    _hold("shoulder", fit_s[j:j + 1], info_s[j:j + 1], ref[None], ref_info[None], statuses=(3,))
    fit_1, info_1, _, _ = run("max_iter = 1", opts=(8.0, 0, 1), expect=1)
    assert info_1[:, 0].tolist() == [1] * ncol and (info_1[:, 1] == 1).all() and np.isfinite(fit_1).all()
    assert np.array_equal(info_1[:, 2:], base_info[:, 2:])
    fit_h, info_h, ref, ref_info = run("half_window_bins = 9", opts=(8.0, 9, 50), expect=0)
    assert info_h[j, 2:].tolist() == [p - 9, 19]
    _hold("half_window_bins", fit_h[j:j + 1], info_h[j:j + 1], ref[None], ref_info[None])
    rc, msg, fit_d, info_d = _raw(engine, phi, df, opts=None, **_half(F))          # NULL options are the defaults, lo / hi the bands
    assert rc == 0 and _bits(fit_d, info_d) == _bits(base_fit, base_info)


# ------------------------------------------------------------------------------------------------- 4. per-column bands
def test_centers_point_at_one_of_two_peaks(engine):
    F, ncol = 1024, 130
    df = _df(F)
    phi, truth = F64.clean_case(F, ncol)
    top = (F + 1) // 2
    main = truth[:, 0]
    mirror = np.where(main < 0.5 * top, main + 0.35 * top, main - 0.35 * top)
    for name, centre, width in (("main", main, truth[:, 1]), ("mirror", mirror, 1.5 * truth[:, 1])):
        pf = engine.fit_peaks(phi, df, centers=centre * df, search=0.1 * top * df)
        bands = F64.bands(F, df, ncol, centers=centre * df, search=0.1 * top * df)
        ref, ref_info = F64.fit(phi, df, bands)
        fit, info = _arrays(pf)
        _hold(f"centres on the {name} peaks", fit, info, ref, ref_info, statuses=(0, 3))
        assert (pf.status == 0).sum() >= ncol - 5
        assert np.all(np.abs(pf.frequency / df - centre) < width) and np.all(np.abs(pf.peak_bin - centre) <= 1)
    both = engine.fit_peaks(phi, df, band=(0.5 * df, (top - 1) * df))
    assert np.all(np.abs(both.peak_bin - main) <= 1)                             # the global maximum without centres


# ------------------------------------------------------------------------------------------------- 5. determinism
def test_two_calls_and_another_column_split(engine):
    F, ncol = 1024, 130
    df = _df(F)
    phi = F64.noisy_case(F, ncol)[0]
    _, _, a_fit, a_info = _raw(engine, phi, df, **_half(F))
    _, _, b_fit, b_info = _raw(engine, phi, df, **_half(F))
    assert _bits(a_fit, a_info) == _bits(b_fit, b_info)
    wide = np.ascontiguousarray(np.concatenate([F64.clean_case(F, 70, seed=3)[0], phi, phi[:, ::-1], F64.noisy_case(F, 130, seed=5)[0]], axis=1))
    assert wide.shape[1] == 460                                                  # two column blocks of peak_find, other row slices
    rc, msg, w_fit, w_info = _raw(engine, wide, df, **_half(F))
    assert rc == 0, msg
    assert _bits(w_fit[70:200], w_info[70:200]) == _bits(a_fit, a_info)
    assert _bits(w_fit[200:330], w_info[200:330]) == _bits(a_fit[::-1], a_info[::-1])
    one = np.ascontiguousarray(phi[:, 17:18])
    _, _, o_fit, o_info = _raw(engine, one, df, **_half(F))
    assert _bits(o_fit, o_info) == _bits(a_fit[17:18], a_info[17:18])


# ------------------------------------------------------------------------------------------------- 6. end to end
def _trajectory(cells=(4, 4, 4), T=256, seed=3):
    """the synthetic silicon of tests/test_gpu_modes.py: 512 atoms, 8 basis sites, one planted mode"""
    from psa_amd import Trajectory, synth
    spec = synth.SyntheticSpec(cells, T, dt_ps=DT, seed=seed,
                               modes=[synth.Mode(3.0, 16, (2 * np.pi / synth.A_SI * 0.25, 0, 0), 0)])
    r0, types, box = synth.lattice(spec.cells)
    vel = synth.velocities_block(spec, synth.mode_tables(spec, r0), 0, T)
    pos = (r0[None] + 0.05 * np.random.default_rng(seed).standard_normal(vel.shape)).astype(np.float32)
    return Trajectory(pos, vel, types, np.arange(T, dtype=np.float32), box, np.diag(box).copy(),
                      np.zeros(3, np.float32), spec.dt_ps), spec.cells


@pytest.fixture(scope="module")
def syn(engine):
    import modes64 as M64
    from psa_amd import SEDCalculator, mass_weights, site_groups
    out = {}
    for T in (256, 100):
        tr, cells = _trajectory(T=T)
        calc = SEDCalculator(tr, *cells).attach(engine=engine)
        mags, vecs = calc.get_k_path("100", 1.0, 6)
        out[T] = dict(traj=tr, calc=calc, groups=site_groups(np.arange(tr.n_atoms) % B_SITES), mags=mags, vecs=vecs,
                      eig=M64.random_unitary(np.random.default_rng(5), len(vecs), B_SITES, 5),
                      weights=mass_weights(tr.types, {1: 1.0, 2: 207.0}))
    reset(engine)
    yield out
    reset(engine)
    engine.invalidate()


@pytest.mark.parametrize("T", [256, 100])
def test_mode_peaks_end_to_end(engine, syn, T):
    s = syn[T]
    calc, args = s["calc"], (s["mags"], s["vecs"], s["eig"], s["groups"])
    df = 1.0 / (T * DT)
    sed = calc.calculate_mode_sed(*args)
    pf = calc.calculate_mode_peaks(*args)
    K, M = len(s["vecs"]), s["eig"].shape[1]
    assert pf.frequency.shape == (K, M) and pf.window.shape == (K, M, 2) and pf.frequency.dtype == np.float32
    two_step = engine.fit_peaks(sed.sed, df)
    assert _bits(*_arrays(pf)) == _bits(*_arrays(two_step))
    pf2, sed2 = calc.calculate_mode_peaks(*args, return_sed=True)
    assert _bits(*_arrays(pf2)) == _bits(*_arrays(pf))
    assert sed2.sed.shape == sed.sed.shape and _bits(sed2.sed) == _bits(sed.sed) and np.array_equal(sed2.freqs, sed.freqs)
    ref, ref_info = F64.fit(sed.sed.reshape(T, K * M), df)
    fit, info = _arrays(pf)
    print(f"T={T}: float64 statuses {np.bincount(ref_info[:, 0], minlength=4).tolist()}, GPU {np.bincount(info[:, 0], minlength=4).tolist()}")
    _hold(f"mode spectra T={T}", fit, info, ref, ref_info)
    assert engine.segment_length == 0


# ------------------------------------------------------------------------------------------------- 7. a planted damped mode
def damped_trajectory(T=1024, bin0=100.3, hwhm_bins=6.0, amplitude=2.0, cells=(4, 4, 4), seed=4):
    """velocities A exp(-Gamma t) cos(k*.r_a - omega0 t) along x on the silicon lattice, k* = 0.25 * 2 pi / a along x,
    omega0 = 2 pi bin0 / T and Gamma = 2 pi hwhm_bins / T per frame; positions jitter around the lattice sites.  Projected
    on +k* only the exp(+i omega0 t) half of the cosine survives the lattice sum: a complex ring-down at bin +bin0."""
    from psa_amd import Trajectory, synth
    r0, types, box = synth.lattice(cells)
    k_star = np.array([2 * np.pi / synth.A_SI * 0.25, 0.0, 0.0])
    t = np.arange(T, dtype=np.float64)[:, None]
    vel = np.zeros((T, len(r0), 3), np.float32)
    vel[:, :, 0] = amplitude * np.exp(-2 * np.pi * hwhm_bins / T * t) * np.cos((r0.astype(np.float64) @ k_star)[None, :] - 2 * np.pi * bin0 / T * t)
    pos = (r0[None] + 0.05 * np.random.default_rng(seed).standard_normal(vel.shape)).astype(np.float32)
    traj = Trajectory(pos, vel, types, np.arange(T, dtype=np.float32), box, np.diag(box).copy(), np.zeros(3, np.float32), DT)
    return traj, cells, k_star.astype(np.float32)


def test_planted_damped_mode(engine):
    from psa_amd import SEDCalculator, site_groups
    T, bin0, w = 1024, 100.3, 6.0
    traj, cells, k_star = damped_trajectory(T, bin0, w)
    calc = SEDCalculator(traj, *cells).attach(engine=engine)
    eig = np.zeros((1, 1, B_SITES, 3), np.complex64)
    eig[0, 0, :, 0] = 1.0 / np.sqrt(B_SITES)
    try:
        pf = calc.calculate_mode_peaks(np.float32([np.linalg.norm(k_star)]), k_star[None], eig, site_groups(np.arange(traj.n_atoms) % B_SITES))
    finally:
        engine.invalidate()
    df = 1.0 / (T * DT)
    e_f0, e_w = abs(pf.frequency[0, 0] / df - bin0) / w, abs(pf.hwhm[0, 0] / df / w - 1.0)
    print(f"planted damped mode: status {pf.status[0, 0]}, f0 {pf.frequency[0, 0] / df:.4f} bins (planted {bin0}), hwhm "
          f"{pf.hwhm[0, 0] / df:.4f} bins (planted {w}); |f0 - truth| / hwhm = {e_f0:.2e}, |hwhm / truth - 1| = {e_w:.2e}; "
          f"lifetime {pf.lifetime[0, 0]:.4f} ps (planted {1.0 / (4 * np.pi * w * df):.4f})")
    assert pf.status[0, 0] == 0 and pf.peak_bin[0, 0] == 100
    assert e_f0 <= 1e-2 and e_w <= 1e-2


# ------------------------------------------------------------------------------------------------- 8. isolation, errors
def test_no_leak_into_sed_calls(engine, syn):
    from psa_amd import Segments, _hip
    s = syn[256]
    calc, tr = s["calc"], s["traj"]
    args = (s["mags"], s["vecs"], s["eig"], s["groups"])
    mean = np.mean(tr.positions, axis=0, dtype=np.float32)
    phi = F64.clean_case(256, 15)[0]
    for kw in ({}, dict(basis_atom_types=[1, 2], summation_mode="incoherent")):
        before = calc.calculate(s["mags"], s["vecs"], **kw)
        calc.calculate_mode_peaks(*args, atom_weights=s["weights"])
        engine.fit_peaks(phi, _df(256))
        after = calc.calculate(s["mags"], s["vecs"], **kw)
        assert after.sed.shape == before.sed.shape and _bits(after.sed) == _bits(before.sed)
    # a projection that has not been finalized yet survives both kinds of peak call
    mean = calc._mean_positions()
    engine.project(_hip.SLOT_VELOCITIES, mean, s["vecs"], None, 0)
    whole = np.array(engine.finalize(tr.n_frames, len(s["vecs"]), False))
    engine.project(_hip.SLOT_VELOCITIES, mean, s["vecs"], None, 0)
    calc.calculate_mode_peaks(*args)
    engine.fit_peaks(phi, _df(256))
    later = engine.finalize(tr.n_frames, len(s["vecs"]), False)
    assert _bits(np.asarray(later)) == _bits(whole)
    # the weights of a peaks call are gone afterwards, and the mode spectra are what they were
    plain = calc.calculate_mode_peaks(*args)
    sed_before = calc.calculate_mode_sed(*args).sed.copy()
    weighted = calc.calculate_mode_peaks(*args, atom_weights=s["weights"])
    assert _bits(*_arrays(weighted)) != _bits(*_arrays(plain))
    assert _bits(*_arrays(calc.calculate_mode_peaks(*args))) == _bits(*_arrays(plain))
    assert _bits(calc.calculate_mode_sed(*args).sed) == _bits(sed_before)
    assert engine.segment_length == 0
    # segments: the mode entry refuses them as psa_sed_modes does, an uploaded spectrum does not care
    base = engine.fit_peaks(phi, _df(256))
    engine.set_segments(Segments(64, 32))
    try:
        with pytest.raises(_hip.PsaHipError, match="segment"):
            calc.calculate_mode_peaks(*args)
        assert _bits(*_arrays(engine.fit_peaks(phi, _df(256)))) == _bits(*_arrays(base))
    finally:
        engine.set_segments(None)
    assert _bits(*_arrays(calc.calculate_mode_peaks(*args))) == _bits(*_arrays(plain))


def test_abi_errors(engine, syn):
    from psa_amd import Segments, _hip
    F, ncol = 256, 15
    df = _df(F)
    phi = F64.clean_case(F, ncol)[0]
    top = (F + 1) // 2
    good = dict(lo=1, hi=top)

    def refused(what, needle, *a, **kw):
        rc, msg, _, _ = _raw(engine, *a, **kw)
        assert rc == -1 and needle in msg, (what, rc, msg)

    refused("spec null", b"spec_host", None, df, F=F, ncol=ncol, **good)
    refused("fit null", b"fit", phi, df, fit=None, **good)
    refused("info null", b"info", phi, df, info=None, **good)
    refused("F < 12", b"F = 11", phi[:11], df, lo=1, hi=6)
    refused("C < 1", b"C = 0", phi, df, ncol=0, **good)
    refused("lo >= hi", b"lo = 9", phi, df, lo=9, hi=9)
    refused("lo = 0", b"lo = 0", phi, df, lo=0, hi=top)
    refused("hi beyond the positive half", b"hi = %d" % (top + 1), phi, df, lo=1, hi=top + 1)
    bands = np.tile(np.array([[1, top]], np.int32), (ncol, 1))
    for what, row in (("bands: lo >= hi", (20, 20)), ("bands: DC", (0, 50)), ("bands: past Nyquist", (5, top + 1))):
        b = bands.copy()
        b[11] = row
        refused(what, b"bands[11]", phi, df, bands=b)
    refused("window_hwhm <= 0", b"window_hwhm", phi, df, opts=(0.0, 0, 50), **good)
    refused("half_window_bins < 0", b"half_window_bins", phi, df, opts=(8.0, -1, 50), **good)
    refused("max_iter < 1", b"max_iter", phi, df, opts=(8.0, 0, 0), **good)
    refused("df", b"df", phi, 0.0, **good)
    rc, msg, fit, info = _raw(engine, phi, df, **good)                          # the context is usable afterwards
    ref, ref_info = F64.fit(phi, df)
    assert rc == 0, msg
    _hold("after the refusals", fit, info, ref, ref_info)

    # the mode entry: its own refusals and those of psa_sed_modes, NULL spectra allowed only here
    s = syn[256]
    tr = s["traj"]
    T, K, M = tr.n_frames, len(s["vecs"]), s["eig"].shape[1]
    engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
    lib, h = engine._lib, engine._h
    mean = np.ascontiguousarray(np.mean(tr.positions, axis=0, dtype=np.float32))
    kv = np.ascontiguousarray(s["vecs"], np.float32)
    idx, off, B = _hip.pack_groups(s["groups"])
    eig = np.ascontiguousarray(s["eig"], np.complex64)

    def modes_fit(fit="alloc", info="alloc", out=None, nbytes=None, lo=1, hi=(T + 1) // 2, opts=(8.0, 0, 50), eig=eig):
        fit = np.zeros((K * M, 6), np.float32) if isinstance(fit, str) else fit
        info = np.zeros((K * M, 4), np.int32) if isinstance(info, str) else info
        o = _hip.PeakOpts(*opts)
        rc = lib.psa_sed_modes_fit(h, _hip.SLOT_VELOCITIES, mean.ctypes.data_as(_hip._f32p), kv.ctypes.data_as(_hip._f32p), K,
                                   idx.ctypes.data_as(_hip._i32p), off.ctypes.data_as(_hip._i64p), B,
                                   None if eig is None else eig.ctypes.data_as(C.c_void_p), M, 0, 1.0 / (T * DT), None, lo, hi,
                                   C.byref(o), None if fit is None else fit.ctypes.data_as(_hip._f32p),
                                   None if info is None else info.ctypes.data_as(_hip._i32p),
                                   None if out is None else out.ctypes.data_as(_hip._f32p),
                                   C.c_size_t((0 if out is None else out.nbytes) if nbytes is None else nbytes))
        return rc, lib.psa_last_error(), fit, info

    def modes_refused(what, needle, **kw):
        rc, msg, _, _ = modes_fit(**kw)
        assert rc == -1 and needle in msg, (what, rc, msg)

    modes_refused("fit null", b"fit", fit=None)
    modes_refused("info null", b"info", info=None)
    modes_refused("eig null", b"eig", eig=None)
    modes_refused("lo >= hi", b"lo = 7", lo=7, hi=7)
    modes_refused("hi past the positive half", b"hi = ", hi=(T + 1) // 2 + 1)
    modes_refused("max_iter", b"max_iter", opts=(8.0, 0, 0))
    modes_refused("window_hwhm", b"window_hwhm", opts=(-1.0, 0, 50))
    modes_refused("out_bytes not exact", b"out_bytes", out=np.zeros((T, K, M), np.float32), nbytes=4 * T * K * M - 4)
    engine.set_segments(Segments(64, 32))
    try:
        modes_refused("segments set", b"segment")
    finally:
        engine.set_segments(None)
    rc, msg = lib.psa_sed_modes(h, _hip.SLOT_VELOCITIES, mean.ctypes.data_as(_hip._f32p), kv.ctypes.data_as(_hip._f32p), K,
                                idx.ctypes.data_as(_hip._i32p), off.ctypes.data_as(_hip._i64p), B, eig.ctypes.data_as(C.c_void_p), M, 0,
                                None, C.c_size_t(4 * T * K * M)), lib.psa_last_error()
    assert rc == -1 and b"null output" in msg                                   # psa_sed_modes still wants its output
    out = np.zeros((T, K, M), np.float32)
    rc, msg, fit_a, info_a = modes_fit()                                        # without the spectra
    assert rc == 0, msg
    rc, msg, fit_b, info_b = modes_fit(out=out)                                 # with them
    assert rc == 0 and _bits(fit_a, info_a) == _bits(fit_b, info_b)
    assert _bits(out) == _bits(s["calc"].calculate_mode_sed(s["mags"], s["vecs"], s["eig"], s["groups"]).sed)
