"""Welch-averaged mode spectra on the GPU (psa_sed_modes_welch, `calculate_mode_sed(segments=...)`,
`calculate_mode_peaks(segments=...)`): the contraction kernel alone against its derived per-element bound
(tests/modes_welch64.py), in one launch and with the segments split over launches; end to end against the float64
restatement; the identities that tie it to the mode-projected SED and to the segment-averaged `calculate`; blocking,
determinism and the budget; the low-rank k-path route; the fits; isolation from the SED entry points; ABI errors.
Every test prints its figures.

Measured on one MI355X: kernel alone 3.8 .. 7.6 u per element against bounds of 25 .. 495 u, the split runs bit-identical
to the single launch; end to end rel_max 8.1e-8 .. 4.3e-7 over the ten cases, per element (reported only) 2.3 .. 19.7 u of
A2_tot; identities <= 2.0e-7, one boxcar segment bit-identical to psa_sed_modes; the three blockings 1.4e-7 to float64 and
bit-identical to each other; low-rank route 8 launches, 1.6e-7; the planted AR(1) mode: |df0| / hwhm 2.7e-7,
|dhwhm| / hwhm 1.2e-7, |dheight| / height 1.3e-8, |dbaseline| / height 4.1e-9 against the float64 fit."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu

B_SITES = 8
MASSES = {1: 1.0, 2: 207.0}


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


def _eig(K, M, seed=5):
    import modes64 as M64
    return M64.random_unitary(np.random.default_rng(seed), K, B_SITES, M)


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


_Q64 = {}


def _reference(syn, T, klist, weighted, disp, seg, eig):
    """(Phi, A2_tot) float64; the float64 projections of the 8 sites are computed once per configuration"""
    import modes_welch64 as W64
    from ref64 import project64
    key = (T, klist, weighted, disp)
    if key not in _Q64:
        s = syn[T]
        tr = s["traj"]
        _Q64[key] = np.stack([project64(tr.positions if disp else tr.velocities, s["mean"], s["klists"][klist][1], g,
                                        s["weights"] if weighted else None, disp) for g in s["groups"]])
    w, U = W64.window64(seg)
    S = W64.segments64(_Q64[key], w, seg.length, seg.hop)
    return W64.contract_welch64(S, eig, 1.0 / (S.shape[3] * U))


# ------------------------------------------------------------------------------------------------- 1. the kernel alone
def test_kernel_against_the_derived_bound(engine):
    """psa_debug_mode_power_welch on uploaded complex64 segments: |Phi_gpu - Phi_64| <= (12 B + 11 + 2 n_seg) u A2_tot per
    element (derived in tests/modes_welch64.py; the proof that this can fail is tests/test_modes_welch_host.py), in one
    launch and with the segments split over launches that accumulate"""
    import modes_welch64 as W64
    for B, M, L, K, ns in W64.CASES:
        S, eig = W64.kernel_case(B, M, L, K, ns)
        scale = W64.kernel_scale(ns)
        ref, a2 = W64.contract_welch64(S, eig, float(scale))
        one = engine.debug_mode_power_welch(S, eig, scale)
        split = engine.debug_mode_power_welch(S, eig, scale, seg_block=1 if ns <= 3 else 2)
        assert one.shape == split.shape == (L, K, M) and one.dtype == np.float32
        e1, e2 = W64.per_element(one, ref, a2), W64.per_element(split, ref, a2)
        print(f"B={B} M={M} L={L} K={K} ns={ns}: one launch {e1 / W64.U:.1f} u, split {e2 / W64.U:.1f} u per element, bound "
              f"{W64.bound(B, ns) / W64.U:.0f} u, rel_max {rel_max(one, ref):.2e}; split run bit-identical: {_bits(one) == _bits(split)}")
        assert e1 <= W64.bound(B, ns)
        assert e2 <= W64.bound(B, ns)


@pytest.mark.parametrize("M", [5, 16, 24, 32, 40])
def test_one_segment_is_the_plain_contraction(engine, M):
    """The two debug entries share one body and the two instantiations of a tile one result: psa_debug_mode_power is
    bit-equal to psa_debug_mode_power_welch on the same spectra as one segment, and to the segment given twice at scale
    0.5 (x 0.5 + x 0.5 is exact), summed in one launch or over two.  B = 2; K = 5: a full tile of 4 k-vectors and a tail of
    one wavefront; T = 100: a partial tile of 64 frequencies; M picks the tiles 8 (padded), 16, 24, 32, and 8 with five passes"""
    import modes_welch64 as W64
    S = W64.kernel_case(2, 6, 100, 5, 1)[0]                                  # (B, K, 3, 1, T)
    rng = np.random.default_rng(M)
    eig = (rng.standard_normal((5, M, 2, 3)) + 1j * rng.standard_normal((5, M, 2, 3))).astype(np.complex64)
    plain = engine.debug_mode_power(S[:, :, :, 0, :], eig)
    assert plain.shape == (100, 5, M) and np.all(plain > 0)
    assert _bits(engine.debug_mode_power_welch(S, eig, 1.0)) == _bits(plain)
    twice = np.repeat(S, 2, axis=3)
    assert _bits(engine.debug_mode_power_welch(twice, eig, 0.5)) == _bits(plain)
    assert _bits(engine.debug_mode_power_welch(twice, eig, 0.5, seg_block=1)) == _bits(plain)


# ------------------------------------------------------------------------------------------------- 2. end to end
# every segment shape with every value of every other factor: two complementary cases per shape (L = 256 needs T = 256)
E2E = [
    # T, (L, H), window, klist, M, weighted, disp
    (256, (64, 32), "hann", "path", 24, False, False),
    (100, (64, 32), "boxcar", "scattered", 5, True, True),
    (100, (100, 30), "hann", "path", 5, False, True),
    (256, (100, 30), "boxcar", "scattered", 24, True, False),
    (256, (64, 64), "boxcar", "path", 5, True, False),
    (100, (64, 64), "hann", "scattered", 24, False, True),
    (100, (48, 80), "boxcar", "path", 24, True, True),
    (256, (48, 80), "hann", "scattered", 5, False, False),
    (256, (256, 256), "hann", "path", 24, True, True),
    (256, (256, 256), "boxcar", "scattered", 5, False, False),
]


@pytest.mark.parametrize("T,shape,window,klist,M,weighted,disp", E2E,
                         ids=[f"T{c[0]}_L{c[1][0]}_H{c[1][1]}_{c[2]}_{c[3]}_M{c[4]}_{'mass' if c[5] else 'plain'}_"
                              f"{'disp' if c[6] else 'vel'}" for c in E2E])
def test_parity_float64(engine, syn, T, shape, window, klist, M, weighted, disp):
    import modes_welch64 as W64
    from psa_amd import Segments
    s = syn[T]
    mags, vecs = s["klists"][klist]
    seg = Segments(shape[0], shape[1], window)
    eig = _eig(len(vecs), M)
    got = s["calcs"][disp].calculate_mode_sed(mags, vecs, eig, s["groups"], atom_weights=s["weights"] if weighted else None,
                                              segments=seg)
    ref, a2 = _reference(syn, T, klist, weighted, disp, seg, eig)
    L = seg.length
    assert got.sed.shape == (L, len(vecs), M) and got.sed.dtype == np.float32 and len(got.groups) == B_SITES
    assert np.array_equal(got.freqs, np.fft.fftfreq(L, d=s["calcs"][disp].dt_ps))
    err = rel_max(got.sed, ref)
    print(f"T={T} L={L} H={seg.hop} {window} ({seg.count(T)} segments) {klist} M={M} mass={weighted} disp={disp}: rel_max {err:.3e}; "
          f"per element (reported) {W64.per_element(got.sed, ref, a2) / W64.U:.1f} u of A2_tot")
    assert err <= 1e-5
    assert engine.segment_length == 0


def test_segment_factors_are_covered():
    shapes = {c[1] for c in E2E}
    assert shapes == {(64, 32), (100, 30), (64, 64), (48, 80), (256, 256)}
    for shape in shapes:
        mine = [c for c in E2E if c[1] == shape]
        assert all(c[1][0] <= c[0] for c in mine)
        for col, values in ((2, ("hann", "boxcar")), (3, ("path", "scattered")), (4, (24, 5)), (5, (False, True)), (6, (False, True))):
            assert {c[col] for c in mine} == set(values), (shape, col)
        assert {c[0] for c in mine} == ({256} if shape[0] > 100 else {256, 100})


# ------------------------------------------------------------------------------------------------- 3. identities
def test_one_boxcar_segment_is_the_mode_sed(engine, syn):
    from psa_amd import Segments, _hip
    for T in (256, 100):
        s = syn[T]
        calc, (mags, vecs), groups, tr = s["calcs"][False], s["klists"]["path"], s["groups"], s["traj"]
        eig = _eig(len(vecs), 24)
        plain = calc.calculate_mode_sed(mags, vecs, eig, groups).sed
        seg = calc.calculate_mode_sed(mags, vecs, eig, groups, segments=Segments(T, T, "boxcar")).sed
        err = rel_max(seg, plain)
        print(f"T={T}: Segments(T, T, boxcar) against no segments: rel_max {err:.3e} (bit-identical: {_bits(seg) == _bits(plain)})")
        assert seg.shape == plain.shape and err <= 1e-5
        # the entry itself with no segments set: one boxcar segment of T frames
        engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
        assert engine.segment_length == 0
        none_set = engine.sed_modes_welch(_hip.SLOT_VELOCITIES, s["mean"], vecs, groups, eig)
        old = engine.sed_modes(_hip.SLOT_VELOCITIES, s["mean"], vecs, groups, eig)
        err = rel_max(none_set, old)
        print(f"T={T}: psa_sed_modes_welch with no segments set against psa_sed_modes: rel_max {err:.3e} "
              f"(bit-identical: {_bits(none_set) == _bits(old)})")
        assert none_set.shape == (T, len(vecs), 24) and _bits(none_set) == _bits(old)      # the same code


def test_cartesian_vectors_are_the_segment_averaged_group_spectra(engine, syn):
    from psa_amd import Segments
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["path"], s["groups"]
    K = len(vecs)
    eig = np.zeros((K, 3 * B_SITES, B_SITES, 3), np.complex64)
    for b in range(B_SITES):
        for c in range(3):
            eig[:, 3 * b + c, b, c] = 1.0
    seg = Segments(100, 30, "hann")
    phi = calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg).sed
    for b in range(B_SITES):
        one = calc.calculate(mags, vecs, basis_atom_indices=groups[b].tolist(), segments=seg).sed
        err = rel_max(np.sum(phi[:, :, 3 * b:3 * b + 3].astype(np.float64), axis=-1), one)
        print(f"Cartesian vectors, site {b}: rel_max {err:.3e}")
        assert one.shape == (100, K) and err <= 1e-5


def test_homogeneity_and_planted_mode(engine, syn):
    from psa_amd import Segments, synth
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["scattered"], s["groups"]
    seg = Segments(64, 32, "hann")
    eig = _eig(len(vecs), 24)
    base = calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg).sed
    doubled = calc.calculate_mode_sed(mags, vecs, np.complex64(2) * eig, groups, segments=seg).sed
    assert np.isfinite(base).all() and base.max() < 1e30
    assert _bits(doubled) == _bits(np.float32(4) * base)
    # the x-polarised planted wave (bin 16 of 256 frames, k* = 0.25 * 2 pi / a along x) answers to the vector x / sqrt(B)
    T = 256
    vecs = np.float32([[0.1, 0.2, 0.0], [2 * np.pi / synth.A_SI * 0.25, 0, 0], [0.9, 0.0, 0.3]])
    n = 3 * B_SITES
    rng = np.random.default_rng(12)
    eig = np.empty((3, n, B_SITES, 3), np.complex64)
    for k in range(3):
        m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        m[:, 0] = 0.0
        m[0::3, 0] = 1.0
        eig[k] = np.linalg.qr(m)[0].T.reshape(n, B_SITES, 3)
    phi = calc.calculate_mode_sed(np.linalg.norm(vecs, axis=1), vecs, eig, groups, segments=Segments(T, T, "hann")).sed
    w_star = int(np.argmax(phi[:, 1, 0]))
    assert w_star in (16, T - 16)
    assert int(np.argmax(phi[w_star, 1, :])) == 0


# ------------------------------------------------------------------------------------------------- 4. blocking
def test_blocking_determinism_and_budget(engine, syn):
    from psa_amd import Segments, _hip
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["path"], s["groups"]
    seg = Segments(64, 32, "hann")                               # 7 segments
    eig = _eig(len(vecs), 24)
    ref = _reference(syn, 256, "path", False, False, seg, eig)[0]
    per_k, unit = 24 * B_SITES * 256, 24 * B_SITES * 64          # bytes of one k-vector of q, of one (k-vector, segment) unit
    got = {}
    try:
        # the whole list with all segments; 15 + 9 k-vectors, 12 of them x one segment per launch; one k-vector, 2 segments
        for name, budget in (("one block", 4 << 30), ("two k-blocks", 18 * per_k), ("bs = 2 < n_seg", per_k + 2 * unit)):
            engine.set_option(_hip.OPT_MODES_WORK_BYTES, budget)
            a = calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg).sed
            b = calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg).sed
            assert _bits(a) == _bits(b)                                           # two identical calls
            got[name] = (a.copy(), rel_max(a, ref))
            print(f"{name} ({budget} bytes): rel_max to float64 {got[name][1]:.3e}")
            assert got[name][1] <= 1e-5
        names = list(got)
        for i, x in enumerate(names):
            for y in names[i + 1:]:
                print(f"{x} vs {y}: bit-identical: {_bits(got[x][0]) == _bits(got[y][0])}")
        engine.set_option(_hip.OPT_MODES_WORK_BYTES, per_k + unit - 1)
        with pytest.raises(_hip.PsaHipError, match=str(per_k + unit)):
            calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg)
        assert engine.segment_length == 0
    finally:
        reset(engine)
    assert _bits(calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg).sed) == _bits(got["one block"][0])


def test_lowrank_route_on_a_k_path(engine, syn):
    """256 k-vectors on [100] with segments set: the low-rank route serves all 8 site groups (one launch count each, as
    tests/test_gpu_modes.py checks it), the result meets float64"""
    import modes_welch64 as W64
    from psa_amd import Segments, _hip
    s = syn[256]
    calc, groups, tr = s["calcs"][False], s["groups"], s["traj"]
    mags, vecs = calc.get_k_path("100", 1.0, 256)
    assert all(_hip.lowrank_plan(vecs, s["mean"], g) is not None for g in groups)
    eig = _eig(256, 24, seed=6)
    seg = Segments(64, 32, "hann")
    try:
        engine.set_option(_hip.OPT_PLANES_EAGER, 1)
        n0 = engine.lowrank_launches()
        low = calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg).sed
        taken = engine.lowrank_launches() - n0
        err = rel_max(low, W64.mode_welch64(tr.velocities, s["mean"], vecs, groups, eig, seg)[0])
        print(f"low-rank route with segments: {taken} launches, rel_max to float64 {err:.3e}")
        assert taken == B_SITES
        assert err <= 1e-5
    finally:
        reset(engine)


# ------------------------------------------------------------------------------------------------- 5. fits
def _arrays(pf):
    fit = np.stack([np.ravel(x) for x in (pf.frequency, pf.hwhm, pf.height, pf.baseline, pf.rss, pf.peak_bin.astype(np.float32))], axis=1)
    w = pf.window.reshape(-1, 2)
    return fit, np.stack([np.ravel(pf.status), np.ravel(pf.iterations), w[:, 0], w[:, 1] - w[:, 0]], axis=1)


def test_peaks_of_segment_averaged_spectra(engine, syn):
    from psa_amd import Segments
    s = syn[256]
    calc, (mags, vecs), groups = s["calcs"][False], s["klists"]["path"], s["groups"]
    eig = _eig(len(vecs), 5)
    seg = Segments(64, 32, "hann")
    df = 1.0 / (64 * calc.dt_ps)
    sed = calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg).sed
    apart = engine.fit_peaks(sed, df)
    fused = calc.calculate_mode_peaks(mags, vecs, eig, groups, segments=seg)
    both, spectra = calc.calculate_mode_peaks(mags, vecs, eig, groups, segments=seg, return_sed=True)
    assert fused.frequency.shape == (len(vecs), 5)
    assert _bits(*_arrays(fused)) == _bits(*_arrays(apart)) == _bits(*_arrays(both))
    assert spectra.sed.shape == (64, len(vecs), 5) and _bits(spectra.sed) == _bits(sed)
    assert np.array_equal(spectra.freqs, np.fft.fftfreq(64, d=calc.dt_ps))
    assert engine.segment_length == 0


def test_planted_lorentzian_mode(engine):
    """the planted AR(1) mode of tests/test_modes_welch_host.py (T = 4096, Segments(512, 256, "hann")): the GPU fit of the
    planted column against the float64 fit of the float64 restatement"""
    import fit64
    import modes_welch64 as W64
    from psa_amd import SEDCalculator, Segments, Trajectory
    p = W64.planted_ar1(0)
    T = W64.PLANTED_T
    tr = Trajectory(p["positions"], p["velocities"], p["types"], np.arange(T, dtype=np.float32), p["box"], np.diag(p["box"]).copy(),
                    np.zeros(3, np.float32), W64.PLANTED_DT)
    calc = SEDCalculator(tr, *p["cells"]).attach(engine=engine)
    try:
        pf = calc.calculate_mode_peaks(np.linalg.norm(p["k"], axis=1), p["k"], p["eig"], p["groups"],
                                       segments=Segments(W64.PLANTED_L, W64.PLANTED_H, "hann"))
    finally:
        engine.invalidate()
    ref, ref_info, _ = W64.planted_fit64(0)
    got, info = _arrays(pf)
    f0, hw = W64.planted_truth()
    m = fit64.compare(got[:1], ref[None])
    print(f"planted AR(1) mode: status {info[0, 0]}, peak bin {got[0, 5]:.0f}, window [{info[0, 2]}, +{info[0, 3]}); against the float64 "
          f"fit: |df0| / hwhm {m[0]:.2e}, |dhwhm| / hwhm {m[1]:.2e}, |dheight| / height {m[2]:.2e}, |dbaseline| / height {m[3]:.2e}; "
          f"against the planted values: f0 off by {(got[0, 0] - f0) / hw:+.3f} half widths, hwhm {got[0, 1] / hw:.3f} of the planted")
    assert info[0, 0] == 0
    assert got[0, 5] == ref[5] and np.array_equal(info[0, 2:], ref_info[2:])
    assert max(m) <= 1e-2


# ------------------------------------------------------------------------------------------------- 6. isolation, errors
def test_no_leak_into_sed_calls(engine, syn):
    from psa_amd import Segments, _hip
    s = syn[256]
    calc, (mags, vecs), groups, tr = s["calcs"][False], s["klists"]["path"], s["groups"], s["traj"]
    eig = _eig(len(vecs), 5)
    seg = Segments(64, 32, "hann")
    # resident first: the test before this one invalidated the slots, and a `calculate` that uploads projects while it
    # streams, with other kernels (and other last bits) than one that finds its array in HBM
    engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
    for kw in ({}, dict(basis_atom_types=[1, 2], summation_mode="incoherent"), dict(segments=Segments(100, 30))):
        before = calc.calculate(mags, vecs, **kw)
        calc.calculate_mode_sed(mags, vecs, eig, groups, atom_weights=s["weights"], segments=seg)
        calc.calculate_mode_peaks(mags, vecs, eig, groups, segments=seg)
        after = calc.calculate(mags, vecs, **kw)
        assert after.sed.shape == before.sed.shape and after.sed.dtype == before.sed.dtype
        assert _bits(after.sed) == _bits(before.sed)
    # a projection that has not been finalized yet survives a segment-averaged mode call
    engine.project(_hip.SLOT_VELOCITIES, s["mean"], vecs, None, 0)
    whole = np.array(engine.finalize(tr.n_frames, len(vecs), False))
    engine.project(_hip.SLOT_VELOCITIES, s["mean"], vecs, None, 0)
    calc.calculate_mode_sed(mags, vecs, eig, groups, segments=seg)
    later = engine.finalize(tr.n_frames, len(vecs), False)
    assert _bits(np.asarray(later)) == _bits(whole)
    assert engine.segment_length == 0
    # weights and segments of the call are gone: the plain mode spectra are what they were
    plain = calc.calculate_mode_sed(mags, vecs, eig, groups).sed.copy()
    calc.calculate_mode_sed(mags, vecs, eig, groups, atom_weights=s["weights"], segments=seg)
    again = calc.calculate_mode_sed(mags, vecs, eig, groups).sed
    assert again.shape == (256, len(vecs), 5) and _bits(again) == _bits(plain)


def test_abi_errors(engine, syn):
    import modes_welch64 as W64
    from psa_amd import Segments, _hip
    s = syn[256]
    tr, (mags, vecs) = s["traj"], s["klists"]["scattered"]
    T, N, K, M = tr.n_frames, tr.n_atoms, len(vecs), 4
    engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
    lib, h = engine._lib, engine._h
    mean = np.ascontiguousarray(s["mean"], np.float32)
    kv = np.ascontiguousarray(vecs, np.float32)
    import modes64 as M64
    good_eig = M64.random_unitary(np.random.default_rng(1), K, 2, M)
    two = ([0, 1, 2, 3], [0, 2, 4])
    seg = Segments(64, 32, "hann")
    L = seg.length

    def call(idx=two[0], off=two[1], B=2, eig=good_eig, M=M, nbytes=None, out="alloc", flags=0, fit=False):
        o = np.zeros((L, K, max(M, 1)), np.float32) if isinstance(out, str) else out
        ip = None if idx is None else np.ascontiguousarray(idx, np.int32)
        op = None if off is None else np.ascontiguousarray(off, np.int64)
        head = (h, _hip.SLOT_VELOCITIES, mean.ctypes.data_as(_hip._f32p), kv.ctypes.data_as(_hip._f32p), K,
                None if ip is None else ip.ctypes.data_as(_hip._i32p), None if op is None else op.ctypes.data_as(_hip._i64p), B,
                None if eig is None else eig.ctypes.data_as(C.c_void_p), M, flags)
        tail = (None if o is None else o.ctypes.data_as(_hip._f32p), C.c_size_t((0 if o is None else o.nbytes) if nbytes is None else nbytes))
        if not fit:
            return lib.psa_sed_modes_welch(*head, *tail), lib.psa_last_error()
        f, i = np.zeros((K * max(M, 1), 6), np.float32), np.zeros((K * max(M, 1), 4), np.int32)
        opts = _hip.PeakOpts(8.0, 0, 50)
        rc = lib.psa_sed_modes_welch_fit(*head, 1.0 / (L * 0.002), None, 1, (L + 1) // 2, C.byref(opts), f.ctypes.data_as(_hip._f32p),
                                         i.ctypes.data_as(_hip._i32p), *tail)
        return rc, lib.psa_last_error()

    def refused(what, needle=b"", **kw):
        for fit in (False, True):
            rc, msg = call(fit=fit, **kw)
            assert rc == -1 and len(msg) > 0 and needle in msg, (what, fit, rc, msg)

    engine.set_segments(seg)
    try:
        refused("eig null", b"eig", eig=None)
        rc, msg = call(out=None, nbytes=4 * L * K * M)
        assert rc == -1 and b"null output" in msg                               # (the fit entry may go without the spectra)
        assert call(out=None, nbytes=0, fit=True)[0] == 0
        rc, msg = call(M=0)
        assert rc == -1 and len(msg) > 0
        refused("flags", b"PSA_F_DISPLACEMENTS", flags=_hip.F_INTENSITY)
        bad = good_eig.copy()
        bad[2, 1, 1, 0] = np.inf
        refused("non-finite eig", b"finite", eig=bad)
        refused("an atom in two groups", b"disjoint", idx=[0, 1, 1, 2])
        refused("index out of range", idx=[0, 1, 2, N])
        refused("negative index", idx=[0, -1, 2, 3])
        refused("out_bytes not exact", b"out_bytes", nbytes=4 * L * K * M - 4)
        refused("the size of the unsegmented result", b"out_bytes", out=np.zeros((T, K, M), np.float32))
        refused("NULL list means one group", idx=None, off=None)
        engine.set_atom_weights(np.ones(N + 1, np.float32))
        try:
            refused("weights of another length", b"weights")
        finally:
            engine.set_atom_weights(None)
        engine.set_option(_hip.OPT_MODES_WORK_BYTES, 24 * 2 * (T + L) - 1)
        try:
            refused("budget below one k-vector and one unit", str(24 * 2 * (T + L)).encode())
        finally:
            engine.set_option(_hip.OPT_MODES_WORK_BYTES, 4 << 30)
        engine.set_segments(Segments(T, T))
        engine.ensure_resident(_hip.SLOT_VELOCITIES, syn[100]["traj"].velocities)   # 100 frames under segments of 256
        refused("L > T", b"exceeds", out=np.zeros((T, K, M), np.float32))
        engine.set_segments(seg)
        engine.ensure_resident(_hip.SLOT_VELOCITIES, tr.velocities)
        # the entries without the segment average still refuse
        o = np.zeros((T, K, M), np.float32)
        ip, op = np.ascontiguousarray(two[0], np.int32), np.ascontiguousarray(two[1], np.int64)
        rc = lib.psa_sed_modes(h, _hip.SLOT_VELOCITIES, mean.ctypes.data_as(_hip._f32p), kv.ctypes.data_as(_hip._f32p), K,
                               ip.ctypes.data_as(_hip._i32p), op.ctypes.data_as(_hip._i64p), 2, good_eig.ctypes.data_as(C.c_void_p), M, 0,
                               o.ctypes.data_as(_hip._f32p), C.c_size_t(o.nbytes))
        assert rc == -1 and b"segment" in lib.psa_last_error()
        # the context is usable afterwards
        out = np.zeros((L, K, M), np.float32)
        rc, msg = call(out=out)
        assert rc == 0, msg
        groups = [np.array([0, 1]), np.array([2, 3])]
        assert rel_max(out, W64.mode_welch64(tr.velocities, s["mean"], vecs, groups, good_eig, seg)[0]) <= 1e-5
    finally:
        reset(engine)
    # the debug entry's own argument check
    S, e = W64.kernel_case(1, 3, 16, 3, 1)
    o = np.zeros((16, 3, 3), np.float32)
    rc = lib.psa_debug_mode_power_welch(h, S.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), 1, 3, 3, 16, 0, 0, 1.0,
                                        o.ctypes.data_as(_hip._f32p))
    assert rc == -1 and b"bad argument" in lib.psa_last_error()
