"""The partial (species-resolved) spectra on the GPU (psa_partial_spectra, `calculate_partial_spectra`,
`calculate_powder_partial_spectra`): the projections of every species bit for bit those of psa_debug_lattice_project on
that species' list; the pair passes element by element inside the bars of tests/partial_cases.py in both forms and for
every cutting, with the exact items bit for bit; the two calculator methods against the float64 restatement
(tests/partial64.py) on the explicit full sphere, on a travelling wave in which one species lags behind another; the sum
rule through the public API; every refusal; no trace in a later calculation."""
import ctypes as Ct

import numpy as np
import pytest

import lattice64 as L64
import lattice_cases as LC
import partial64 as R
import partial_cases as C
import power64
import power_cases as P
from engine_state import reset

pytestmark = pytest.mark.gpu

BOXES = {"cubic": LC.CUBIC, "triclinic": LC.TRICLINIC}
FIELDS = ("density", "longitudinal", "transverse")


@pytest.fixture(autouse=True)
def _clean(engine):
    reset(engine)
    yield
    reset(engine)


@pytest.fixture(scope="module", autouse=True)
def _forget(engine):
    yield
    engine.invalidate()


def _resident(engine, pos, vel):
    from psa_amd import _hip
    engine.ensure_resident(_hip.SLOT_POSITIONS, pos)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, vel)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the projections ----------------------------------------------------------------------------------------------------
# (species sizes, K, frames, currents, box, weights, shuffled lists); LAT_CHAIN = 128, LAT_KS = 512, LAT_FRAMES = 4
PROJECT_CASES = [
    ((129,), 1, 1, True, "cubic", "unit", False),
    ((1, 127), 2, 3, False, "triclinic", "signed", True),
    ((128, 0, 129), 511, 4, True, "cubic", "sqrt_mass", True),
    ((1, 127, 128, 129, 0, 5, 64, 3), 512, 5, False, "triclinic", "signed", True),
    ((129, 128), 513, 3, True, "triclinic", "signed", True),
    ((0, 7, 0), 2, 4, True, "cubic", "unit", True),
]


@pytest.mark.parametrize("case", PROJECT_CASES, ids=[f"S{len(c[0])}_K{c[1]}_T{c[2]}_{'j' if c[3] else 'rho'}_{c[4]}" for c in PROJECT_CASES])
def test_projection_is_the_lattice_kernels_bit_for_bit(engine, case):
    from psa_amd import _hip, commensurate_vectors
    sizes, K, T, currents, box_name, wk, shuffled = case
    box = BOXES[box_name]
    inv = LC.inverse(box)
    ind = LC.mixed_indices(K, seed=K) if K <= 2 else commensurate_vectors(box, 2.6)[0][:K]
    assert ind.shape == (K, 3)
    n_all = sum(sizes) + 5
    pos, vel = LC.trajectory(n_all, T, seed=n_all + K, box=box)
    w = LC.weights(wk, n_all, seed=2)
    order = np.random.default_rng(3).permutation(n_all) if shuffled else np.arange(n_all)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    species = [order[cuts[i]:cuts[i + 1]].astype(np.int32) for i in range(len(sizes))]
    _resident(engine, pos, vel)
    engine.set_atom_weights(w)
    got = engine.debug_partial_project(inv, ind, species, currents)
    assert got.shape == (K, len(sizes), 4 if currents else 1, T)
    for a, g in enumerate(species):
        want = engine.debug_lattice_project(inv, ind, g, currents)
        assert np.array_equal(_bits(got[:, a]), _bits(want)), a
        if g.size == 0:
            assert not got[:, a].any()
    assert got.any()
    again = engine.debug_partial_project(inv, ind, species, currents)
    assert np.array_equal(_bits(got), _bits(again))
    if K >= 2:                                                             # cut into blocks of vectors: S NC series each
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, len(sizes) * (4 if currents else 1) * T * 8 * max(1, K // 3))
        assert np.array_equal(_bits(got), _bits(engine.debug_partial_project(inv, ind, species, currents)))


# ---- 2. the pair passes ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    return C.references()


def _power(engine, args, k_block, seg_block):
    seg, _, khat, norm, bin_of, n_bins = args
    return engine.debug_partial_power(seg, khat, norm, bin_of, n_bins, k_block, seg_block)


def _diagonal(S):
    return [C.n_pairs(S) - C.n_pairs(S - a) for a in range(S)]


CASE_IDS = [(kind, c["name"]) for kind, cases in (("vector", C.VECTOR_CASES), ("shell", C.SHELL_CASES)) for c in cases]


@pytest.mark.parametrize("kind,name", CASE_IDS, ids=[f"{k}_{n}" for k, n in CASE_IDS])
def test_pair_pass_within_the_bars_for_every_cutting(engine, refs, kind, name):
    c, args, ref, bars = refs[kind][name]
    K, ns = args[0].shape[0], c["ns"]
    cuttings = [(c["k_block"], c["seg_block"])]
    if "tail" not in name:
        cuttings += [x for x in ((0, 0), (1, 1), (2, ns), (K, 2)) if x not in cuttings]
    for kb, sb in cuttings:
        got = _power(engine, args, kb, sb)
        assert got.shape == ref["out"].shape and got.dtype == np.float32
        b = bars if (kind == "shell" or sb == c["seg_block"]) else C.vector_bars(ref, ns, sb)
        fr = C.worst(got, ref, b)
        print(f"{kind} {name} cut ({kb}, {sb}): " + ", ".join(f"{C.ROWS[r]} {f:.3f} of its bar at {at}" for r, (f, at) in enumerate(fr)))
        assert max(f for f, _ in fr) <= 1.0, (kb, sb, fr)
        if got.shape[0] == 3:
            assert (got[2][_diagonal(c["S"])] >= 0).all()                  # transverse_aa: a sum of squares
    if c["relation"] == "i":
        assert not ref["out"][0][1].any()                                  # F^b = i F^a: the cross density is 0 in the reference


@pytest.mark.parametrize("L", C.EXACT_L)
def test_exact_items_bit_for_bit_for_every_cutting(engine, L):
    seg, k, norm = C.exact_vector(L)
    ref = R.vector64(seg, k, norm)["out"].astype(np.float32)
    for kb, sb in C.VECTOR_CUTS:
        got = engine.debug_partial_power(seg, P.khat32(k), norm, None, 0, kb, sb)
        assert np.array_equal(_bits(got), _bits(ref)), ("vector", kb, sb)
    seg, k, bin_of, n_bins, norm = C.exact_shell(L)
    ref = R.shell64(seg, k, bin_of, n_bins, norm)["out"].astype(np.float32)
    assert not ref[..., [0, 3, 5]].any() and ref[..., [1, 2, 4]].all()
    for kb, sb in C.SHELL_CUTS:
        got = engine.debug_partial_power(seg, P.khat32(k), norm, bin_of, n_bins, kb, sb)
        assert np.array_equal(_bits(got), _bits(ref)), ("shell", kb, sb)   # o = 0 and o = L / 2 are their own mirrors
    assert (ref[2][_diagonal(C.EXACT_S)] >= 0).all()


@pytest.mark.parametrize("cut", [(0, 0), (5, 2)])
def test_diagonal_pairs_agree_with_the_one_species_passes(engine, refs, cut):
    """pair (a, a) against psa_debug_dynamic_power / psa_debug_lattice_shell on species a's rows: within the sum of both bars"""
    kb, sb = cut
    c, args, ref, bars = refs["vector"]["S3_families"]
    seg, k, khat, norm, _, _ = args
    got = _power(engine, args, kb, sb)
    bars = C.vector_bars(ref, c["ns"], sb)
    for a, row in enumerate(_diagonal(c["S"])):
        one = np.ascontiguousarray(seg[:, a])
        scale = np.float32(1.0 / norm)
        other = engine.debug_dynamic_power(one, k, scale, kb, sb)
        allow = bars[:, row] + P.dynamic_bars(power64.dynamic64(one, k, scale), c["ns"], sb)
        assert np.all(np.abs(got[:, row].astype(np.float64) - other) <= allow), a
    c, args, ref, bars = refs["shell"]["S3_families"]
    seg, k, khat, norm, bin_of, n_bins = args
    got = _power(engine, args, kb, sb)
    for a, row in enumerate(_diagonal(c["S"])):
        one = np.ascontiguousarray(seg[:, a])
        other = engine.debug_lattice_shell(one, khat, bin_of, n_bins, norm, kb, sb)
        allow = bars[:, row] + P.shell_bars(power64.shell64(one, k, bin_of, n_bins, norm))
        assert np.all(np.abs(got[:, row].astype(np.float64) - other) <= allow), a


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------
def _calculator(engine, pos, vel, box, dt=0.002, cells=(1, 1, 1)):
    from psa_amd import SEDCalculator, Trajectory
    T, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, vel, np.ones(n, np.int32), np.arange(T, dtype=np.float32), box, np.diag(box).copy(),
                    np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, *cells).attach(engine=engine)


EDGES = np.array([0.05, 0.2, 0.45, 0.65, 0.85, 1.0, 1.15])                # the first shell lies below the shortest vector
SEGMENTS = {"none": None, "hann_64_32": (64, 32, "hann"), "boxcar_64_64": (64, 64, "boxcar")}


@pytest.fixture(scope="module", params=list(BOXES))
def wave(request):
    """T = 256, N = 130 split 64 / 65 / 1 (shuffled), the half-space of |k| < 1.15 in 6 shells of which the first is empty, a
    travelling wave on one of its vectors in which species 1 lags species 0 by 1.1 rad, sqrt-mass weights; the float64
    projections of the explicit full sphere, once for every segment shape"""
    from psa_amd import commensurate_vectors, shell_bins
    box = BOXES[request.param]
    inv = LC.inverse(box)
    half, _, q = commensurate_vectors(box, EDGES[-1], EDGES[0])
    b, sel, avail, used = shell_bins(q, EDGES)
    half, b, q = half[sel], b[sel], q[sel]
    assert 100 <= half.shape[0] <= 300 and avail[0] == 0 and np.all(avail[1:] > 0)
    order = np.random.default_rng(7).permutation(130)
    species = [order[:64].tolist(), order[64:129].tolist(), order[129:].tolist()]
    pos, vel = C.lagged_wave(130, 256, box, half[np.flatnonzero(b == 2)[3]], 20, species[1], 1.1)
    w = LC.weights("sqrt_mass", 130, seed=23)
    full, b_full = np.concatenate([half, -half]), np.concatenate([b, b])
    return dict(box=box, inv=inv, half=half, bins=b, avail=avail, pos=pos, vel=vel, w=w, full=full, b_full=b_full, species=species,
                q_full=R.project64(pos, vel, full, inv, species, w, True))


def _window(s):
    return (None, None, None) if s is None else (s.window_array(), s.length, s.hop)


def _pair_errors(got, ref):
    """per pair (a, b): max |got - ref| in units of sqrt(max X_aa max X_bb) of the reference; the largest"""
    pr = R.pairs(3)
    top = np.array([np.max(np.abs(ref[i])) for i in (0, 3, 5)])            # the diagonal rows of three species
    unit = np.sqrt(top[pr[:, 0]] * top[pr[:, 1]])
    assert (unit > 0).all()
    return float(np.max(np.max(np.abs(got.astype(np.float64) - ref), axis=(1, 2)) / unit))


@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_calculators_parity_float64_on_the_full_sphere(engine, wave, seg):
    from psa_amd import PartialSpectra, PowderPartialSpectra, Segments
    s = None if SEGMENTS[seg] is None else Segments(*SEGMENTS[seg])
    L = 256 if s is None else s.length
    sp = wave["species"]
    calc = _calculator(engine, wave["pos"], wave["vel"], wave["box"])
    per64 = R.spectra64(wave["q_full"], wave["full"], wave["inv"], *_window(s))
    per = calc.calculate_partial_spectra(wave["full"], sp, atom_weights=wave["w"], segments=s)
    assert isinstance(per, PartialSpectra) and per.density.shape == (6, L, wave["full"].shape[0]) and per.density.dtype == np.float32
    assert per.pairs.tolist() == R.pairs(3).tolist() and [g.tolist() for g in per.groups] == sp
    np.testing.assert_allclose(per.weight_norms, [np.sum(wave["w"][g].astype(np.float64) ** 2) for g in sp])
    np.testing.assert_allclose(per.k_vectors, L64.lattice_k(wave["full"], wave["inv"]), rtol=0, atol=1e-13)
    errs = {f"vector {n}": _pair_errors(getattr(per, n), ref) for n, ref in zip(FIELDS, per64)}
    assert (per.transverse[[0, 3, 5]] >= 0).all()
    lag = per64[0][1]                                                      # the cross term of the two large species is not their geometric mean
    assert np.max(np.abs(lag)) > 0 and np.min(lag) < 0
    pw = calc.calculate_powder_partial_spectra(EDGES, sp, atom_weights=wave["w"], segments=s)
    ref = R.shell_mean64(per64, wave["b_full"], 6)
    assert isinstance(pw, PowderPartialSpectra) and pw.density.shape == (6, L, 6) and pw.density.dtype == np.float32
    for n, want in zip(FIELDS, ref):
        errs[f"powder {n}"] = _pair_errors(getattr(pw, n), want)
    print(f"{seg}: {errs}")
    assert max(errs.values()) <= 1e-5
    for n in FIELDS:
        assert not getattr(pw, n)[:, :, 0].any()                           # the empty shell
    np.testing.assert_array_equal(pw.counts, 2 * np.bincount(wave["bins"], minlength=6))
    np.testing.assert_array_equal(pw.available, 2 * wave["avail"])
    assert np.array_equal(pw.indices, wave["half"]) and np.array_equal(pw.bin_index, wave["bins"]) and np.isnan(pw.q[0])
    np.testing.assert_allclose(pw.freqs, np.fft.fftfreq(L, 0.002))
    # the shell form against the per-vector form averaged on the host in float64
    host = R.shell_mean64([getattr(per, n).astype(np.float64) for n in FIELDS], wave["b_full"], 6)
    shell = {n: _pair_errors(getattr(pw, n), want) for n, want in zip(FIELDS, host)}
    print(f"{seg}: shell form against per-vector form: {shell}")
    assert max(shell.values()) <= 1e-6
    if s is None:                                                          # the density alone
        rho = calc.calculate_partial_spectra(wave["full"], sp, atom_weights=wave["w"], currents=False)
        assert rho.longitudinal is None and rho.transverse is None and _pair_errors(rho.density, per64[0]) <= 1e-5
        rho = calc.calculate_powder_partial_spectra(EDGES, sp, atom_weights=wave["w"], currents=False)
        assert rho.longitudinal is None and rho.transverse is None and _pair_errors(rho.density, ref[0]) <= 1e-5


def test_max_per_bin_blockings_repeat_empty_species(engine, wave):
    from psa_amd import Segments, _hip
    s = Segments(64, 32, "hann")
    sp = wave["species"]
    calc = _calculator(engine, wave["pos"], wave["vel"], wave["box"])
    pw = calc.calculate_powder_partial_spectra(EDGES, sp, atom_weights=wave["w"], segments=s, max_per_bin=9, seed=3)
    np.testing.assert_array_equal(pw.counts, 2 * np.minimum(wave["avail"], 9))
    full, b_full = np.concatenate([pw.indices, -pw.indices]), np.concatenate([pw.bin_index, pw.bin_index])
    q = R.project64(wave["pos"], wave["vel"], full, wave["inv"], sp, wave["w"], True)
    ref = R.shell_mean64(R.spectra64(q, full, wave["inv"], *_window(s)), b_full, 6)
    errs = {n: _pair_errors(getattr(pw, n), want) for n, want in zip(FIELDS, ref)}
    print(f"max_per_bin = 9: {errs}")
    assert max(errs.values()) <= 1e-5
    other = calc.calculate_powder_partial_spectra(EDGES, sp, atom_weights=wave["w"], segments=s, max_per_bin=9, seed=4)
    assert not np.array_equal(other.indices, pw.indices)
    # the engine: a repeat gives the same bits in both forms; the per-vector form cut into blocks of vectors too
    _resident(engine, wave["pos"], wave["vel"])
    engine.set_atom_weights(wave["w"])
    one = engine.partial_spectra(wave["inv"], wave["half"], sp, None, 0, True)
    assert np.array_equal(_bits(one), _bits(engine.partial_spectra(wave["inv"], wave["half"], sp, None, 0, True)))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 3 * 4 * 256 * 8 * 37)   # 37 vectors of q, transformed where they lie
    assert np.array_equal(_bits(one), _bits(engine.partial_spectra(wave["inv"], wave["half"], sp, None, 0, True)))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
    engine.set_segments(s)
    sh = engine.partial_spectra(wave["inv"], wave["half"], sp, wave["bins"], 6, True)
    assert np.array_equal(_bits(sh), _bits(engine.partial_spectra(wave["inv"], wave["half"], sp, wave["bins"], 6, True)))
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 3 * 4 * 8 * (37 * 256 + 50 * 64))   # 37 vectors of q, 50 (vector, segment) units
    cut = engine.partial_spectra(wave["inv"], wave["half"], sp, wave["bins"], 6, True)
    ulp = np.spacing(np.maximum(np.abs(sh), np.abs(cut)))
    assert np.all(np.abs(sh - cut) <= ulp)                                 # the order of the float64 sums alone
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
    # an empty species gives zeros in all of its pairs and leaves the others alone; all empty: zeros
    holed = engine.partial_spectra(wave["inv"], wave["half"], [sp[0], [], sp[2]], wave["bins"], 6, True)
    assert not holed[:, [1, 3, 4]].any() and np.array_equal(_bits(holed[:, [0, 2, 5]]), _bits(sh[:, [0, 2, 5]]))
    assert not engine.partial_spectra(wave["inv"], wave["half"], [[], []], None, 0, False).any()
    assert not engine.debug_partial_project(wave["inv"], wave["half"], [[], []], False).any()


# ---- 4. the sum rule through the public API ----------------------------------------------------------------------------------
def test_sum_rule_against_the_spectra_of_the_union(engine, wave):
    from psa_amd import Segments
    s = Segments(64, 32, "hann")
    sp = wave["species"]
    calc = _calculator(engine, wave["pos"], wave["vel"], wave["box"])
    per = calc.calculate_partial_spectra(wave["half"], sp, atom_weights=wave["w"], segments=s)
    pw = calc.calculate_powder_partial_spectra(EDGES, sp, atom_weights=wave["w"], segments=s)
    of = np.empty(130, int)
    for a, g in enumerate(sp):
        of[g] = a
    worst = 0.0
    for coef in (np.ones(3), np.array([1.0, -0.6, 2.5])):
        wu = (coef[of] * wave["w"]).astype(np.float32)
        union = (calc.calculate_lattice_spectra(wave["half"], atom_weights=wu, segments=s),
                 calc.calculate_powder_spectra(EDGES, atom_weights=wu, segments=s))
        for parts, whole in zip((per, pw), union):
            factor = np.abs(coef[parts.pairs[:, 0]] * coef[parts.pairs[:, 1]]) * np.where(parts.pairs[:, 0] == parts.pairs[:, 1], 1.0, 2.0)
            for n in FIELDS:
                size = np.max(np.tensordot(factor, np.abs(getattr(parts, n).astype(np.float64)), axes=(0, 0)))
                err = np.max(np.abs(parts.combine(coef, n) - getattr(whole, n).astype(np.float64))) / size
                worst = max(worst, err)
                assert err <= 2e-5, (coef, type(parts).__name__, n, err)
    print(f"sum rule: worst {worst:.2e} of max sum |c_a c_b X_ab|")


# ---- 5. refusals, and no trace -----------------------------------------------------------------------------------------------
def test_refusals(engine, wave):
    from psa_amd import Segments, _hip
    pos, vel, inv = wave["pos"], wave["vel"], np.ascontiguousarray(wave["inv"])
    _resident(engine, pos, vel)
    lib, h = engine._lib, engine._h
    f32p, i32p, i64p, f64p = Ct.POINTER(Ct.c_float), Ct.POINTER(Ct.c_int32), Ct.POINTER(Ct.c_int64), Ct.POINTER(Ct.c_double)
    ind = np.ascontiguousarray(wave["half"][:9])
    bins = np.ascontiguousarray(wave["bins"][:9])
    idx = np.arange(130, dtype=np.int32)
    off = np.array([0, 64, 129, 130], np.int64)
    out, sh = np.empty((3, 6, 256, 9), np.float32), np.empty((3, 6, 256, 6), np.float32)
    bp, ip, op, sp = inv.ctypes.data_as(f64p), ind.ctypes.data_as(i32p), out.ctypes.data_as(f32p), sh.ctypes.data_as(f32p)
    binp, xp, fp = bins.ctypes.data_as(i32p), idx.ctypes.data_as(i32p), off.ctypes.data_as(i64p)

    def call(box=bp, n=ip, K=9, b=None, nb=0, x=xp, o=fp, S=3, cur=1, res=op, size=out.nbytes):
        return lib.psa_partial_spectra(h, box, n, K, b, nb, x, o, S, cur, res, size)

    def refused(rc, word):
        msg = lib.psa_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    assert call() == 0
    assert call(b=binp, nb=6, res=sp, size=sh.nbytes) == 0
    # the species
    refused(call(S=0), "species")
    refused(call(S=9), "species")
    refused(call(x=None), "null")
    refused(call(o=None), "null")
    for bad, word in (([0, 64, 63, 130], "ascending"), ([1, 64, 129, 130], "begin at 0"), ([0, 64, 129, -1], "ascending")):
        refused(call(o=np.array(bad, np.int64).ctypes.data_as(i64p)), word)
    twice = idx.copy()
    twice[100] = 5
    refused(call(x=twice.ctypes.data_as(i32p)), "disjoint")
    for bad in (-1, 130):
        far = idx.copy()
        far[77] = bad
        refused(call(x=far.ctypes.data_as(i32p)), "out of bounds")
    refused(lib.psa_debug_partial_project(h, bp, ip, 9, xp, fp, 9, 1, out.ctypes.data_as(Ct.c_void_p)), "species")
    refused(lib.psa_debug_partial_project(h, bp, ip, 9, xp, fp, 3, 1, None), "null")
    z = np.zeros((2, 9, 4, 1, 8), np.complex64)
    refused(lib.psa_debug_partial_power(h, z.ctypes.data_as(Ct.c_void_p), None, None, 2, 0, 9, 0, 1, 8, 0, 0, 1.0, op), "species")
    refused(lib.psa_debug_partial_power(h, z.ctypes.data_as(Ct.c_void_p), None, None, 2, 0, 2, 0, 1, 8, 0, 0, 0.0, op), "norm")
    refused(lib.psa_debug_partial_power(h, None, None, None, 2, 0, 2, 0, 1, 8, 0, 0, 1.0, op), "null")
    down = np.array([1, 0], np.int32)
    refused(lib.psa_debug_partial_power(h, z.ctypes.data_as(Ct.c_void_p), None, down.ctypes.data_as(i32p), 2, 2, 2, 0, 1, 8, 0, 0, 1.0, op),
            "sorted by bin")
    # everything psa_lattice_spectra refuses
    refused(call(box=None), "null")
    refused(call(n=None), "null")
    refused(call(res=None), "null")
    refused(call(K=0), "at least one")
    refused(call(size=out.nbytes - 4), "out_bytes")
    refused(call(b=binp, nb=6), "out_bytes")                               # the shell form is (3, P, L, n_bins)
    refused(call(cur=2), "currents")
    for bad_inv, word in ((np.full(9, np.nan), "finite"), (np.zeros(9), "singular")):
        refused(call(box=bad_inv.ctypes.data_as(f64p)), word)
    far = ind.copy()
    far[4, 1] = -_hip.LAT_MAX_INDEX - 1
    refused(call(n=far.ctypes.data_as(i32p)), "is served")
    bb = bins.copy()
    bb[2] = 6
    refused(call(b=bb.ctypes.data_as(i32p), nb=6, res=sp, size=sh.nbytes), "outside")
    nn = ind.copy()
    nn[7] = (0, -1, 2)
    refused(call(n=nn.ctypes.data_as(i32p), b=binp, nb=6, res=sp, size=sh.nbytes), "half-space")
    assert call(n=nn.ctypes.data_as(i32p)) == 0                            # per vector: allowed
    engine.set_atom_weights(np.ones(129, np.float32))
    refused(call(), "weights")
    engine.set_atom_weights(None)
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 3 * 4 * 8 * 256 - 1)    # one vector holds S NC series
    refused(call(), "budget")
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 * 8 * 256)            # ... which serves one species
    one = np.empty((3, 1, 256, 9), np.float32)
    solo = np.array([0, 130], np.int64)
    assert call(o=solo.ctypes.data_as(i64p), S=1, res=one.ctypes.data_as(f32p), size=one.nbytes) == 0
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)
    engine.set_segments(Segments(512, 256, "hann"))
    big = np.empty((3, 6, 512, 9), np.float32)
    refused(call(res=big.ctypes.data_as(f32p), size=big.nbytes), "segment length")
    engine.set_segments(None)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, np.ascontiguousarray(vel[:128]))
    refused(call(), "shape")
    engine.release(_hip.SLOT_VELOCITIES)
    refused(call(), "velocities")
    rho = np.empty((1, 6, 256, 9), np.float32)
    assert call(cur=0, res=rho.ctypes.data_as(f32p), size=rho.nbytes) == 0     # the density needs none
    engine.release(_hip.SLOT_POSITIONS)
    refused(call(cur=0, res=rho.ctypes.data_as(f32p), size=rho.nbytes), "positions")


def test_no_trace_in_the_other_entry_points(engine, wave):
    """an ordinary `calculate` and a `calculate_lattice_spectra` give the bits they gave before the partial calls in between"""
    from psa_amd import Segments
    calc = _calculator(engine, wave["pos"], wave["vel"], wave["box"], cells=(4, 4, 4))
    mags, vecs = calc.get_k_path("100", 1.0, 24)
    for _ in range(2):                      # (the first call uploads and projects at once, the next builds what is cached)
        calc.calculate(mags, vecs)
    s = Segments(64, 32, "hann")
    before = calc.calculate(mags, vecs)
    lat_before = calc.calculate_lattice_spectra(wave["half"][:40], segments=s, atom_weights=wave["w"])
    pow_before = calc.calculate_powder_spectra(EDGES, segments=s, atom_weights=wave["w"])
    calc.calculate_powder_partial_spectra(EDGES, wave["species"], segments=s, atom_weights=wave["w"])
    calc.calculate_partial_spectra(wave["half"][:20], wave["species"], currents=False)
    after = calc.calculate(mags, vecs)
    lat_after = calc.calculate_lattice_spectra(wave["half"][:40], segments=s, atom_weights=wave["w"])
    pow_after = calc.calculate_powder_spectra(EDGES, segments=s, atom_weights=wave["w"])
    assert np.array_equal(_bits(before.sed), _bits(after.sed))
    for n in FIELDS:
        assert np.array_equal(_bits(getattr(lat_before, n)), _bits(getattr(lat_after, n))), n
        assert np.array_equal(_bits(getattr(pow_before, n)), _bits(getattr(pow_after, n))), n
    engine.timings()                                                       # (reset)
    calc.calculate_powder_partial_spectra(EDGES, wave["species"])
    timings = engine.timings()
    assert timings["project"] > 0 and timings["fft"] > 0 and timings["epilogue"] > 0 and timings["d2h"] > 0
