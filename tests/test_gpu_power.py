"""The passes that follow the FFT in psa_dynamic_spectra, psa_lattice_spectra and psa_self_spectra, driven alone through
psa_debug_dynamic_power, psa_debug_lattice_shell and psa_debug_self_power on transformed segments of the test's making
(tests/power_cases.py: inputs, bars and their derivation; tests/power64.py: the float64 references): the exact items bit for
bit, every element of every random case inside its bar with the worst element printed, transverse >= 0, the same bits from a
repeated call and -- in the shell and self forms -- from another cutting, every refusal, and no trace in the spectra
computed afterwards.  The shapes reach every grid-stride tail of dynamic_power_kernel, lattice_shell_kernel,
self_power_kernel and lattice_finish_kernel; the tail of self_reduce_kernel (n_groups L > 2^24, a 130 MB input) is not
reached."""
import ctypes as Ct

import numpy as np
import pytest

import lattice_cases as C
import power64 as R
import power_cases as P
from engine_state import reset

pytestmark = pytest.mark.gpu

ROWS = ("density", "longitudinal", "transverse")


@pytest.fixture(autouse=True)
def _clean(engine):
    reset(engine)
    yield
    reset(engine)


@pytest.fixture(scope="module", autouse=True)
def _forget(engine):
    yield
    engine.invalidate()


def _same(a, b):
    return np.array_equal(P.bits(a), P.bits(b))


def _dynamic(engine, args, **cut):
    seg, k, scale = args
    return engine.debug_dynamic_power(seg, k, scale, **cut)


def _shell(engine, args, **cut):
    seg, k, bin_of, n_bins, norm = args
    return engine.debug_lattice_shell(seg, P.khat32(k), bin_of, n_bins, norm, **cut)


def _self(engine, args, mirror, **cut):
    work, grp, cols, scale = args
    return engine.debug_self_power(work, grp, cols, scale, mirror, **cut)


def _inside(kind, name, got, ref, bars):
    for r, (f, at) in enumerate(P.worst(got, ref, bars)):
        print(f"{kind} {name} {ROWS[r]}: worst fraction of the bar {f:.3f} at {at}")
        assert f <= 1.0, (kind, name, ROWS[r], f, at)
    if got.ndim == 3 and got.shape[0] == 3:
        assert (got[2] >= 0).all(), (kind, name, float(got[2].min()))


# ---- exact items ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", P.EXACT_L)
def test_exact_items_bit_for_bit(engine, L):
    seg, k, scale = P.exact_dynamic(L)
    ref = R.dynamic64(seg, k, scale)["out"].astype(np.float32)
    for kb, sb in P.DYNAMIC_CUTS:
        assert _same(engine.debug_dynamic_power(seg, k, scale, kb, sb), ref), ("dynamic", kb, sb)
    assert not P.bits(engine.debug_dynamic_power(0 * seg, k, scale, 2, 3)).any()
    assert _same(engine.debug_dynamic_power(seg[:, :1], k, scale, 2, 3), ref[:1])                  # density alone

    seg, k, bin_of, n_bins, norm = P.exact_shell(L)
    ref = R.shell64(seg, k, bin_of, n_bins, norm)["out"].astype(np.float32)
    for kb, sb in P.SHELL_CUTS:
        got = engine.debug_lattice_shell(seg, P.khat32(k), bin_of, n_bins, norm, kb, sb)
        assert _same(got, ref), ("shell", kb, sb)
        assert not P.bits(got[:, :, [0, 3, 5]]).any()                       # empty bins first, in the middle, last
    assert not P.bits(engine.debug_lattice_shell(0 * seg, P.khat32(k), bin_of, n_bins, norm, 3, 3)).any()
    assert _same(engine.debug_lattice_shell(seg[:, :1], P.khat32(k), bin_of, n_bins, norm, 2, 1), ref[:1])

    for mirror in (True, False):
        work, grp, cols, sc = P.exact_self(L, mirror)
        ref = R.self64(work, grp, cols, sc, mirror).astype(np.float32)
        for cut in P.SELF_CUTS:
            assert _same(engine.debug_self_power(work, grp, cols, sc, mirror, **cut), ref), ("self", mirror, cut)
        assert not P.bits(engine.debug_self_power(0 * work, grp, cols, sc, mirror)).any()


# ---- per element ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in P.DYNAMIC_CASES])
def test_dynamic_power_inside_its_bars(engine, name):
    c, args, ref, bars = P.references()["dynamic"][name]
    got = _dynamic(engine, args, k_block=c["k_block"], seg_block=c["seg_block"])
    _inside("dynamic", name, got, ref, bars)
    assert _same(got, _dynamic(engine, args, k_block=c["k_block"], seg_block=c["seg_block"]))
    if c["k_block"] or c["seg_block"]:
        # another cutting: the vectors' blocks change nothing, the segments' blocks only what their bars allow
        assert _same(got, _dynamic(engine, args, k_block=1, seg_block=c["seg_block"]))
        whole = _dynamic(engine, args)
        other = P.dynamic_bars(ref, c["ns"], 0)
        _inside("dynamic", name + " uncut", whole, ref, other)
        assert (np.abs(whole.astype(np.float64) - got) <= bars + other).all()


@pytest.mark.parametrize("name", [c["name"] for c in P.SHELL_CASES])
def test_lattice_shell_inside_its_bars(engine, name):
    c, args, ref, bars = P.references()["shell"][name]
    got = _shell(engine, args, k_block=c["k_block"], seg_block=c["seg_block"])
    _inside("shell", name, got, ref, bars)
    empty = np.bincount(args[2], minlength=args[3]) == 0
    assert not P.bits(got[:, :, empty]).any()
    assert _same(got, _shell(engine, args, k_block=c["k_block"], seg_block=c["seg_block"]))
    if c["k_block"] or c["seg_block"]:
        assert _same(got, _shell(engine, args))
        assert _same(got, _shell(engine, args, k_block=1, seg_block=1))


@pytest.mark.parametrize("name", [c["name"] for c in P.SELF_CASES])
def test_self_power_inside_its_bars(engine, name):
    c, args, ref, bars = P.references()["self"][name]
    cut = dict(n_chunks=c["n_chunks"], atom_block=c["atom_block"], vec_block=c["vec_block"], seg_block=c["seg_block"])
    got = _self(engine, args, c["mirror"], **cut)
    _inside("self", name, got, ref, bars)
    assert _same(got, _self(engine, args, c["mirror"], **cut))
    if any(cut.values()):
        assert _same(got, _self(engine, args, c["mirror"]))
        assert _same(got, _self(engine, args, c["mirror"], n_chunks=1, atom_block=1, vec_block=1, seg_block=1))


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    lib, h = engine._lib, engine._h
    f32p, i32p, f64p, vp = Ct.POINTER(Ct.c_float), Ct.POINTER(Ct.c_int32), Ct.POINTER(Ct.c_double), Ct.c_void_p

    def refused(rc, word):
        msg = lib.psa_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    seg, k, scale = P.exact_dynamic(64)
    out = np.empty((3, 64, 5), np.float32)
    sp, kp, op = seg.ctypes.data_as(vp), k.ctypes.data_as(f32p), out.ctypes.data_as(f32p)
    assert lib.psa_debug_dynamic_power(h, sp, kp, 5, 1, 4, 64, 0, 0, scale, op) == 0
    refused(lib.psa_debug_dynamic_power(h, None, kp, 5, 1, 4, 64, 0, 0, scale, op), "null")
    refused(lib.psa_debug_dynamic_power(h, sp, None, 5, 1, 4, 64, 0, 0, scale, op), "null")
    refused(lib.psa_debug_dynamic_power(h, sp, kp, 5, 1, 4, 64, 0, 0, scale, None), "null")
    for bad in ((0, 1, 4, 64, 0, 0), (5, 1, 0, 64, 0, 0), (5, 1, 4, 0, 0, 0), (5, 1, 4, 64, -1, 0), (5, 1, 4, 64, 0, -1)):
        refused(lib.psa_debug_dynamic_power(h, sp, kp, *bad, scale, op), "positive")
    refused(lib.psa_debug_dynamic_power(h, sp, kp, 5, 2, 4, 64, 0, 0, scale, op), "currents")
    kk = k.copy()
    kk[3, 1] = np.nan
    refused(lib.psa_debug_dynamic_power(h, sp, kk.ctypes.data_as(f32p), 5, 1, 4, 64, 0, 0, scale, op), "not finite")

    seg, k, bin_of, n_bins, norm = P.exact_shell(64)
    kh = P.khat32(k)
    out = np.empty((3, 64, 6), np.float32)
    sp, kp, bp, op = seg.ctypes.data_as(vp), kh.ctypes.data_as(f32p), bin_of.ctypes.data_as(i32p), out.ctypes.data_as(f32p)
    assert lib.psa_debug_lattice_shell(h, sp, kp, bp, 7, 6, 1, 4, 64, 0, 0, norm, op) == 0
    assert lib.psa_debug_lattice_shell(h, sp, None, bp, 7, 6, 0, 16, 64, 0, 0, norm, op) == 0        # no currents: no k / |k|
    refused(lib.psa_debug_lattice_shell(h, None, kp, bp, 7, 6, 1, 4, 64, 0, 0, norm, op), "null")
    refused(lib.psa_debug_lattice_shell(h, sp, None, bp, 7, 6, 1, 4, 64, 0, 0, norm, op), "null")
    refused(lib.psa_debug_lattice_shell(h, sp, kp, None, 7, 6, 1, 4, 64, 0, 0, norm, op), "null")
    refused(lib.psa_debug_lattice_shell(h, sp, kp, bp, 7, 6, 1, 4, 64, 0, 0, norm, None), "null")
    for bad in ((0, 6, 1, 4, 64, 0, 0), (7, 6, 1, 0, 64, 0, 0), (7, 6, 1, 4, 0, 0, 0), (7, 6, 1, 4, 64, -2, 0), (7, 6, 1, 4, 64, 0, -2)):
        refused(lib.psa_debug_lattice_shell(h, sp, kp, bp, *bad, norm, op), "positive")
    refused(lib.psa_debug_lattice_shell(h, sp, kp, bp, 7, 0, 1, 4, 64, 0, 0, norm, op), "at least one bin")
    refused(lib.psa_debug_lattice_shell(h, sp, kp, bp, 7, 4, 1, 4, 64, 0, 0, norm, op), "outside")    # bin 4 of four bins
    for norm_bad in (0.0, -1.0, float("nan")):
        refused(lib.psa_debug_lattice_shell(h, sp, kp, bp, 7, 6, 1, 4, 64, 0, 0, norm_bad, op), "norm")
    bb = bin_of.copy()
    bb[0] = -1
    refused(lib.psa_debug_lattice_shell(h, sp, kp, bb.ctypes.data_as(i32p), 7, 6, 1, 4, 64, 0, 0, norm, op), "outside")
    bb = bin_of.copy()
    bb[[1, 3]] = bb[[3, 1]]
    refused(lib.psa_debug_lattice_shell(h, sp, kp, bb.ctypes.data_as(i32p), 7, 6, 1, 4, 64, 0, 0, norm, op), "sorted")

    work, grp, cols, sc = P.exact_self(64, True)
    out = np.empty((64, 3), np.float32)
    wp, gp, cp, op = work.ctypes.data_as(vp), grp.ctypes.data_as(i32p), sc.ctypes.data_as(f64p), out.ctypes.data_as(f32p)
    good = (3, 5, 4, 64)
    assert lib.psa_debug_self_power(h, wp, *good, gp, 3, 3, cp, 1, 0, 0, 0, 0, op) == 0
    refused(lib.psa_debug_self_power(h, None, *good, gp, 3, 3, cp, 1, 0, 0, 0, 0, op), "null")
    refused(lib.psa_debug_self_power(h, wp, *good, None, 3, 3, cp, 1, 0, 0, 0, 0, op), "null")
    refused(lib.psa_debug_self_power(h, wp, *good, gp, 3, 3, None, 1, 0, 0, 0, 0, op), "null")
    refused(lib.psa_debug_self_power(h, wp, *good, gp, 3, 3, cp, 1, 0, 0, 0, 0, None), "null")
    for bad in ((0, 5, 4, 64), (3, 0, 4, 64), (3, 5, 0, 64), (3, 5, 4, 0)):
        refused(lib.psa_debug_self_power(h, wp, *bad, gp, 3, 3, cp, 1, 0, 0, 0, 0, op), "positive")
    refused(lib.psa_debug_self_power(h, wp, *good, gp, 0, 3, cp, 1, 0, 0, 0, 0, op), "positive")
    refused(lib.psa_debug_self_power(h, wp, *good, gp, 3, 0, cp, 1, 0, 0, 0, 0, op), "positive")
    refused(lib.psa_debug_self_power(h, wp, *good, gp, 3, 3, cp, 2, 0, 0, 0, 0, op), "mirror")
    for bad in ((-1, 0, 0, 0), (65536, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)):
        refused(lib.psa_debug_self_power(h, wp, *good, gp, 3, 3, cp, 1, *bad, op), "n_chunks")
    refused(lib.psa_debug_self_power(h, wp, 3, 4, 4, 64, gp, 3, 3, cp, 1, 0, 0, 0, 0, op), "tile")      # the groups end at 5
    for row, val, word in ((0, (1, 0), "tile"), (2, (0, 2), "tile"), (1, (1, 3), "column"), (1, (1, -1), "column"),
                           (2, (1, 1), "column")):                          # gap at 0; descending; outside; outside; used twice
        gg = grp.copy()
        gg[row] = val
        refused(lib.psa_debug_self_power(h, wp, *good, gg.ctypes.data_as(i32p), 3, 3, cp, 1, 0, 0, 0, 0, op), word)
    ss = sc.copy()
    ss[1] = np.inf
    refused(lib.psa_debug_self_power(h, wp, *good, gp, 3, 3, ss.ctypes.data_as(f64p), 1, 0, 0, 0, 0, op), "not finite")


# ---- the spectra themselves -----------------------------------------------------------------------------------------------
def _calculator(engine, pos, vel, box, cells=(4, 4, 4)):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, vel, np.ones(n, np.int32), np.arange(n_t, dtype=np.float32), box, np.diag(box).copy(),
                    np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, *cells).attach(engine=engine)


@pytest.mark.parametrize("seg", [None, (32, 16, "hann")], ids=["whole", "hann_32_16"])
def test_no_negative_transverse_for_a_longitudinal_current(engine, seg):
    """every atom moves along d = (1, 2, 2) / 3 and every k is a multiple of d: the current is longitudinal up to the float32
    rounding of the velocities, the transverse spectrum a few u^2 of the longitudinal one -- and not negative, in
    psa_dynamic_spectra and in both forms of psa_lattice_spectra (psa_self_spectra has no transverse part)"""
    from psa_amd import Segments, _hip
    pos, vel = C.trajectory(40, 128, seed=5, box=C.CUBIC)
    d = np.array([1.0, 2.0, 2.0]) / 3.0
    vel = (np.sum(vel * d, axis=2, keepdims=True) * d).astype(np.float32)
    ind = np.array([[1, 2, 2], [2, 4, 4], [3, 6, 6], [5, 10, 10]], np.int32)
    inv = C.inverse(C.CUBIC)
    k = (2 * np.pi * ind @ inv.T).astype(np.float32)
    engine.ensure_resident(_hip.SLOT_POSITIONS, pos)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, vel)
    engine.set_segments(None if seg is None else Segments(*seg))
    results = {"dynamic": engine.dynamic_spectra(k), "lattice": engine.lattice_spectra(inv, ind),
               "shell": engine.lattice_spectra(inv, ind, bin_of=np.array([0, 0, 1, 3], np.int32), n_bins=4)}
    for name, got in results.items():
        lon, tra = got[1].astype(np.float64), got[2].astype(np.float64)
        print(f"{name}: min transverse {tra.min():.3e}, max transverse / max longitudinal {tra.max() / lon.max():.3e}")
        assert (got[2] >= 0).all(), (name, float(got[2].min()))
        # what is left is error: of a projection at most 2^-17 sum_a |v_a| with its transform, so of a power at most
        # 2^-34 N sum_a |v_a|^2, and sum_a |v_a|^2 is about the mean of the longitudinal spectrum: 40 x 2^-34 = 2e-9 of it
        assert lon.max() > 0 and tra.max() <= 1e-7 * lon.max(), name


def test_no_trace_in_the_spectra(engine):
    """`calculate`, the dynamic, lattice and self spectra give the bits they gave before the debug calls in between"""
    from psa_amd import Segments
    pos, vel = C.trajectory(40, 128, seed=8, box=C.CUBIC)
    calc = _calculator(engine, pos, vel, C.CUBIC)
    mags, vecs = calc.get_k_path("100", 1.0, 12)
    for _ in range(2):                      # (the first call uploads and projects at once, the next builds what is cached)
        calc.calculate(mags, vecs)
    s = Segments(32, 16, "hann")
    ind = C.mixed_indices(12, seed=3)
    edges = np.array([0.05, 0.4, 0.7, 1.0])
    k = (2 * np.pi * ind @ C.inverse(C.CUBIC).T).astype(np.float32)

    def everything():
        res = [calc.calculate_dynamic_spectra(np.linalg.norm(k, axis=1), k, segments=s), calc.calculate_lattice_spectra(ind, segments=s),
               calc.calculate_powder_spectra(edges, segments=s), calc.calculate_self_spectra(ind, segments=s),
               calc.calculate_powder_self_spectra(edges, segments=s)]
        return [calc.calculate(mags, vecs).sed] + [getattr(r, n) for r in res for n in ROWS if getattr(r, n) is not None]
    before = everything()
    for L in P.EXACT_L:
        engine.debug_dynamic_power(*P.exact_dynamic(L), 2, 3)
        seg, kk, bin_of, n_bins, norm = P.exact_shell(L)
        engine.debug_lattice_shell(seg, P.khat32(kk), bin_of, n_bins, norm, 2, 1)
        for mirror in (True, False):
            work, grp, cols, sc = P.exact_self(L, mirror)
            engine.debug_self_power(work, grp, cols, sc, mirror, **P.SELF_CUTS[1])
    after = everything()
    assert len(before) == 1 + 3 + 3 + 3 + 1 + 1
    for i, (a, b) in enumerate(zip(before, after)):
        assert a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), i
