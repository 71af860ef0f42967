"""The spectral stage on the GPU -- the batched FFT, the kernels of k2_epilogue.hip, the k map of folded (k, -k) lists,
the Welch segment stage with every block regime, the block-by-block complex result, single_bin -- against exact NumPy
twins where the operation is a permutation plus correctly rounded arithmetic, and against float64 per k-row elsewhere.
Inputs, twins and the derivation of every bar: tests/spectral_cases.py; that the planted faults are visible and that a
float32 model of the stage uses at most half of the end-to-end bars: tests/test_spectral_host.py.

a. Epilogue kernels alone.  One cheap projection gives a slab of the wanted geometry; psa_slab_write puts a crafted slab
   in its place, psa_sed_set_kmap a crafted map, psa_sed_finalize runs the kernel.  The complex result and the intensity
   result are compared BIT FOR BIT with finalize_model / transpose_model; the companion intensity is held to 6 u of the
   float64 sum of the device's own result, psa_result_intensity to the companion's bits, the chiral phase to CHIRAL_BAR
   on every element.  (result_intensity_kernel itself cannot be reached through the ABI: every call that leaves a valid
   complex result also leaves its companion intensity, so psa_result_intensity never recomputes.  What can be asserted
   is that it never serves a stale one.)
b. Full spectrum through Engine.calculate, per k-row against float64: a T axis and a K axis, folded lists (fold on
   against the float64 SED of the unfolded list and against fold off), the block-by-block path with a folded list and
   both of its copy strategies.
c. Welch, per k-row against float64, on shapes that take every split of segment_blocks(): none, k-vectors with a ragged
   last block, segments with a ragged last block / a single last segment / even blocks -- those also with two groups
   and with mirrored columns.
d. single_bin against the float64 DFT of the float64 projection.

Each case prints its shape, the regime taken, the worst error and its ratio to the bar."""
import numpy as np
import pytest

import dense_cases as D
import spectral_cases as W
from conftest import rel_max
from ref64 import intensity64, project64, row_rel, scale_B, sed64
from test_gpu_dense_envelope import TOL, TOL_ROW
from welch64 import welch_intensity64
from engine_state import reset

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng(engine):
    reset(engine)
    try:
        yield engine
    finally:
        reset(engine)
        for slot in (0, 1):
            engine.release(slot)
        engine.invalidate()


@pytest.fixture(scope="module")
def mirror():
    """the mirror flag: the library's constant, checked against what psa_k_pairs sets on a (k, -k) list"""
    from psa_amd import _hip
    kmap, uniq = _hip.k_pairs(np.float32([[0.3, -0.2, 0.9], [-0.3, 0.2, -0.9]]))
    assert list(uniq) == [0] and kmap[1] == _hip.KMAP_MIRROR
    return _hip.KMAP_MIRROR


def _assert_bits(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    g, w = W.bits(got), W.bits(want)
    bad = np.argwhere(g != w)
    print(f"{name}: {g.size} words, {len(bad)} differ")
    assert len(bad) == 0, f"{name}: {len(bad)} of {g.size} words differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]:#010x} != {w[tuple(bad[0])]:#010x}"


# ---- a. the epilogue kernels alone ------------------------------------------------------------------------------------
_ZEROS = {}


def _slab_of(engine, T, rows, intensity):
    """a result slab of (rows, 3, T) complex64 / (rows, T) float32 on the device: a zero trajectory of two atoms, `rows`
    random k-vectors without pairs"""
    from psa_amd import _hip
    z = _ZEROS.setdefault(T, np.zeros((T, 2, 3), np.float32))
    engine.ensure_resident(0, z)
    engine.project(0, D.positions(2, 3), D.k_list(rows, seed=11), None, _hip.F_INTENSITY if intensity else 0)


def _install(engine, slab, kmap):
    engine.slab_write(0, slab)
    if kmap is not None:
        engine.set_kmap(kmap)


@pytest.mark.parametrize("T,rows,K_out,name", W.epilogue_table())
def test_finalize_complex_bit_for_bit(eng, mirror, T, rows, K_out, name):
    kmap = W.k_map(name, rows, K_out, mirror)
    slab = W.craft_complex(rows, T)
    _slab_of(eng, T, rows, False)
    _install(eng, slab, kmap)
    out, inten = eng.finalize(T, K_out, False, with_intensity=True)
    tag = f"complex T={T} rows={rows} K_out={K_out} {name}"
    _assert_bits(tag, out, W.finalize_model(slab, kmap, T, mirror))
    ratio = W.intensity_check(inten, out)
    print(f"{tag}: companion intensity {ratio:.3f} x (6 u)")
    assert ratio <= 1.0
    _assert_bits(tag + " result_intensity", np.asarray(eng.result_intensity(T, K_out)), np.asarray(inten))


@pytest.mark.parametrize("T,rows,K_out,name", W.epilogue_table())
def test_finalize_intensity_bit_for_bit(eng, mirror, T, rows, K_out, name):
    kmap = W.k_map(name, rows, K_out, mirror)
    slab = W.craft_intensity(rows, T)
    _slab_of(eng, T, rows, True)
    _install(eng, slab, kmap)
    out = eng.finalize(T, K_out, True)
    _assert_bits(f"intensity T={T} rows={rows} K_out={K_out} {name}", out, W.transpose_model(slab, kmap, mirror))


@pytest.mark.parametrize("T", [1, 2, 65, 100])
def test_chiral_phase_every_element(eng, mirror, T):
    rows, K_out = 9, 17
    kmap = W.k_map("twins", rows, K_out, mirror)
    _slab_of(eng, T, rows, False)
    _install(eng, W.craft_chiral(rows, T), kmap)
    out = eng.finalize(T, K_out, False)
    _assert_bits(f"chiral slab T={T}", out, W.finalize_model(W.craft_chiral(rows, T), kmap, T, mirror))
    for c1, c2 in ((0, 1), (1, 2), (2, 0)):
        got = np.asarray(eng.result_chiral_phase(T, K_out, c1, c2))
        ref = W.chiral_ref64(out, c1, c2)
        assert np.all(np.isfinite(got)) and np.all(np.abs(got) <= np.float32(np.pi / 2) * (1 + 2.0 ** -22))
        err = np.abs(got.astype(np.float64) - ref)
        i = np.unravel_index(np.argmax(err), err.shape)
        print(f"chiral T={T} ({c1}, {c2}): worst {err.max():.3e} rad at {i} = {err.max() / W.CHIRAL_BAR:.3f} x bar {W.CHIRAL_BAR:.2e}")
        assert err.max() <= W.CHIRAL_BAR


def test_result_intensity_never_serves_a_stale_slab(eng, mirror):
    from psa_amd import _hip
    T, rows, K_out = W.EPILOGUE_BASE
    kmap = W.k_map("alternating", rows, K_out, mirror)
    a = W.craft_complex(rows, T, specials=False)
    b = np.ascontiguousarray(a[::-1]) * np.float32(3)                  # other values in every cell
    _slab_of(eng, T, rows, False)
    _install(eng, a, kmap)
    out_a, inten_a = eng.finalize(T, K_out, False, with_intensity=True)
    _assert_bits("first slab", np.asarray(eng.result_intensity(T, K_out)), np.asarray(inten_a))
    _install(eng, b, kmap)
    with pytest.raises(_hip.PsaHipError, match="finalized complex result"):
        eng.result_intensity(T, K_out)                                 # the result on the device is the old slab's
    out_b = eng.finalize(T, K_out, False)
    _assert_bits("second slab", out_b, W.finalize_model(b, kmap, T, mirror))
    got = np.asarray(eng.result_intensity(T, K_out))
    assert W.intensity_check(got, out_b) <= 1.0
    assert W.intensity_check(got, out_a) > 1e3                         # not the first slab's


# ---- b. the full spectrum, per row ------------------------------------------------------------------------------------
_WORST = {}


def _check(tag, name, got, ref, scale):
    """rel_max <= scale TOL and every k-row <= scale TOL_ROW; prints both with their ratios"""
    got = np.asarray(got)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), name
    err, rows = rel_max(got, ref), row_rel(got, ref)
    a, b = err / (scale * TOL), float(rows.max()) / (scale * TOL_ROW)
    for key, v in ((f"{tag} TOL", a), (f"{tag} TOL_ROW", b)):
        _WORST[key] = max(_WORST.get(key, 0.0), v)
    msg = (f"{name} {tag} {got.shape}: rel_max {err:.2e} = {a:.2f} x bar, worst row {rows.max():.2e} (k {int(np.argmax(rows))}) = "
           f"{b:.2f} x bar; worst so far " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(_WORST.items())))
    print(msg)
    assert a <= 1.0 and b <= 1.0, msg


def _calculate(engine, c, groups=None, flags=0, **kw):
    engine.ensure_resident(0, c["data"])
    n0 = engine.lowrank_launches()
    got = engine.calculate(0, c["r"], c["k"], groups, flags, **kw)
    assert engine.lowrank_launches() == n0
    return got


def _full(engine, c, name):
    """complex + companion intensity, and incoherent on two groups, each per row against float64; returns the complex pair"""
    from psa_amd import _hip
    data, r, k = c["data"], c["r"], c["k"]
    out, inten = _calculate(engine, c, with_intensity=True)
    _check("complex", name, out, sed64(data, r, k), 1)
    _check("companion", name, inten, intensity64(data, r, k, [None]), 2)
    assert W.intensity_check(np.asarray(inten), np.asarray(out)) <= 1.0
    groups = W.two_groups(data.shape[1])
    _check("incoherent", name, _calculate(engine, c, groups, _hip.F_INTENSITY), intensity64(data, r, k, groups), 2)
    return np.array(out), np.array(inten)


@pytest.mark.parametrize("family,K,T", W.full_table())
def test_full_spectrum_per_row(eng, family, K, T):
    _full(eng, W.full_case(family, K, T), f"{family} K={K} T={T}")


@pytest.mark.parametrize("family,name,T", W.fold_table())
def test_folded_lists_per_row(eng, mirror, family, name, T):
    from psa_amd import _hip
    c = W.folded_case(family, name, T)
    kmap, uniq = _hip.k_pairs(c["k"])
    n_mirrored = int(np.count_nonzero(kmap & np.uint32(mirror)))
    assert len(uniq) < len(c["k"]) and n_mirrored >= 5, "the list does not fold"
    tag = f"{family} {name} T={T} K_out={len(c['k'])} rows={len(uniq)} mirrored={n_mirrored}"
    on, on_i = _full(eng, c, tag + " fold on")
    eng.set_option(_hip.OPT_FOLD_PAIRS, 0)
    off, off_i = _calculate(eng, c, with_intensity=True)
    _check("complex", tag + " fold off", off, sed64(c["data"], c["r"], c["k"]), 1)
    a, b = float(row_rel(on, np.asarray(off)).max()), float(row_rel(on_i, np.asarray(off_i)).max())
    print(f"{tag}: fold on against off, worst row complex {a:.2e}, companion {b:.2e}")
    assert a <= TOL_ROW and b <= 2 * TOL_ROW


def test_pipelined_folded_list_both_copy_strategies(eng, mirror, monkeypatch):
    from psa_amd import _hip
    monkeypatch.setenv("PSA_PIPELINE_BLOCKS", W.PIPELINE_BLOCKS)
    res = {}
    for order in ("runs2", "scattered"):
        c, where = W.pipeline_case(order)
        kmap, uniq = _hip.k_pairs(c["k"])
        assert len(c["k"]) >= 192 and np.array_equal(uniq, np.arange(100))
        runs = W.pipeline_runs_model(kmap, [16, 16, 40, 28], mirror)
        assert (max(runs) <= 8) == (order == "runs2"), runs
        name = f"pipelined {order} blocks 16,16,40,28 runs {runs}"
        out, inten = _calculate(eng, c, with_intensity=True)
        _check("complex", name, out, sed64(c["data"], c["r"], c["k"]), 1)
        _check("companion", name, inten, intensity64(c["data"], c["r"], c["k"], [None]), 2)
        res[order] = (np.array(out)[:, where], np.array(inten)[:, where])
    _assert_bits("copy per block against one copy at the end, complex", res["scattered"][0], res["runs2"][0])
    _assert_bits("copy per block against one copy at the end, intensity", res["scattered"][1], res["runs2"][1])


# ---- c. Welch, per row, every block regime ----------------------------------------------------------------------------
def _regime(K_local, c):
    b = W.segment_blocks_model(K_local, c["data"].shape[0], c["L"], c["H"])
    return b, dict(regime=b["regime"], k_ragged=b["k_blocks"][-1] != b["nk"], s_ragged=b["s_blocks"][-1] != b["ns"],
                   last_s=b["s_blocks"][-1])


@pytest.mark.parametrize("name,variant,kind", W.welch_table())
def test_welch_per_row(eng, mirror, name, variant, kind):
    from psa_amd import Segments, _hip
    c = W.welch_case(name, variant)
    kmap, uniq = _hip.k_pairs(c["k"])
    assert len(uniq) == c["K_local"]
    b, took = _regime(c["K_local"], c)
    assert took == c["expect"], (took, c["expect"])
    w = W.window(kind, c["L"])
    seg = Segments(c["L"], c["H"], w)
    assert np.array_equal(seg.window_array(), w)
    groups = None if c["groups"] == [None] else c["groups"]
    ref = welch_intensity64(c["data"], c["r"], c["k"], c["groups"], w, c["L"], c["H"])
    tag = (f"welch {name} {variant or 'one group'} {kind} K_out={len(c['k'])} T={c['data'].shape[0]} L={c['L']} H={c['H']}: "
           f"{b['regime']} split, k blocks {b['k_blocks'][:3]}{'...' if len(b['k_blocks']) > 3 else ''}, segment blocks {b['s_blocks']}")
    eng.set_segments(seg)
    on = np.array(_calculate(eng, c, groups, _hip.F_INTENSITY))
    _check("welch", tag, on, ref, 2)
    if len(uniq) < len(c["k"]):
        eng.set_option(_hip.OPT_FOLD_PAIRS, 0)
        b_off, _ = _regime(len(c["k"]), c)
        off = np.array(_calculate(eng, c, groups, _hip.F_INTENSITY))
        _check("welch", tag + f" | fold off: {b_off['regime']} split, segment blocks {b_off['s_blocks']}", off, ref, 2)
        a = float(row_rel(on, off).max())
        print(f"  fold on against off: worst row {a:.2e}")
        assert a <= 2 * TOL_ROW


# ---- d. single_bin ----------------------------------------------------------------------------------------------------
SINGLE_BIN = [(1, "all"), (1023, "all"), (1024, "dup"), (1025, "disp"), (2500, "all"), (1024, "all")]
_BIN_WORST = [0.0, 0.0]


@pytest.mark.parametrize("T,mode", SINGLE_BIN)
def test_single_bin_against_the_float64_dft(eng, T, mode):
    """The form: a one-vector list under K1_AUTO with no cached planes (asserted) is below the 17 k-vectors of the f16
    forms (2 K <= 32: k1_pair_eligible) and is served by k1_split, "3 x bf16" -- as tests/test_gpu_dense_envelope.py selects
    that form for lists of up to 16; in displacement mode the float32 difference array is materialised first, so the same
    kernel runs on it."""
    from psa_amd import _hip
    n = 7
    rng = np.random.default_rng(900 + T)
    r0 = D.positions(n, 41, edge=10.0, shift=40.0 if mode == "disp" else 0.0)
    if mode == "disp":
        data = (r0[None].astype(np.float64) + 0.05 * rng.standard_normal((T, n, 3))).astype(np.float32)
        r = np.mean(data, axis=0, dtype=np.float32)
    else:
        data, r = rng.standard_normal((T, n, 3)).astype(np.float32), r0
    idx = np.array([0, 3, 3, 5], np.int32) if mode == "dup" else None
    n_g = n if idx is None else len(idx)
    k = D.k_list(1, seed=23)
    slot, flags = (1, _hip.F_DISPLACEMENTS) if mode == "disp" else (0, 0)
    eng.ensure_resident(slot, data)
    q = project64(data, r, k, idx, None, mode == "disp")[0]
    B = scale_B(data, r, idx, None, mode == "disp")
    for b in sorted({0, 1 % T, T // 2, T - 1}):
        got = eng.single_bin(slot, r, k[0], idx, b, flags)
        assert eng.plane_cache()[0] == 0
        ref = W.single_bin_ref64(q, b)
        bar = W.single_bin_bar("bf16x3", n_g, B, ref)
        err = np.maximum(np.abs(got.real.astype(np.float64) - ref.real), np.abs(got.imag.astype(np.float64) - ref.imag))
        _BIN_WORST[0], _BIN_WORST[1] = max(_BIN_WORST[0], float(np.max(err / bar))), max(_BIN_WORST[1], float(np.max(err / B.mean(axis=1))))
        print(f"single_bin T={T} {mode} n_g={n_g} bin {b}: worst error {err.max():.3e} = {np.max(err / bar):.3f} x bar "
              f"({np.max(err / B.mean(axis=1)) / W.U:.2f} u of mean B); worst so far {_BIN_WORST[0]:.3f} x bar, {_BIN_WORST[1] / W.U:.2f} u")
        assert np.all(err <= bar)
