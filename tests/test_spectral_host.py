"""Proof, without a GPU, that the spectral-stage suite (tests/test_gpu_spectral.py) can fail and that its end-to-end
bars leave room for a correct float32 implementation.

  * The crafted slabs of tests/spectral_cases.py have the properties the exact tests rest on: all values distinct, none
    its own conjugate, no conjugate or negation of one equal to another, the special cells present.  For every (T, rows,
    K_out, map) of the GPU table, finalize_model differs in at least one bit from every planted fault that is not a
    no-op at that shape -- a wrong mirror index, a DC bin read one past the row or not conjugated, a dropped or an extra
    conjugation, a dropped ragged tile, a swap inside a tile, a Nyquist bin not conjugated -- and transpose_model from a
    mirrored column that is not reversed.  Every fault is live in at least one case of the table.
  * A float32 model of the whole stage -- the model of the projection split (dense_cases), SciPy's complex64 FFT, the
    float32 division, squares and sums; for Welch the segment stage with its blocks -- stays within HALF of TOL and
    TOL_ROW (doubled for intensities) on every end-to-end case of the GPU table.  The worst ratios are printed.
  * Faults on the Welch and fold paths -- a later segment block overwriting, the ragged last block dropped, inv_norm from
    the block's own segment count, a mirrored Welch column not reversed, a second group overwriting the first, a 1e-3
    relative error on the incoherent rows beside a coherent one -- exceed the row bar at least 5 x.  The last one passes
    the older rel_max <= 1e-5 bar: that is what the per-row metric is for."""
import numpy as np
import pytest

import spectral_cases as W
from conftest import rel_max
from ref64 import intensity64, row_rel, sed64
from test_gpu_dense_envelope import TOL, TOL_ROW
from welch64 import welch_intensity64

import dense_cases as D


@pytest.fixture(scope="module")
def mirror():
    """the mirror flag of a k map, from the library's constant, checked against what psa_k_pairs sets on a (k, -k) list"""
    from psa_amd import _hip
    k = np.float32([[0.3, -0.2, 0.9], [-0.3, 0.2, -0.9]])
    kmap, uniq = _hip.k_pairs(k)
    assert list(uniq) == [0] and kmap[0] == 0 and kmap[1] == _hip.KMAP_MIRROR
    return _hip.KMAP_MIRROR


# ---- crafted slabs --------------------------------------------------------------------------------------------------
def _geometries():
    return sorted({(T, rows) for T, rows, _, _ in W.epilogue_table()})


@pytest.mark.parametrize("T,rows", _geometries())
def test_crafted_slabs_have_the_stated_properties(T, rows):
    for slab in (W.craft_complex(rows, T), W.craft_chiral(rows, T) if rows >= 4 else W.craft_complex(rows, T)):
        assert slab.shape == (rows, 3, T) and slab.dtype == np.complex64 and not np.any(np.isnan(slab.view(np.float32)))
    slab = W.craft_complex(rows, T)
    v = slab.reshape(-1)
    n = v.size
    as_bits = lambda re, im: (np.ascontiguousarray(re, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        np.ascontiguousarray(im, np.float32).view(np.uint32).astype(np.uint64)
    own = as_bits(v.real, v.imag)
    assert len(np.unique(own)) == n, "values are not distinct"
    assert np.all(v.imag != 0), "a value is its own conjugate"
    for what, other in (("conjugate", as_bits(v.real, -v.imag)), ("negation", as_bits(-v.real, -v.imag))):
        assert not np.intersect1d(own, other).size, f"the {what} of a value is a value of the slab"
    if n >= 20:
        re, im = v.real.copy().view(np.uint32), v.imag.copy().view(np.uint32)
        for val in (0.0, -0.0, W.SUBNORMAL, W.FLT_MAX, np.inf, -np.inf):
            assert np.any(re == np.float32(val).view(np.uint32)), f"no real part {val}"
        for val in (W.SUBNORMAL, -W.FLT_MAX, np.inf, -np.inf):
            assert np.any(im == np.float32(val).view(np.uint32)), f"no imaginary part {val}"
    inten = W.craft_intensity(rows, T).reshape(-1)
    assert len(np.unique(inten.view(np.uint32))) == inten.size
    if inten.size >= 10:
        for val in (0.0, -0.0, W.SUBNORMAL, W.FLT_MAX, np.inf):
            assert np.any(inten.view(np.uint32) == np.float32(val).view(np.uint32))


def _live(fault, T, K_out, kmap, mirror):
    """whether the fault changes anything at this shape"""
    mirrored = kmap is not None and bool(np.any(np.asarray(kmap, np.uint32) & np.uint32(mirror)))
    plain = kmap is None or bool(np.any((np.asarray(kmap, np.uint32) & np.uint32(mirror)) == 0))
    return {"mirror_T-1-w": mirrored and T > 1, "dc_to_T": mirrored, "dc_in_place": mirrored, "no_conj": mirrored,
            "conj_plain": plain, "drop_last_tile": K_out % 16 != 0, "swap_in_tile": K_out >= 2,
            "nyquist_not_conj": mirrored and T % 2 == 0}[fault]


@pytest.mark.parametrize("T,rows,K_out,name", W.epilogue_table())
def test_every_planted_fault_changes_bits(mirror, T, rows, K_out, name):
    kmap = W.k_map(name, rows, K_out, mirror)
    slab = W.craft_complex(rows, T)
    good = W.finalize_model(slab, kmap, T, mirror)
    assert good.shape == (T, K_out, 3)
    assert np.array_equal(W.bits(good), W.bits(W.finalize_model(slab, kmap, T, mirror)))
    for fault in W.FINALIZE_FAULTS:
        if not _live(fault, T, K_out, kmap, mirror):
            continue
        bad = W.finalize_model(slab, kmap, T, mirror, fault=fault)
        assert not np.array_equal(W.bits(good), W.bits(bad)), f"{fault} is invisible at T={T} rows={rows} K_out={K_out} {name}"
    inten = W.craft_intensity(rows, T)
    good_i = W.transpose_model(inten, kmap, mirror)
    if kmap is not None and np.any(kmap & np.uint32(mirror)) and T > 2:
        assert not np.array_equal(W.bits(good_i), W.bits(W.transpose_model(inten, kmap, mirror, fault="unreversed")))
    # the model against a direct statement on one plain and one mirrored column
    src = np.arange(rows) if kmap is None else (kmap & ~np.uint32(mirror)).astype(int)
    for col in (0, K_out - 1):
        m = kmap is not None and bool(kmap[col] & np.uint32(mirror))
        for w in (0, T // 2, T - 1):
            cell = slab[src[col], 1, (T - w) % T if m else w]
            with np.errstate(all="ignore"):
                re, im = np.float32(cell.real) / np.float32(T), np.float32(cell.imag) / np.float32(T)
            want = np.array([re, -im if m else im], np.float32)
            assert np.array_equal(want.view(np.uint32), np.array([good[w, col, 1].real, good[w, col, 1].imag], np.float32).view(np.uint32))
            assert good_i[w, col].view(np.uint32) == inten[src[col], (T - w) % T if m else w].view(np.uint32)


def test_every_fault_is_live_somewhere_in_the_table(mirror):
    for fault in W.FINALIZE_FAULTS:
        n = sum(_live(fault, T, K_out, W.k_map(name, rows, K_out, mirror), mirror) for T, rows, K_out, name in W.epilogue_table())
        assert n >= 3, fault


# ---- the bars of the exact-arithmetic items ---------------------------------------------------------------------------
def test_intensity_bar_sees_1e_6_on_one_element_and_holds_on_the_special_cells(mirror):
    T, rows, K_out = W.EPILOGUE_BASE
    out = W.finalize_model(W.craft_complex(rows, T), W.k_map("alternating", rows, K_out, mirror), T, mirror)
    with np.errstate(all="ignore"):
        good = W.intensity32([out])
    assert W.intensity_check(good, out) <= 1.0
    finite = np.flatnonzero(np.isfinite(good.reshape(-1)) & (good.reshape(-1) > 1e-3))
    bad = good.copy().reshape(-1)
    bad[finite[7]] *= np.float32(1 + 1e-6)                        # 17 u on one element: the old rtol 2e-6 .. 5e-6 passes it
    assert W.intensity_check(bad.reshape(good.shape), out) > 1.0
    assert np.isinf(good).any() and (good == 0).sum() == 0


def test_chiral_reference_is_continuous_and_the_bar_is_the_documented_sum():
    assert W.CHIRAL_BAR == 19 * 2.0 ** -22
    pi_err = abs(float(np.float32(np.pi)) - np.pi) * 2 ** 22
    two_pi_err = abs(float(np.float32(2 * np.pi)) - 2 * np.pi) * 2 ** 22
    assert 18 < 12 + 1 + 2 + 3 * pi_err + two_pi_err + 1 + 0.5 + 0.25 <= 19
    # f(d) near the wrap (+-pi) and the folds (+-pi/2): neighbours 1e-9 apart map to neighbours 1e-9 apart
    for d0 in (np.pi, -np.pi, np.pi / 2, -np.pi / 2, 0.0, 2 * np.pi):
        for eps in (-1e-9, 1e-9):
            z = np.zeros((1, 2, 3), np.complex128)
            z[0, 0, 0], z[0, 0, 1] = np.exp(1j * d0), 1.0
            z[0, 1, 0], z[0, 1, 1] = np.exp(1j * (d0 + eps)), 1.0
            f = W.chiral_ref64(z, 0, 1)
            assert abs(f[0, 0] - f[0, 1]) <= 2e-9, (d0, eps, f)
    z = np.zeros((1, 1, 3), np.complex64)                          # (0, 0) against (0, 0): zero; against (-0, -0): pi -> 0
    assert W.chiral_ref64(z, 0, 1)[0, 0] == 0.0


def test_segment_blocks_model_takes_the_regimes_the_table_names():
    regimes = set()
    for name, (Kb, kind, T, L, H, regime, k_rag, s_rag, last) in W.WELCH_SHAPES.items():
        for variant in ("",) + W.WELCH_VARIANTS.get(name, ()):
            c = W.welch_case(name, variant)
            b = W.segment_blocks_model(c["K_local"], T, L, H)
            assert sum(b["k_blocks"]) == c["K_local"] and sum(b["s_blocks"]) == b["n_seg"] == 1 + (T - L) // H
            assert max(b["k_blocks"]) * max(b["s_blocks"]) * L <= max(c["K_local"] * T, L), "segment buffer larger than q"
            got = dict(regime=b["regime"], k_ragged=b["k_blocks"][-1] != b["nk"], s_ragged=b["s_blocks"][-1] != b["ns"],
                       last_s=b["s_blocks"][-1])
            assert got == c["expect"], (name, variant, b)
            regimes.add((got["regime"], got["k_ragged"], got["s_ragged"]))
    assert {("none", False, False), ("k", True, False), ("segments", False, True), ("segments", False, False)} <= regimes
    b = W.segment_blocks_model(2, 200, 64, 7)
    assert (b["nk"], b["ns"], b["s_blocks"]) == (1, 6, [6, 6, 6, 2])
    b = W.segment_blocks_model(24, 256, 64, 2)
    assert (b["nk"], b["ns"], b["s_blocks"]) == (1, 96, [96, 1])


# ---- the float32 model stays inside half of the end-to-end bars -------------------------------------------------------
_WORST = {}


def _ratios(tag, got, ref, scale):
    """rel_max / (scale TOL) and the worst row / (scale TOL_ROW); kept for the summary line"""
    assert np.all(np.isfinite(got))
    a, b = rel_max(got, ref) / (scale * TOL), float(row_rel(got, ref).max()) / (scale * TOL_ROW)
    for key, v in ((f"{tag} TOL", a), (f"{tag} TOL_ROW", b)):
        _WORST[key] = max(_WORST.get(key, 0.0), v)
    return a, b


def _print_worst():
    print("  worst ratio of the float32 model so far: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(_WORST.items())))


def _full_model(c, name):
    """the float32 model on a full-spectrum case: complex + companion intensity, and incoherent on two groups"""
    data, r, k = c["data"], c["r"], c["k"]
    S = W.spectrum32(W.q_model(c))
    out = [_ratios("complex", S, sed64(data, r, k), 1), _ratios("companion", W.intensity32([S]), intensity64(data, r, k, [None]), 2)]
    groups = W.two_groups(data.shape[1])
    Sg = [W.spectrum32(W.q_model(D.with_idx(c, g))) for g in groups]
    out.append(_ratios("incoherent", W.intensity32(Sg), intensity64(data, r, k, groups), 2))
    worst = max(max(p) for p in out)
    print(f"{name}: float32 model at (TOL, TOL_ROW) ratios complex {out[0][0]:.2f} {out[0][1]:.2f}, companion {out[1][0]:.2f} "
          f"{out[1][1]:.2f}, incoherent {out[2][0]:.2f} {out[2][1]:.2f}")
    _print_worst()
    assert worst <= 0.5, name


@pytest.mark.parametrize("family,K,T", W.full_table())
def test_float32_model_full_spectrum(family, K, T):
    _full_model(W.full_case(family, K, T), f"{family} K={K} T={T}")


@pytest.mark.parametrize("family,name,T", W.fold_table())
def test_float32_model_folded_lists(family, name, T):
    _full_model(W.folded_case(family, name, T), f"{family} {name} T={T}")


@pytest.mark.parametrize("order", ["runs2", "scattered"])
def test_float32_model_pipelined(mirror, order):
    from psa_amd import _hip
    c, where = W.pipeline_case(order)
    kmap, uniq = _hip.k_pairs(c["k"])
    assert len(uniq) == 100 and np.array_equal(uniq, np.arange(100))
    blocks = [16, 16, 40, 28]
    runs = W.pipeline_runs_model(kmap, blocks, mirror)
    print(f"{order}: runs of columns per block {runs}")
    assert (max(runs) <= 8) == (order == "runs2")
    assert np.array_equal(c["k"][where], W.pipeline_case("runs2")[0]["k"])
    if order == "runs2":
        _full_model(c, "pipelined list")


def _welch_model(c, kind, mirror, fault=None):
    """(L, K_out) float32 by the float32 model and the float64 reference of a Welch case"""
    from psa_amd import _hip
    kmap, uniq = _hip.k_pairs(c["k"])
    assert len(uniq) == c["K_local"]
    w = W.window(kind, c["L"])
    cu = dict(c, k=np.ascontiguousarray(c["k"][uniq]))
    qs = [W.q_model(cu if g is None else D.with_idx(cu, g)) for g in c["groups"]]
    rows = W.welch_model32(qs, w, c["L"], c["H"], fault=None if fault == "unreversed" else fault)
    got = W.transpose_model(rows, kmap, mirror, fault="unreversed" if fault == "unreversed" else None)
    ref = welch_intensity64(c["data"], c["r"], c["k"], c["groups"], w, c["L"], c["H"])
    return got, ref


@pytest.mark.parametrize("name,variant,kind", W.welch_table())
def test_float32_model_welch(mirror, name, variant, kind):
    c = W.welch_case(name, variant)
    got, ref = _welch_model(c, kind, mirror)
    a, b = _ratios("welch", got, ref, 2)
    print(f"welch {name} {variant or 'one group'} {kind}: float32 model at (2 TOL, 2 TOL_ROW) ratios {a:.2f} {b:.2f}")
    _print_worst()
    assert max(a, b) <= 0.5


# ---- faults on the Welch and fold paths --------------------------------------------------------------------------------
WELCH_FAULT_CASES = [("overwrite", "seg_ragged", ""), ("overwrite", "seg_last_single", ""), ("drop_ragged", "seg_ragged", ""),
                     ("drop_ragged", "seg_last_single", ""), ("norm_ns", "seg_ragged", ""), ("norm_ns", "seg_last_single", ""),
                     ("group_overwrite", "seg_ragged", "groups"), ("group_overwrite", "seg_last_single", "groups"),
                     ("unreversed", "seg_last_single", "fold12")]


@pytest.mark.parametrize("kind", W.WELCH_WINDOWS)
@pytest.mark.parametrize("fault,name,variant", WELCH_FAULT_CASES)
def test_welch_faults_exceed_the_row_bar(mirror, fault, name, variant, kind):
    c = W.welch_case(name, variant)
    bad, ref = _welch_model(c, kind, mirror, fault=fault)
    ratio = float(row_rel(bad, ref).max()) / (2 * TOL_ROW)
    print(f"{fault} on {name} {variant} {kind}: worst row {ratio:.1f} x the bar")
    assert ratio >= 5


@pytest.mark.parametrize("kind", W.WELCH_WINDOWS)
def test_error_on_the_incoherent_rows_passes_rel_max_and_fails_the_row_bar(mirror, kind):
    c = W.welch_case("k_split_ragged", "")
    good, ref = _welch_model(c, kind, mirror)
    loud = len(c["k"]) // 2
    assert int(np.argmax(ref.max(axis=0))) == loud
    bad = W.incoherent_rows_fault(good, loud)
    old, ratio = rel_max(bad, ref), float(row_rel(bad, ref).max()) / (2 * TOL_ROW)
    print(f"1e-3 on the incoherent rows, {kind}: rel_max {old:.2e} (old bar {W.OLD_BAR:.0e}), worst row {ratio:.0f} x the bar")
    assert old <= W.OLD_BAR
    assert ratio >= 5
