"""Inputs, NumPy twins and bars of the spectral stage -- everything after the projection: the batched FFT, the kernels
of k2_epilogue.hip, the k map of folded (k, -k) lists, the Welch segment stage and the block-by-block complex result --
shared by the host proof (tests/test_spectral_host.py) and the GPU suite (tests/test_gpu_spectral.py).  Seeded, NumPy and
SciPy only; the mirror flag of a k map is an argument (the tests take it from psa_amd._hip).

Crafted slabs.  craft_complex / craft_intensity fill a slab with values that encode their own position, all distinct,
every imaginary part negative (so no value is its own conjugate or the conjugate or negation of another one), plus a few
cells with +0.0, -0.0, a subnormal, FLT_MAX and +-inf in one of their parts.  finalize_model / transpose_model are the
exact twins of scale_transpose_c64_kernel and transpose_f32_kernel: a permutation, a correctly rounded float32 division
of each part by T, a sign flip.  The GPU suite compares bits; fault= plants the mistakes the host proof shows to change
bits.

Bars, none of them measured from the kernels (u = 2^-24):
  exact items        bit equality, no tolerance.
  intensity_bar      sum_c |out|^2 of three complex64 values: six non-negative products and five additions.  No
                     cancellation, so every term carries at most (1 + u)^6 whatever the order and whether a product is
                     fused into its addition: relative error <= 6 u of the float64 sum of the same float32 values.  A
                     product below the normal range is rounded to a multiple of 2^-149 instead (absolute 2^-150 each, the
                     additions of such values are exact): + 6 * 2^-150.  Reference zero: exactly zero; reference beyond
                     FLT_MAX: inf.
  CHIRAL_BAR         the folded phase difference f(d), d = angle(z1) - angle(z2), is continuous, 2 pi-periodic and has
                     slope +-1 (the wrap's jump at +-pi folds to 0 on both sides), so an error of d is an error of f of
                     the same size and no element needs a mask.  In units of 2^-22 = ulp(pi):
                       two atan2f at the OpenCL limit of 6 ulp, |angle| <= pi                     12
                       a1 - a2, |.| <= 2 pi < 8: half an ulp of [4, 8)                             1
                       + PI, |.| <= 3 pi < 16: half an ulp of [8, 16)                              2
                       float32 PI - pi = 8.7e-8, three uses (+ PI, - PI, the fold)                 3 x 0.37
                       float32 TWO_PI - 2 pi = 1.7e-7 as the modulus of one wrap                   0.73
                       m + TWO_PI (negative remainder), result < 8                                 1
                       m - PI, |.| <= pi                                                           0.5
                       the fold PI - d, |.| <= pi / 2                                              0.25
                     fmodf is exact.  Sum 18.6 -> CHIRAL_BAR = 19 * 2^-22 rad = 4.5e-6.
  single_bin_bar     S_c = (1/T) sum_t q[c, t] e^(-2 pi i b t / T) with the sum in float64: an error of q[c, t] of at most
                     bound(form, n_g) B[c, t] (tests/dense_cases.py) passes the mean by the triangle inequality,
                     bound * mean_t B[c, t]; the float64 twiddles and sum add nothing visible, the final rounding to
                     float32 half an ulp of the component -- one ulp is allowed.
  end to end         the project's bars, imported by the tests from tests/test_gpu_dense_envelope.py: TOL (global
                     max-norm) and TOL_ROW (each k-row against its own maximum, ref64.row_rel), twice both for
                     intensities.  rocFFT's accuracy cannot be derived; tests/test_spectral_host.py shows that a float32
                     model of the whole stage (model of the projection split, SciPy's complex64 FFT, float32 epilogue)
                     uses at most half of each on every case below.
"""
import numpy as np
import scipy.fft

import dense_cases as D

U = 2.0 ** -24
FLT_MAX = np.finfo(np.float32).max
SUBNORMAL = np.float32(2.0 ** -140)
CHIRAL_BAR = 19 * 2.0 ** -22
OLD_BAR = 1e-5                                  # rel_max bar of tests/test_gpu_segments.py


# ---- crafted slabs --------------------------------------------------------------------------------------------------
_SPECIALS = [("re", 0.0), ("re", -0.0), ("re", SUBNORMAL), ("re", FLT_MAX), ("re", np.inf), ("re", -np.inf),
             ("im", SUBNORMAL), ("im", -FLT_MAX), ("im", np.inf), ("im", -np.inf)]


def _special_cells(n_cells):
    """flat cell numbers of the special values: spread over the slab, distinct; fewer in a slab too small for all"""
    n = min(len(_SPECIALS), n_cells // 2)
    step = max(1, n_cells // (n + 1)) if n else 1
    return [(1 + j) * step % n_cells for j in range(n)]


def craft_complex(rows, T, specials=True):
    """(rows, 3, T) complex64: cell number i = (row * 3 + c) * T + w -> (1 + i 2^-14) - i (2 + i 2^-14), exact in float32
    (i < 2^14).  Real parts in [1, 2), imaginary parts in (-4, -2]: no two values, conjugates or negations coincide."""
    n = rows * 3 * T
    assert n < 2 ** 14
    i = np.arange(n, dtype=np.float64)
    re, im = (1 + i * 2.0 ** -14).astype(np.float32), (-(2 + i * 2.0 ** -14)).astype(np.float32)
    if specials:
        for cell, (part, val) in zip(_special_cells(n), _SPECIALS):
            (re if part == "re" else im)[cell] = val
    out = np.empty(n, np.complex64)
    out.real, out.imag = re, im
    return out.reshape(rows, 3, T)


def craft_chiral(rows, T):
    """craft_complex with component pairs that are equal, opposite and zero (with both signs of zero): row % 4 = 1: c1 = c0;
    2: c1 = -c0; 3: c2 = (+-0, +-0), the signs running through all four combinations along w; 0: untouched"""
    s = craft_complex(rows, T)
    for r in range(rows):
        if r % 4 == 1:
            s[r, 1] = s[r, 0]
        elif r % 4 == 2:
            s[r, 1].real, s[r, 1].imag = -s[r, 0].real, -s[r, 0].imag
        elif r % 4 == 3:
            w = np.arange(T)
            s[r, 2].real = np.where(w % 2 == 0, 0.0, -0.0)
            s[r, 2].imag = np.where(w // 2 % 2 == 0, 0.0, -0.0)
    return s


def craft_intensity(rows, T):
    """(rows, T) float32: 1 + i 2^-14 at cell i = row * T + w, with +0.0, -0.0, a subnormal, FLT_MAX and inf in a few"""
    n = rows * T
    assert n < 2 ** 14
    v = (1 + np.arange(n, dtype=np.float64) * 2.0 ** -14).astype(np.float32)
    vals = [0.0, -0.0, SUBNORMAL, FLT_MAX, np.inf]
    m = min(len(vals), n // 2)
    for j in range(m):
        v[(1 + j) * max(1, n // (m + 1)) % n] = vals[j]
    return v.reshape(rows, T)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize % 4 == 0 else np.uint8)


# ---- k maps ---------------------------------------------------------------------------------------------------------
MAPS = ("none", "identity", "all_mirrored", "alternating", "twins", "permutation", "last_tile")


def k_map(name, rows, K_out, mirror):
    """uint32 (K_out,) k map (None for "none"): entry = slab row | mirror flag.  "none" and "identity" have K_out = rows."""
    mirror = np.uint32(mirror)
    col = np.arange(K_out)
    if name in ("none", "identity"):
        assert K_out == rows
        return None if name == "none" else col.astype(np.uint32)
    if name == "all_mirrored":
        src, flag = col % rows, np.ones(K_out, bool)
    elif name == "alternating":
        src, flag = col % rows, col % 2 == 1
    elif name == "twins":                                        # columns 2 r and 2 r + 1 from row r: plain, mirrored
        src, flag = (col // 2) % rows, col % 2 == 1
    elif name == "permutation":
        rng = np.random.default_rng(1000 * rows + K_out)
        src, flag = rng.permutation(col % rows), rng.random(K_out) < 0.5
    elif name == "last_tile":                                    # mirrored entries only in the last 16-column tile
        src, flag = col % rows, col >= (K_out - 1) // 16 * 16
    else:
        raise KeyError(name)
    return (src.astype(np.uint32) | np.where(flag, mirror, np.uint32(0))).astype(np.uint32)


EPILOGUE_T = [1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 129]
EPILOGUE_GEOM = [(1, 1), (8, 15), (8, 16), (9, 17), (16, 31), (16, 32), (17, 33), (25, 49)]
EPILOGUE_BASE = (65, 9, 17)


def epilogue_table():
    """[(T, rows, K_out, map name)]: one axis at a time around EPILOGUE_BASE -- T and the geometry each with a map that
    mirrors every other column and one that mirrors only the last tile, every map at the base -- then a few corners"""
    T0, r0, K0 = EPILOGUE_BASE
    out = []
    for name in ("alternating", "last_tile"):
        out += [(T, r0, K0, name) for T in EPILOGUE_T]
        out += [(T0, r, K, name) for r, K in EPILOGUE_GEOM if (r, K) != (r0, K0)]
    out += [(T0, r0, r0 if name in ("none", "identity") else K0, name) for name in MAPS if name not in ("alternating", "last_tile")]
    out += [(1, 1, 1, "none"), (1, 1, 1, "all_mirrored"), (129, 1, 1, "all_mirrored"), (2, 25, 49, "permutation"),
            (129, 25, 49, "twins"), (1, 16, 32, "all_mirrored"), (2, 8, 15, "twins"), (64, 17, 33, "permutation"),
            (3, 25, 25, "identity"), (100, 16, 31, "all_mirrored")]
    return out


def _entries(kmap, rows, mirror):
    if kmap is None:
        return np.arange(rows), np.zeros(rows, bool)
    kmap = np.asarray(kmap, np.uint32)
    return (kmap & ~np.uint32(mirror)).astype(np.int64), (kmap & np.uint32(mirror)) != 0


FINALIZE_FAULTS = ("mirror_T-1-w", "dc_to_T", "dc_in_place", "no_conj", "conj_plain", "drop_last_tile", "swap_in_tile",
                   "nyquist_not_conj")


def _mirror_index(T, fault):
    w = np.arange(T)
    if fault == "mirror_T-1-w":
        return T - 1 - w
    idx = (T - w) % T
    if fault == "dc_to_T":                       # T - 0 = T: one past the row, which is the next row's first value
        idx = T - w
    return idx


def finalize_model(slab, kmap, T, mirror, fault=None):
    """(T, K_out, 3) complex64, the exact twin of psa_sed_finalize on a complex slab (rows, 3, T):
    out[w, col, c] = slab[row, c, w] / T for a plain column, conj(slab[row, c, (T - w) % T] / T) for a mirrored one -- real
    and imaginary part divided separately in float32, the conjugation a sign flip.  fault: one of FINALIZE_FAULTS."""
    slab = np.ascontiguousarray(slab, np.complex64)
    rows = slab.shape[0]
    assert slab.shape == (rows, 3, T)
    src, flag = _entries(kmap, rows, mirror)
    K_out = len(src)
    flat = np.concatenate([slab.reshape(-1), np.zeros(1, np.complex64)])      # dc_to_T reads one value further
    re = np.zeros((T, K_out, 3), np.float32)
    im = np.zeros((T, K_out, 3), np.float32)
    n_t = np.float32(T)
    last_tile = (K_out - 1) // 16 * 16
    with np.errstate(all="ignore"):
        for col in range(K_out):
            if fault == "drop_last_tile" and col >= last_tile and K_out % 16:
                continue
            m = bool(flag[col])
            idx = _mirror_index(T, fault) if m else np.arange(T)
            for c in range(3):
                v = flat[(src[col] * 3 + c) * T + idx]
                x, y = v.real / n_t, v.imag / n_t
                conj = m
                if fault == "no_conj":
                    conj = False
                elif fault == "conj_plain":
                    conj = True
                if conj:
                    y = -y
                if fault == "dc_in_place" and m:                  # bin 0 passed on as it lies in the slab: not conjugated
                    y[0] = -y[0]
                if fault == "nyquist_not_conj" and m and T % 2 == 0:
                    y[T // 2] = -y[T // 2]
                re[:, col, c], im[:, col, c] = x, y
    if fault == "swap_in_tile" and K_out >= 2:                    # (entry 0, component 1) <-> (entry 1, component 0)
        for a in (re, im):
            t = a[:, 0, 1].copy()
            a[:, 0, 1] = a[:, 1, 0]
            a[:, 1, 0] = t
    out = np.empty((T, K_out, 3), np.complex64)
    out.real, out.imag = re, im
    return out


def transpose_model(rows_tw, kmap, mirror, fault=None):
    """(T, K_out) float32, the exact twin of psa_sed_finalize on an intensity slab (rows, T): out[w, col] = slab[row, w],
    or slab[row, (T - w) % T] for a mirrored column -- a permutation.  fault "unreversed": mirrored columns read forwards."""
    slab = np.ascontiguousarray(rows_tw, np.float32)
    rows, T = slab.shape
    src, flag = _entries(kmap, rows, mirror)
    out = np.empty((T, len(src)), np.float32)
    w = np.arange(T)
    for col in range(len(src)):
        out[:, col] = slab[src[col], (T - w) % T if flag[col] and fault != "unreversed" else w]
    return out


# ---- bars -----------------------------------------------------------------------------------------------------------
def intensity_ref64(out):
    """sum_c |out|^2 in float64 of the float32 values of out (T, K, 3) complex64"""
    o = np.asarray(out)
    with np.errstate(all="ignore"):
        return np.sum(o.real.astype(np.float64) ** 2 + o.imag.astype(np.float64) ** 2, axis=-1)


def intensity_check(got, out):
    """The worst |got - ref| / (6 u ref + 6 2^-150) over the elements of a float32 intensity (T, K) of out (T, K, 3)
    whose reference is finite, positive and representable; asserts the rest: zero stays zero, overflow is inf."""
    got, ref = np.asarray(got), intensity_ref64(out)
    assert got.shape == ref.shape and got.dtype == np.float32
    over = ref > float(FLT_MAX)                                   # (includes inf)
    assert np.all(np.isposinf(got[over])), "an element beyond FLT_MAX must be inf"
    zero = ref == 0
    assert not np.any(got[zero]), "an element whose reference is zero must be exactly zero"
    live = ~over & ~zero
    if not live.any():
        return 0.0
    assert np.all(np.isfinite(got[live]))
    err = np.abs(got[live].astype(np.float64) - ref[live])
    return float(np.max(err / (6 * U * ref[live] + 6 * 2.0 ** -150)))


def chiral_ref64(out, c1, c2):
    """the folded phase difference of components c1, c2 of out (T, K, 3) complex64, in float64 (option "C" of
    calculate_chiral_phase)"""
    o = np.asarray(out)
    a = [np.arctan2(o[..., c].imag.astype(np.float64), o[..., c].real.astype(np.float64)) for c in (c1, c2)]
    d = a[0] - a[1]
    d = np.mod(d + np.pi, 2 * np.pi) - np.pi
    return np.where(d > np.pi / 2, np.pi - d, np.where(d < -np.pi / 2, -np.pi - d, d))


def single_bin_ref64(q, b):
    """(3,) complex128: bin b of FFT_t(q) / T of q (3, T) complex128, as a plain DFT with the angle reduced in integers"""
    T = q.shape[-1]
    t = np.arange(T, dtype=np.int64)
    return q @ np.exp(-2j * np.pi * ((b * t) % T) / T) / T


def single_bin_bar(form, n_g, B, ref):
    """(3,) float64 bound on either part of component c: bound(form, n_g) mean_t B[c, t] + one float32 ulp of the
    component's larger part"""
    big = np.maximum(np.abs(ref.real), np.abs(ref.imag)).astype(np.float32)
    return D.bound(form, n_g) * B.mean(axis=1) + np.spacing(big).astype(np.float64)


# ---- the segment stage ----------------------------------------------------------------------------------------------
def segment_blocks_model(K_local, T, L, H):
    """Twin of segment_blocks() in api_project.hip: the segment buffer holds nk k-vectors x ns segments, never more
    than q (K_local, 3, T).  dict(n_seg, nk, ns, regime: "none" | "k" | "segments", k_blocks, s_blocks: the block sizes)"""
    n_seg = 1 + (T - L) // H
    units = max(1, K_local * T // L)
    if units >= n_seg:
        ns, nk = n_seg, max(1, min(K_local, units // n_seg))
    else:
        ns, nk = units, 1
    split = lambda n, b: [min(b, n - i) for i in range(0, n, b)]
    regime = "segments" if ns < n_seg else "k" if nk < K_local else "none"
    return dict(n_seg=n_seg, nk=nk, ns=ns, regime=regime, k_blocks=split(K_local, nk), s_blocks=split(n_seg, ns))


WELCH_FAULTS = ("overwrite", "drop_ragged", "norm_ns", "group_overwrite")


def welch_model32(q_groups, window, L, H, fault=None):
    """(K, L) float32 slab rows, a float32 restatement of segment_stage() with its blocks: per group, k block and segment
    block: window (one float32 product per part), complex64 FFT (SciPy), / L per part, the squares summed in float32 in
    the kernel's order, times inv_norm, written by the call's first block of a row and added by the later ones.
    q_groups: [(K, 3, T) complex]; fault: one of WELCH_FAULTS."""
    w = np.asarray(window, np.float32)
    K, _, T = q_groups[0].shape
    blk = segment_blocks_model(K, T, L, H)
    n_seg = blk["n_seg"]
    seg_U = float(np.dot(w.astype(np.float64), w.astype(np.float64))) / L
    acc = np.zeros((K, L), np.float32)
    n_l = np.float32(L)
    for gi, q in enumerate(q_groups):
        q = np.asarray(q).astype(np.complex64)
        first = gi == 0 or fault == "group_overwrite"
        s0 = 0
        for bs in blk["s_blocks"]:
            if fault == "drop_ragged" and bs < blk["ns"]:
                continue
            inv_norm = np.float32(1.0 / ((bs if fault == "norm_ns" else n_seg) * seg_U))
            s = np.zeros((K, L), np.float32)
            for sg in range(s0, s0 + bs):
                x = q[:, :, sg * H:sg * H + L]
                seg = np.empty_like(x)
                seg.real, seg.imag = w * x.real, w * x.imag
                F = scipy.fft.fft(seg, axis=-1)
                for c in range(3):
                    re, im = F[:, c].real / n_l, F[:, c].imag / n_l
                    s += re * re + im * im
            p = s * inv_norm
            acc = p if (first and s0 == 0) or (fault == "overwrite") else acc + p
            s0 += bs
    return acc


def incoherent_rows_fault(out, loud, rel=1e-3):
    """the planted fault of the per-row metric: every column of out (L, K) but the loud one is off by the relative error"""
    bad = np.array(out, np.float32)
    cols = np.arange(bad.shape[1]) != loud
    bad[:, cols] *= np.float32(1 + rel)
    return bad


# ---- a float32 model of the full-spectrum stage -----------------------------------------------------------------------
def q_model(c):
    """(K, 3, T) complex64 projection of a dense_cases case by the model of the split its k-list length is served by
    under the default options: "3 x bf16" up to 16 k-vectors, "2 x f16" above"""
    model = D.model_bf16 if len(c["k"]) <= 16 else D.model_f16
    return model(c).astype(np.complex64)


def spectrum32(q):
    """(T, K, 3) complex64: SciPy's complex64 FFT of q (K, 3, T) complex64 and the float32 division of each part by T"""
    T = q.shape[-1]
    F = scipy.fft.fft(np.ascontiguousarray(q, np.complex64), axis=-1)
    assert F.dtype == np.complex64
    out = np.empty((T, q.shape[0], 3), np.complex64)
    out.real, out.imag = (F.real / np.float32(T)).transpose(2, 0, 1), (F.imag / np.float32(T)).transpose(2, 0, 1)
    return out


def intensity32(spectra):
    """(T, K) float32: sum over the groups' spectra (T, K, 3) complex64 and the components of |.|^2, in float32"""
    acc = None
    for S in spectra:
        s = np.zeros(S.shape[:2], np.float32)
        for c in range(3):
            s += S[..., c].real * S[..., c].real + S[..., c].imag * S[..., c].imag
        acc = s if acc is None else acc + s
    return acc


def two_groups(n):
    return [np.arange(0, n, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)]


# ---- case tables of the end-to-end parts ------------------------------------------------------------------------------
FULL_T = [1, 2, 63, 64, 65, 96, 97, 127, 257]                    # at K = 40: powers of two, composites, primes
FULL_K = [15, 16, 17, 31, 32, 33]                                # at T = 96
FULL_FAMILIES = ("coherent", "quiet_frames")
FOLD_LISTS = ("pairs", "pairs_gamma", "pairs_twins", "last_tile")
FOLD_T = [64, 65, 97]
N_ATOMS = {"coherent": 4096, "quiet_frames": 1000}              # dense_cases' own sizes


def full_table():
    """[(family, K, T)] of the T axis and the K axis"""
    return [(f, 40, T) for f in FULL_FAMILIES for T in FULL_T] + [(f, K, 96) for f in FULL_FAMILIES for K in FULL_K if K != 40]


def full_case(family, K, T):
    return D.case(family, K=K, n=N_ATOMS[family], T=T)


def folded_list(name, base):
    """a k-list with (k, -k) pairs built from the vectors base (n, 3) and their exact negations"""
    n = len(base)
    if name == "pairs":
        k = np.concatenate([base, -base])
    elif name == "pairs_gamma":
        k = np.concatenate([base[:n // 2], -base, np.zeros((1, 3), np.float32), base[n // 2:]])
    elif name == "pairs_twins":                                  # k_3 and -k_5 twice more
        k = np.concatenate([base, base[3:4], -base, -base[5:6], base[3:4]])
    elif name == "last_tile":                                    # 32 plain columns = two whole tiles, 5 partners in the third
        k = np.concatenate([base, -base[:5]])
    else:
        raise KeyError(name)
    return np.ascontiguousarray(k, np.float32)


def folded_case(family, name, T):
    """the family's case (20 base vectors; last_tile: 32) with the folded list in place of its k-list.  The coherent
    family's loud row is base[n // 2], so it and its partner are both in the list."""
    c = D.case(family, K=32 if name == "last_tile" else 20, n=N_ATOMS[family], T=T)
    c["k"] = folded_list(name, c["k"])
    return c


def fold_table():
    return [(f, name, T) for f in FULL_FAMILIES for name in FOLD_LISTS for T in FOLD_T]


PIPELINE_BLOCKS = "16,16,40"                                     # of 100 rows: the remaining 28 are a fourth block


def pipeline_case(order):
    """quiet_frames with 100 vectors and their negations, K_out = 200 >= 192: the block-by-block path.  order "runs2": the
    negations in the vectors' order (two runs of columns per block, copied per block); "scattered": the negations in a
    seeded random order (a block's partners lie apart: one copy at the end).  The unique rows and their order are the
    same, so both project the same blocks.  Returns (case, column of every vector of "runs2" in this list)."""
    c = D.case("quiet_frames", K=100, n=N_ATOMS["quiet_frames"], T=96)
    base = c["k"]
    perm = np.arange(100) if order == "runs2" else np.random.default_rng(17).permutation(100)
    c["k"] = np.ascontiguousarray(np.concatenate([base, -base[perm]]), np.float32)
    where = np.concatenate([np.arange(100), 100 + np.argsort(perm)])
    return c, where


def pipeline_runs_model(kmap, blocks, mirror):
    """runs of consecutive output columns per block of slab rows, as calculate_pipelined() counts them (more than 8 in
    any block: one copy at the end)"""
    src, _ = _entries(kmap, 0, mirror)
    edges = np.concatenate([[0], np.cumsum(blocks)])
    runs = []
    for b in range(len(blocks)):
        cols = np.flatnonzero((src >= edges[b]) & (src < edges[b + 1]))
        runs.append(int(1 + np.sum(np.diff(cols) != 1)) if len(cols) else 0)
    return runs


# Welch: name -> (K of the base list, list kind, T, L, H, regime, ragged k block, ragged segment block, size of the last
# segment block); list kinds: "plain" (K random vectors), "kmg" (k, -k, Gamma: two rows after folding), "fold12" (K
# vectors and the negations of 12 of them, K rows after folding)
WELCH_SHAPES = {
    "no_split":        (24, "plain", 256, 64, 64, "none", False, False, 4),
    "k_split_ragged":  (24, "plain", 256, 64, 32, "k", True, False, 7),
    "seg_ragged":      (1, "kmg", 200, 64, 7, "segments", False, True, 2),
    "seg_even":        (1, "kmg", 200, 64, 8, "segments", False, False, 6),
    "seg_last_single": (24, "plain", 256, 64, 2, "segments", False, True, 1),
    "L_odd":           (24, "plain", 256, 63, 32, "k", True, False, 7),
    "L_prime":         (24, "plain", 256, 97, 40, "k", True, False, 4),
    "L_is_T":          (24, "plain", 256, 256, 256, "none", False, False, 1),
    "H_over_L":        (24, "plain", 256, 48, 80, "none", False, False, 3),
}
WELCH_VARIANTS = {"seg_ragged": ("groups",), "seg_even": ("groups",), "seg_last_single": ("groups", "fold12")}
WELCH_WINDOWS = ("boxcar", "hann")
WELCH_N = 1000


def welch_table():
    """[(shape name, variant: "" | "groups" | "fold12", window)]"""
    out = []
    for name in WELCH_SHAPES:
        for variant in ("",) + WELCH_VARIANTS.get(name, ()):
            out += [(name, variant, w) for w in WELCH_WINDOWS]
    return out


def window(kind, L):
    """float32 (L,): boxcar, or the periodic Hann window 0.5 - 0.5 cos(2 pi n / L) in the arithmetic of
    scipy.signal.get_window("hann", L).  The GPU suite hands the array itself to psa_amd.Segments."""
    if kind == "boxcar":
        return np.ones(L, np.float32)
    return (0.5 + 0.5 * np.cos(np.linspace(-np.pi, np.pi, L + 1)[:L])).astype(np.float32)


def welch_case(name, variant):
    """dict: the coherent family's case with the shape's list (k: the full, unfolded list), K_local (rows after folding),
    groups ([None] or two index arrays), T, L, H and the expected split"""
    Kb, kind, T, L, H, regime, k_rag, s_rag, last = WELCH_SHAPES[name]
    if variant == "fold12":
        kind = "fold12"
    c = D.case("coherent", K=max(Kb, 2), n=WELCH_N, T=T)
    base = c["k"]
    if kind == "kmg":                                            # the loud vector, its negation, Gamma
        loud = base[len(base) // 2]
        c["k"] = np.ascontiguousarray(np.stack([loud, -loud, np.zeros(3, np.float32)]), np.float32)
        K_local = 2
    elif kind == "fold12":
        c["k"] = np.ascontiguousarray(np.concatenate([base, -base[:12]]), np.float32)
        K_local = len(base)
    else:
        K_local = len(base)
    c.update(K_local=K_local, groups=two_groups(WELCH_N) if variant == "groups" else [None], L=L, H=H,
             expect=dict(regime=regime, k_ragged=k_rag, s_ragged=s_rag, last_s=last))
    return c
