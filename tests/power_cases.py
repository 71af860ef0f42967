"""Inputs, NumPy twins and bars of the passes that follow the FFT in the dynamic, lattice and self spectra --
dynamic_power_kernel, lattice_shell_kernel, lattice_finish_kernel, self_power_kernel, self_reduce_kernel and the host loops
around them (sub-blocks of vectors and segments, the `first` flag, bins that straddle a block, atom chunks, the column map)
-- shared by the host proof (tests/test_power_host.py) and the GPU suite (tests/test_gpu_power.py).  Seeded, NumPy only.
The float64 references are in tests/power64.py.

The twins (dynamic_model, shell_model, self_model) restate each kernel's arithmetic in float32, operation by operation, and
the host loops in their order; fused=True forms every a * b + c with one rounding, as the compiler's contraction does.
fault= plants one mistake (FAULTS); the host proof shows that each breaks an exact item or a bar.

Exact items.  Gaussian-integer cells re = 1 + i mod 512, im = -(1 + i div 512), i the cell's flat number: |re|, |im| <= 2^9,
all distinct, re > 0 > im, so no cell is the conjugate or the negation of another.  k along an axis (k / |k| exactly a unit
vector) or zero, every scale a power of two.  |cell|^2 < 2^19; the float32 sums of the dynamic pass (3 components x 4
segments) stay below 2^23 and are exact with or without contraction; the shell and self passes add float32 terms below 2^21
in float64 (exact) and round once, to the float32 nearest the exact value.  So the float64 reference rounded once to
float32 is the only right answer, bit for bit.

Bars on random inputs, none measured from the kernels.  u = 2^-24, g(n) = n u / (1 - n u); "ref" is power64 on the same
float32 inputs.  bs: most segments of a sub-block, nblk: sub-blocks of segments (the per-vector form adds a later block's
result to the earlier ones' in float32: one rounding each).  No input is near the subnormal range.
  density (per-vector)   |F_0|^2 = fl(re^2 + im^2): every product carries at most 2 roundings; the chain over a block's
                         segments bs - 1 more; the scale 1; later blocks nblk - 1.  Non-negative terms:
                             |got - ref| <= g(bs + nblk + 1) ref
  density (shell), self  the term's 2 roundings, float64 sums, the finish pass's rounding:  g(3) ref
  longitudinal           pr = sum_c h_c Re F_c with h the float32 rounding of k / |k| (u), three products and two additions
                         (3 roundings on the longest path): |pr - pr64| <= g(4) Sx, Sx = sum_c |h_c| |Re F_c|, likewise pi, Sy.
                         |pr^2 - pr64^2| <= (2 g(4) + g(4)^2) Sx^2 <= g(8) Sx^2; fl(pr^2 + pi^2) adds 2 roundings:
                         g(10) (Sx^2 + Sy^2) <= g(10) LAM_s, LAM_s = (sum_c |h_c| |F_c|)^2 (triangle inequality).  Then the
                         chain, the scale and the blocks as above:
                             per-vector  |got - ref| <= g(bs + nblk + 9) scale LAM        shell  g(11) scale LAM
                         relative to LAM, not to the value: h.F cancels.
  transverse             t_c = fl(F_c - h_c (pr, pi)) per part.  Against F_perp of the reference the part is off by
                         d_c = |h_c| Sx (g(4) [pr] + u [h_c] + u [the product, not fused]) + u |t_c| [the subtraction]
                             <= 6 u |h_c| Sx + u |F_perp,c| (1 + ..)
                         so ||d|| <= 6 u sqrt(Sx^2 + Sy^2) + u sqrt(P_s) <= 6 u sqrt(A_s) + u sqrt(P_s)   (Cauchy-Schwarz,
                         |h| = 1), and  |sum t^2 - P_s| <= 2 sqrt(P_s) ||d|| + ||d||^2
                             <= 12 u sqrt(A_s P_s) + 2 u P_s + (36 + 12 + 1) u^2 A_s               (P_s <= A_s).
                         The squares and their sum are non-negative terms with n roundings on the longest path: n u P_s more.
                         sum_s sqrt(A_s P_s) <= sqrt(A P), P <= sqrt(A P), and transverse = scale / 2 times the sum:
                             |got - ref| <= scale (a u sqrt(A P) + b u^2 A) + u ref
                             a = (12 + 2 + n) / 2 + 0.01,  b = 49 / 2 -> 25
                         the last term is the rounding of the scale (the finish pass in the shell form); 0.01 and the
                         rounding up of b hold the products of first-order terms (n u <= 2^-18).
                             per-vector  n = 2 + (3 bs - 1) + (nblk - 1) = 3 bs + nblk      a = 7.01 + (3 bs + nblk) / 2
                             shell       n = 2 + 2 (three components of one term)           a = 9.01
                         A model of the arithmetic on 20 000 random directions needs a >= 2.5 and b >= 5.1; these are
                         above both.  And transverse >= 0 everywhere: it is a sum of squares.
  Every bar is widened by (1 + 2^-20) for the float64 sums of the shell and self forms and of the reference.
The difference 0.5 (|F|^2 - |h.F|^2) the kernels formed before is off by about 3 u A whatever P: it breaks the bar wherever
P << A, and goes negative (fault "parent_transverse").

Not covered: the stride tail of self_reduce_kernel, first reached at n_groups L > 2^24 (a 130 MB input).
"""
import numpy as np

import power64 as R

U = 2.0 ** -24
WIDEN = 1.0 + 2.0 ** -20
B_TR = 25.0
FAMILIES = ("long", "1e-4", "1e-2", "1", "trans", "k0")
FAULTS = {
    "mirror_no_zero": ("shell", "self"),      # the mirror taken at L - o without the o = 0 case
    "mirror_dropped": ("shell", "self"),
    "khat_neighbour": ("dynamic", "shell"),   # the k / |k| row of the next vector
    "swap_13": ("dynamic", "shell"),          # components 1 and 3 swapped
    "seg_stride": ("dynamic", "shell", "self"),   # the segment stride L + 1
    "bin_clip": ("shell",),                   # max(bin_start, g0) dropped
    "first_later": ("dynamic",),              # `first` true on a later segment block
    "chunk_twice": ("self",),                 # a chunk's last atom counted by the next chunk too
    "perm_ignored": ("self",),                # the column of a group taken as its number
    "parent_transverse": ("dynamic", "shell"),    # 0.5 (all - lon) in place of the perpendicular form
}


def g(n):
    assert n * U < 2.0 ** -18
    return n * U / (1.0 - n * U)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- float32 arithmetic ---------------------------------------------------------------------------------------------------
def _fma(a, b, c, fused):
    """a b + c in float32: one rounding (the product of two float32 is exact in float64) or two"""
    if fused:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def _sq2(x, y, fused):
    """fl(x x + y y)"""
    return _fma(x, x, y * y, fused)


def _current_terms(f, h, fused, fault):
    """f: three (re, im) pairs of float32 arrays, h: three float32 scalars or arrays -> (lon, tra) of one (segment, side):
    |h.F|^2 and sum_c |F_c - h_c (h.F)|^2 as the kernels form them"""
    if fault == "swap_13":
        f = [f[2], f[1], f[0]]
    zero = np.zeros_like(f[0][0])
    pr, pi = zero, zero
    for c in range(3):
        pr, pi = _fma(h[c], f[c][0], pr, fused), _fma(h[c], f[c][1], pi, fused)
    lon = _sq2(pr, pi, fused)
    tra = zero
    if fault == "parent_transverse":
        for c in range(3):
            tra = tra + _sq2(f[c][0], f[c][1], fused)
        return lon, tra                                                    # `all`: the caller subtracts
    for c in range(3):
        tx, ty = _fma(-h[c], pr, f[c][0], fused), _fma(-h[c], pi, f[c][1], fused)
        tra = tra + _sq2(tx, ty, fused)
    return lon, tra


def _rows(block, fault):
    """block (n, ns, L) complex64 of one upload -> a reader (row r, segment s, frequencies idx) -> (re, im) float32; idx may
    reach L (the element after the row's end) and the segment stride may be off by one: flat addresses, clipped"""
    n, ns, L = block.shape
    flat = np.ascontiguousarray(block).reshape(-1)
    stride = L + 1 if fault == "seg_stride" else L

    def read(r, s, idx):
        at = np.minimum((np.asarray(r)[..., None] * ns) * L + s * stride + idx, flat.size - 1)
        v = flat[at]
        return np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)
    return read


def _cuts(n, block):
    b = n if block == 0 else min(block, n)
    return [(i, min(b, n - i)) for i in range(0, n, b)]


# ---- the twins ------------------------------------------------------------------------------------------------------------
def khat32(k_vectors):
    return R.khat64(k_vectors).astype(np.float32)


def dynamic_model(seg, k_vectors, scale, k_block=0, seg_block=0, fused=False, fault=None):
    """dynamic_power_kernel under power_block: seg (K, NC, ns, L) -> (1 or 3, L, K) float32"""
    K, NC, n_seg, L = seg.shape
    h_all, scale = khat32(k_vectors), np.float32(scale)
    out = np.full((3 if NC == 4 else 1, L, K), np.nan, np.float32)
    o = np.arange(L)
    for k1, nb in _cuts(K, k_block):
        kk = np.arange(nb)
        hk = h_all[np.minimum(k1 + kk + 1, K - 1)] if fault == "khat_neighbour" else h_all[k1 + kk]
        h = [hk[:, c:c + 1] for c in range(3)]
        for s0, ns in _cuts(n_seg, seg_block):
            read = _rows(seg[k1:k1 + nb, :, s0:s0 + ns].reshape(nb * NC, ns, L), fault)
            den = lon = tra = np.zeros((nb, L), np.float32)
            for s in range(ns):
                den = den + _sq2(*read(kk * NC, s, o), fused)
                if NC == 4:
                    l, t = _current_terms([read(kk * NC + 1 + c, s, o) for c in range(3)], h, fused, fault)
                    lon, tra = lon + l, tra + t
            first = s0 == 0 or fault == "first_later"
            new = [den * scale]
            if NC == 4:
                new += [lon * scale, np.float32(0.5) * ((tra - lon if fault == "parent_transverse" else tra) * scale)]
            for r, v in enumerate(new):
                out[r, :, k1:k1 + nb] = v.T if first else out[r, :, k1:k1 + nb] + v.T
    return out


def shell_model(seg, k_vectors, bin_of, n_bins, norm, k_block=0, seg_block=0, fused=False, fault=None):
    """lattice_shell_kernel under power_block, then lattice_finish_kernel: (1 or 3, L, n_bins) float32"""
    K, NC, n_seg, L = seg.shape
    h_all = khat32(k_vectors)
    bins = np.asarray(bin_of, np.int64)
    count = np.bincount(bins, minlength=n_bins)
    start = np.concatenate([[0], np.cumsum(count)])
    scale = np.divide(1.0, 2.0 * count * float(norm) * 1.0 * 1.0 * 1.0, out=np.zeros(n_bins), where=count > 0)
    rows = 3 if NC == 4 else 1
    acc = np.zeros((rows, L, n_bins))
    o = np.arange(L)
    om = L - o if fault == "mirror_no_zero" else (L - o) % L
    for g0, nb in _cuts(K, k_block):
        for s0, ns in _cuts(n_seg, seg_block):
            read = _rows(seg[g0:g0 + nb, :, s0:s0 + ns].reshape(nb * NC, ns, L), fault)
            for b in np.unique(bins[g0:g0 + nb]):
                k_lo = (start[b] if fault == "bin_clip" else max(start[b], g0)) - g0
                k_hi = min(start[b + 1], g0 + nb) - g0
                tot = np.zeros((rows, L))
                for k in range(k_lo, k_hi):
                    k = max(k, 0)                                          # (a row before the block: some other vector's)
                    hk = h_all[min(g0 + k + 1, K - 1) if fault == "khat_neighbour" else g0 + k]
                    for s in range(ns):
                        for idx in (o,) if fault == "mirror_dropped" else (o, om):
                            tot[0] += _sq2(*read(k * NC, s, idx), fused)
                            if NC == 4:
                                l, t = _current_terms([read(k * NC + 1 + c, s, idx) for c in range(3)], hk, fused, fault)
                                tot[1] += l
                                tot[2] += np.float32(0.5) * (t - l if fault == "parent_transverse" else t)
                acc[:, :, b] += tot
    return (acc * scale).astype(np.float32)


def self_chunks(n_chunks, L, ng, na):
    """the chunk rule of the run (0) or the caller's number"""
    n_ot = min((L + 255) // 256, 1 << 12)
    return n_chunks if n_chunks else max(1, min(64, (2048 + n_ot * ng - 1) // (n_ot * ng), na))


def self_model(work, groups, cols, scale, mirror, n_chunks=0, atom_block=0, vec_block=0, seg_block=0, fused=False, fault=None):
    """self_power_kernel and self_reduce_kernel under self_power_run, then lattice_finish_kernel: (L, cols) float32"""
    n_atoms, n_vec, n_seg, L = work.shape
    grp = np.asarray(groups, np.int64).reshape(-1, 2)
    n_groups, starts = grp.shape[0] - 1, grp[:, 0]
    acc = np.zeros((L, cols))
    o = np.arange(L)
    om = L - o if fault == "mirror_no_zero" else (L - o) % L
    sides = (o, om) if mirror and fault != "mirror_dropped" else (o,)
    for a0, na in _cuts(n_atoms, atom_block):
        for v0, nv in _cuts(n_vec, vec_block):
            g_first = int(np.searchsorted(starts, v0, "right")) - 1
            ng = min(n_groups, int(np.searchsorted(starts, v0 + nv, "left"))) - g_first
            nc = self_chunks(n_chunks, L, ng, na)
            for s0, ns in _cuts(n_seg, seg_block):
                read = _rows(work[a0:a0 + na, v0:v0 + nv, s0:s0 + ns].reshape(na * nv, ns, L), fault)
                for gl in range(ng):
                    gi = g_first + gl
                    k_lo, k_hi = max(starts[gi], v0) - v0, min(starts[gi + 1], v0 + nv) - v0
                    col = gi % cols if fault == "perm_ignored" else grp[gi, 1]
                    total = acc[:, col].copy()
                    for ch in range(nc):
                        a_lo, a_hi = na * ch // nc, na * (ch + 1) // nc
                        if fault == "chunk_twice" and ch + 1 < nc:
                            a_hi = min(a_hi + 1, na)
                        part = np.zeros(L)
                        for k in range(k_lo, k_hi):
                            for a in range(a_lo, a_hi):
                                for s in range(ns):
                                    for idx in sides:
                                        part += _sq2(*read(a * nv + k, s, idx), fused)
                        total += part
                    acc[:, col] = total
    return (acc * np.asarray(scale, np.float64)[None, :]).astype(np.float32)


# ---- bars -----------------------------------------------------------------------------------------------------------------
def _blocks(n_seg, seg_block):
    bs = n_seg if seg_block == 0 else min(seg_block, n_seg)
    return bs, -(-n_seg // bs)


def _tr_bar(ref, scale, a):
    return WIDEN * (scale * (a * U * np.sqrt(ref["A"] * ref["P"]) + B_TR * U * U * ref["A"]) + U * ref["out"][2])


def dynamic_bars(ref, n_seg, seg_block):
    """(1 or 3, L, K) bars of the per-vector form"""
    bs, nblk = _blocks(n_seg, seg_block)
    bars = [WIDEN * g(bs + nblk + 1) * ref["out"][0]]
    if ref["A"] is not None:
        bars += [WIDEN * g(bs + nblk + 9) * ref["scale"] * ref["LAM"], _tr_bar(ref, ref["scale"], 7.01 + (3 * bs + nblk) / 2)]
    return np.stack(bars)


def shell_bars(ref):
    bars = [WIDEN * g(3) * ref["out"][0]]
    if ref["A"] is not None:
        bars += [WIDEN * g(11) * ref["scale"] * ref["LAM"], _tr_bar(ref, ref["scale"], 9.01)]
    return np.stack(bars)


def self_bars(ref_out):
    return WIDEN * g(3) * ref_out


def fraction(got, ref, bar):
    """(worst |got - ref| / bar, its index): an element with bar 0 must equal the reference (else inf); nan counts as inf"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0, 0.0, err / bar)
    f = np.where(np.isnan(f), np.inf, f)
    i = np.unravel_index(int(np.argmax(f)), f.shape)
    return float(f[i]), tuple(int(x) for x in i)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def gaussian_cells(shape, first=0):
    """complex64 cells that encode their own flat number: re = 1 + i mod 512, im = -(1 + i div 512)"""
    n = int(np.prod(shape))
    assert first + n <= 512 * 512
    i = first + np.arange(n)
    out = np.empty(n, np.complex64)
    out.real, out.imag = 1 + i % 512, -(1 + i // 512)
    return out.reshape(shape)


AXES = np.array([[2, 0, 0], [0, 0.5, 0], [0, 0, -3], [0, 0, 0], [-1, 0, 0], [0, 4, 0], [0, 0, 1], [0.25, 0, 0]], np.float32)


def axis_vectors(K):
    return np.ascontiguousarray(AXES[np.arange(K) % len(AXES)])


def random_directions(rng, K):
    k = rng.standard_normal((K, 3))
    return (k * rng.uniform(0.1, 9.0, (K, 1))).astype(np.float32)


def _normal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def current_segments(rng, k_vectors, NC, ns, L, families):
    """(K, NC, ns, L) complex64: per vector a magnitude 2^m, m in [-20, 20], per segment a factor 2^(j / 2), j in [-6, 6];
    the current of vector i is of family families[i mod len]: a longitudinal part along k / |k| and a transverse part of the
    given relative size ("long": none, "trans": no longitudinal part, "k0": the vector itself is set to zero by the caller)"""
    K = k_vectors.shape[0]
    h = R.khat64(k_vectors)
    mag = 2.0 ** rng.integers(-20, 21, K)
    pw = 2.0 ** (rng.integers(-6, 7, ns) / 2.0)
    amp = (mag[:, None, None] * pw[None, :, None])
    seg = np.empty((K, NC, ns, L), np.complex128)
    seg[:, 0] = _normal(rng, (K, ns, L)) * amp
    if NC == 4:
        for i in range(K):
            fam = families[i % len(families)]
            t1 = np.cross(h[i], rng.standard_normal(3)) if h[i].any() else np.array([1.0, 0, 0])
            t1 /= np.linalg.norm(t1)
            t2 = np.cross(h[i], t1) if h[i].any() else np.array([0, 1.0, 0])
            eps = {"long": 0.0, "1e-4": 1e-4, "1e-2": 1e-2, "1": 1.0, "trans": 1.0, "k0": 1.0}[fam]
            a_l = 0.0 if fam == "trans" else 1.0
            ax = h[i] if h[i].any() else np.array([0, 0, 1.0])
            f = (a_l * ax[:, None, None] * _normal(rng, (ns, L)) + eps * (t1[:, None, None] * _normal(rng, (ns, L)) +
                                                                          t2[:, None, None] * _normal(rng, (ns, L))))
            seg[i, 1:4] = f * amp[i][None]
    return seg.astype(np.complex64)


def family_vectors(rng, K, families):
    k = random_directions(rng, K)
    for i in range(K):
        if families[i % len(families)] == "k0":
            k[i] = 0
    return k


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _dyn(name, K, NC, ns, L, k_block=0, seg_block=0, families=FAMILIES):
    return dict(name=name, K=K, NC=NC, ns=ns, L=L, k_block=k_block, seg_block=seg_block, families=families)


DYNAMIC_CASES = [
    _dyn("L1", 1, 4, 1, 1, families=("1e-2",)), _dyn("L2", 1, 4, 1, 2, families=("long",)),
    _dyn("L255", 1, 1, 1, 255), _dyn("L256", 1, 4, 1, 256, families=("1e-4",)), _dyn("L257", 1, 4, 1, 257, families=("long",)),
    _dyn("L16385_tail", 1, 4, 1, 16385, families=("1e-4",)), _dyn("L16385_density", 1, 1, 1, 16385),
    _dyn("K65537_tail", 65537, 4, 1, 1), _dyn("K65537_density", 65537, 1, 1, 1),
    _dyn("families_ns2", 12, 4, 2, 257), _dyn("families_ns7", 6, 4, 7, 33),
    _dyn("cut_remainders", 5, 4, 7, 70, k_block=2, seg_block=3), _dyn("cut_every_segment", 6, 4, 7, 33, k_block=4, seg_block=1),
    _dyn("cut_density", 5, 1, 7, 70, k_block=3, seg_block=2),
]


def dynamic_inputs(case):
    rng = np.random.default_rng(sum(map(ord, case["name"])))
    k = family_vectors(rng, case["K"], case["families"])
    seg = current_segments(rng, k, case["NC"], case["ns"], case["L"], case["families"])
    scale = np.float32(1.0 / (case["L"] ** 2 * case["ns"] * 0.375))
    return seg, k, scale


def _shell(name, counts, NC, ns, L, k_block=0, seg_block=0, families=FAMILIES):
    return dict(name=name, counts=counts, NC=NC, ns=ns, L=L, k_block=k_block, seg_block=seg_block, families=families)


def _sparse_counts(n_bins, filled):
    c = np.zeros(n_bins, np.int64)
    for b, n in filled.items():
        c[b] = n
    return c


SHELL_CASES = [
    _shell("L1", [1], 1, 1, 1), _shell("L2", [1], 1, 1, 2), _shell("L257", [1], 1, 1, 257), _shell("L262145_tail", [1], 1, 1, 262145),
    _shell("L257_currents", [1], 4, 3, 257, families=("long",)),
    _shell("bins65537_tail", _sparse_counts(65537, {0: 1, 3: 2, 65535: 1, 65536: 3}), 4, 1, 1),
    _shell("finish_tail", _sparse_counts((1 << 20) + 5, {1: 2, 1 << 19: 1, (1 << 20) + 4: 1}), 1, 1, 1),
    _shell("straddle_two", [0, 1, 2, 0, 4, 0], 4, 3, 33, k_block=3, seg_block=2),
    _shell("straddle_three", [0, 1, 2, 0, 4, 0], 4, 1, 33, k_block=2),
    _shell("families", [6, 0, 6], 4, 3, 130), _shell("families_cut", [5, 7], 4, 3, 65, k_block=5, seg_block=1),
    _shell("density_cut", [2, 0, 5], 1, 3, 65, k_block=3, seg_block=2),
]


def shell_inputs(case):
    rng = np.random.default_rng(1000 + sum(map(ord, case["name"])))
    counts = np.asarray(case["counts"], np.int64)
    bin_of = np.repeat(np.arange(counts.size), counts).astype(np.int32)
    K = bin_of.size
    k = family_vectors(rng, K, case["families"])
    seg = current_segments(rng, k, case["NC"], case["ns"], case["L"], case["families"])
    norm = float(case["ns"]) * 0.375 * float(case["L"]) ** 2
    return seg, k, bin_of, int(counts.size), norm


def _self(name, na, counts, ns, L, mirror, n_chunks=0, atom_block=0, vec_block=0, seg_block=0):
    """counts: vectors per shell (mirror on) or the number of vectors as a one-element list (per-vector form, shuffled columns)"""
    return dict(name=name, na=na, counts=counts, ns=ns, L=L, mirror=mirror, n_chunks=n_chunks, atom_block=atom_block,
                vec_block=vec_block, seg_block=seg_block)


SELF_CASES = [
    _self("L1", 1, [1], 1, 1, True), _self("L257", 1, [1], 1, 257, True), _self("L257_plain", 1, [1], 1, 257, False),
    _self("L1048577_tail", 1, [1], 1, 1048577, True),
    _self("na1_rule", 1, [2, 0, 1], 2, 33, True), _self("na3_chunks2", 3, [2, 0, 1], 2, 33, True, n_chunks=2),
    _self("na3_chunks_na", 3, [3], 2, 33, False, n_chunks=3), _self("na64_chunk1", 64, [1, 2], 1, 9, True, n_chunks=1),
    _self("na65_rule", 65, [1, 2], 1, 9, True), _self("na65_chunks2_cut", 65, [3], 3, 9, False, n_chunks=2, atom_block=24, seg_block=2),
    _self("groups_straddle", 5, [0, 3, 4, 0, 1], 3, 33, True, n_chunks=2, atom_block=3, vec_block=2, seg_block=2),
    _self("permutation_cut", 5, [7], 3, 33, False, vec_block=3, atom_block=2, n_chunks=0),
]


def self_groups(case, rng):
    """(groups (n_groups + 1, 2), cols, scale (cols,), nv)"""
    counts = np.asarray(case["counts"], np.int64)
    norm = float(case["ns"]) * 0.375 * float(case["L"]) ** 2
    if case["mirror"]:
        first = np.concatenate([[0], np.cumsum(counts)])
        grp = np.stack([first, np.concatenate([np.arange(counts.size), [0]])], axis=1)
        scale = np.divide(1.0, 2.0 * counts * norm, out=np.zeros(counts.size), where=counts > 0)
        return grp.astype(np.int32), int(counts.size), scale, int(counts.sum())
    nv = int(counts[0])
    perm = rng.permutation(nv)
    if nv > 1 and np.array_equal(perm, np.arange(nv)):
        perm = perm[::-1].copy()
    grp = np.stack([np.arange(nv + 1), np.concatenate([perm, [0]])], axis=1)
    return grp.astype(np.int32), nv, np.full(nv, 1.0 / norm), nv


def self_inputs(case):
    rng = np.random.default_rng(2000 + sum(map(ord, case["name"])))
    grp, cols, scale, nv = self_groups(case, rng)
    na, ns, L = case["na"], case["ns"], case["L"]
    amp = 2.0 ** rng.integers(-20, 21, (na, nv, 1, 1)) * 2.0 ** (rng.integers(-6, 7, (1, 1, ns, 1)) / 2.0)
    work = (_normal(rng, (na, nv, ns, L)) * amp).astype(np.complex64)
    return work, grp, cols, scale


_REFERENCES = {}


def references():
    """kind -> case name -> (case, the entry's arguments, float64 reference, bars); computed once and left unchanged"""
    if not _REFERENCES:
        out = {"dynamic": {}, "shell": {}, "self": {}}
        for c in DYNAMIC_CASES:
            args = dynamic_inputs(c)
            ref = R.dynamic64(*args)
            out["dynamic"][c["name"]] = (c, args, ref, dynamic_bars(ref, c["ns"], c["seg_block"]))
        for c in SHELL_CASES:
            args = shell_inputs(c)
            ref = R.shell64(*args)
            out["shell"][c["name"]] = (c, args, ref, shell_bars(ref))
        for c in SELF_CASES:
            args = self_inputs(c)
            ref = R.self64(*args, c["mirror"])
            out["self"][c["name"]] = (c, args, dict(out=ref), self_bars(ref))
        _REFERENCES.update(out)
    return _REFERENCES


def worst(got, ref, bars):
    """per row of the result (the self form has one): (fraction of the bar, index)"""
    if got.ndim == 2:
        return [fraction(got, ref["out"], bars)]
    return [fraction(got[r], ref["out"][r], bars[r]) for r in range(got.shape[0])]


# exact items
def exact_dynamic(L):
    """K = 5 (x, y, -z, 0, -x), NC = 4, 4 segments; scale 2^-14; cut into (2 vectors, 3 segments) too"""
    seg = gaussian_cells((5, 4, 4, L))
    return seg, axis_vectors(5), np.float32(2.0 ** -14)


def exact_shell(L):
    """bins of 0, 1, 2, 0, 4, 0 vectors, NC = 4, 4 segments; norm 2^14"""
    counts = np.array([0, 1, 2, 0, 4, 0])
    bin_of = np.repeat(np.arange(6), counts).astype(np.int32)
    return gaussian_cells((7, 4, 4, L)), axis_vectors(7), bin_of, 6, 2.0 ** 14


def exact_self(L, mirror):
    """3 atoms, 5 vectors, 4 segments; shells of 1, 0, 4 vectors or five shuffled columns; scales powers of two"""
    work = gaussian_cells((3, 5, 4, L))
    if mirror:
        grp, cols, scale = np.array([[0, 0], [1, 1], [1, 2], [5, 0]], np.int32), 3, np.array([2.0 ** -15, 0.0, 2.0 ** -17])
    else:
        grp, cols = np.array([[0, 3], [1, 0], [2, 4], [3, 1], [4, 2], [5, 0]], np.int32), 5
        scale = 2.0 ** -np.arange(12.0, 17.0)
    return work, grp, cols, scale


EXACT_L = (64, 63)
DYNAMIC_CUTS = ((0, 0), (2, 3), (3, 1))                                    # (k_block, seg_block)
SHELL_CUTS = ((0, 0), (3, 3), (2, 1))                                      # bin 4 straddles two and three blocks
SELF_CUTS = (dict(), dict(n_chunks=2, atom_block=2, vec_block=2, seg_block=3), dict(n_chunks=3, vec_block=3, seg_block=1))
