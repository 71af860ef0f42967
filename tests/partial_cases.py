"""Inputs, the NumPy twin and the bars of the pair passes of the partial spectra -- partial_power_kernel,
partial_shell_kernel (psa_amd/csrc/partial.hip), lattice_finish_kernel and the host loop around them (power_block:
sub-blocks of vectors and segments, the `first` flag, bins that straddle a block) -- shared by the host proof
(tests/test_partial_host.py) and the GPU suite (tests/test_gpu_partial.py).  Seeded, NumPy only.  The float64 reference is
tests/partial64.py; the float32 helpers, the families of currents and the Gaussian-integer cells are those of
tests/power_cases.py.

The twin (pair_model) restates the kernels' arithmetic in float32, operation by operation, and the host loop in its order;
fused=True forms every a * b + c with one rounding, as the compiler's contraction does.  fault= plants one mistake
(FAULTS); the host proof shows that each breaks an exact item or a bar.

Exact items.  Gaussian-integer cells (power_cases.gaussian_cells: re = 1 + i mod 512 > 0 > im = -(1 + i div 512), all
distinct), k along an axis or zero, every scale a power of two.  With at most 2^15 cells |im| <= 2^6, a product of two cells
stays below 2^18 + 2^12, the float32 sums (3 components x 4 segments) below 2^23: exact with or without contraction; the
shell pass adds them in float64 (exact) and rounds once.  So the float64 reference rounded once to float32 is the only
right answer, bit for bit, for every cutting.

Bars on random inputs, none measured from the kernels.  u = 2^-24, g(n) = n u / (1 - n u); "ref" and the fields D, LAM, A,
PP, M are partial64's on the same float32 inputs.  A cross term has no lower bound of its own (F^b = i F^a gives 0), so no
bar is relative to the value: each is relative to a sum of products of the two species' moduli.  bs: most segments of a
sub-block, nblk: sub-blocks of segments (the per-vector form adds a later block's result in float32: one rounding each,
of a partial sum that is at most the sum of its terms' moduli).
  density       the term fl(ar br + ai bi): 2 roundings on the longest path, |ar br| + |ai bi| <= |F^a_0| |F^b_0|;
                the chain over a block's segments bs - 1 more; the scale 1; later blocks nblk - 1:
                    per-vector  |got - ref| <= g(bs + nblk + 1) scale D          shell  g(3) scale D
                (shell: the term's 2 roundings, float64 sums, the finish pass's rounding)
  longitudinal  pr^a = sum_c h_c Re F^a_c with h the float32 rounding of k / |k|: |pr^a - pr64^a| <= g(4) Sx^a, Sx^a =
                sum_c |h_c| |Re F^a_c| (power_cases), and |pr64^a| <= Sx^a; so |pr^a pr^b - pr64^a pr64^b| <= (2 g(4) + g(4)^2)
                Sx^a Sx^b <= g(8) Sx^a Sx^b; fl(pr^a pr^b + pi^a pi^b) adds 2 roundings: g(10) (Sx^a Sx^b + Sy^a Sy^b) <=
                g(10) sqrt(Sx^a^2 + Sy^a^2) sqrt(Sx^b^2 + Sy^b^2) <= g(10) (sum_c |h_c| |F^a_c|) (sum_c |h_c| |F^b_c|) = g(10) LAM_s:
                    per-vector  g(bs + nblk + 9) scale LAM                        shell  g(11) scale LAM
  transverse    t^a_c = fl(F^a_c - h_c (pr^a, pi^a)) is off from F^a_perp,c by a vector d^a, ||d^a|| <= 6 u ||F^a|| + u ||F^a_perp||
                (power_cases: the projection's g(4), the rounding of h_c, the product, the subtraction).  Then
                    |sum_c Re t^a_c conj t^b_c - sum_c Re F^a_perp,c conj F^b_perp,c| <= ||d^a|| ||F^b_perp|| + ||F^a_perp|| ||d^b|| + ||d^a|| ||d^b||
                        <= 6 u M_s + 2 u PP_s + 49 u^2 A_s                        (||F_perp|| <= ||F||)
                The six products and their sum carry n roundings on the longest path, relative to sum_c |t^a_c| |t^b_c| <=
                ||t^a|| ||t^b||: n u PP_s more.  transverse = scale / 2 times the sum:
                    |got - ref| <= scale (u (3.01 M + ((2 + n) / 2 + 0.01) PP) + 25 u^2 A)
                (0.01 and the rounding up of 49 / 2 hold the products of first-order terms, n u <= 2^-18)
                    per-vector  n = 4 (a term: 2 for a component's pair of products, 2 for the sum over components) + (bs - 1)
                                    + 1 (the scale; the half is exact) + (nblk - 1) = bs + nblk + 3
                    shell       n = 4 + 1 (the finish pass) = 5
                For a = b this is power_cases' bar with M = 2 sqrt(A P): 12 u sqrt(A P) + ...; and transverse_aa >= 0.
  Every bar is widened by (1 + 2^-20) for the float64 sums of the shell form and of the reference.
The difference form 0.5 (sum_c Re F^a_c conj F^b_c - longitudinal) is off by about 3 u A whatever PP: fault "diff_transverse".
"""
import numpy as np

import partial64 as R
import power_cases as P
from power_cases import U, WIDEN, _cuts, _fma, bits, fraction, g  # noqa: F401  (bits, fraction: for the tests)

B_TR = 25.0
ROWS = ("density", "longitudinal", "transverse")
FAULTS = (
    "conj_dropped",        # the second factor not conjugated: ar br - ai bi
    "pair_map",            # a pair whose species are two apart reads the species in between: (0, 2) reads species 1
    "species_stride",      # a vector's series taken NC apart instead of S NC
    "mirror_one_factor",   # the partner's term with the first factor mirrored and the second not
    "mirror_no_zero",      # the mirror taken at L - o without the o = 0 case
    "mirror_dropped",
    "offdiag_doubled",     # a != b counted twice
    "khat_neighbour",      # the k / |k| row of the next vector
    "diff_transverse",     # 0.5 (all - lon) in place of the perpendicular form
    "bin_clip",            # max(bin_start, g0) dropped
)
SHELL_ONLY = ("mirror_one_factor", "mirror_no_zero", "mirror_dropped", "bin_clip")


def n_pairs(S):
    return S * (S + 1) // 2


# ---- the twin -------------------------------------------------------------------------------------------------------------
def _dot2(x, y, fused):
    """fl(x.re y.re + x.im y.im)"""
    return _fma(x[0], y[0], x[1] * y[1], fused)


def _pair_terms(fa, fb, h, fused, fault):
    """fa, fb: per component (re, im) of the two factors (NC entries each), h: three float32 -> (den, lon, tra) of one
    (segment, side) as pair_terms of partial.hip forms them"""
    if fault == "conj_dropped":
        fb = [(re, -im) for re, im in fb]
    den = _dot2(fa[0], fb[0], fused)
    if len(fa) == 1:
        return den, None, None
    zero = np.zeros_like(den)
    pa, pb = [zero, zero], [zero, zero]
    for c in range(3):
        for p, f in ((pa, fa), (pb, fb)):
            p[0], p[1] = _fma(h[c], f[1 + c][0], p[0], fused), _fma(h[c], f[1 + c][1], p[1], fused)
    lon = _dot2(pa, pb, fused)
    tra = zero
    for c in range(3):
        if fault == "diff_transverse":
            tra = tra + _dot2(fa[1 + c], fb[1 + c], fused)                  # `all`: the caller subtracts
            continue
        ta = (_fma(-h[c], pa[0], fa[1 + c][0], fused), _fma(-h[c], pa[1], fa[1 + c][1], fused))
        tb = (_fma(-h[c], pb[0], fb[1 + c][0], fused), _fma(-h[c], pb[1], fb[1 + c][1], fused))
        tra = tra + _dot2(ta, tb, fused)
    return den, lon, (tra - lon if fault == "diff_transverse" else tra)


def _reader(block, S, NC, fault):
    """block (nb, S, NC, ns, L) of one upload -> read(k, species (P,), component, s, idx) -> (re, im) float32 (.., P, L); flat
    addresses, clipped, so that a wrong stride reads some other cell and never past the upload"""
    nb, _, _, ns, L = block.shape
    flat = np.ascontiguousarray(block).reshape(-1)
    per_k = NC if fault == "species_stride" else S * NC

    def read(k, sp, c, s, idx):
        row = np.asarray(k)[..., None, None] * per_k + (np.asarray(sp) * NC + c)[:, None]
        v = flat[np.minimum((row * ns + s) * L + idx, flat.size - 1)]
        return np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)
    return read


def _species_of_pairs(S, fault):
    pr = R.pairs(S)
    a, b = pr[:, 0].copy(), pr[:, 1].copy()
    if fault == "pair_map":
        b = np.where(b - a >= 2, b - 1, b)
    return a, b


def pair_model(seg, khat, norm, bin_of=None, n_bins=0, k_block=0, seg_block=0, fused=False, fault=None):
    """seg (K, S, NC, ns, L) complex64, khat (K, 3) float32.  bin_of None: partial_power_kernel under power_block ->
    (1 or 3, P, L, K) float32; else partial_shell_kernel under power_block, then lattice_finish_kernel -> (1 or 3, P, L, n_bins)"""
    K, S, NC, n_seg, L = seg.shape
    NP, rows = n_pairs(S), 3 if NC == 4 else 1
    sa, sb = _species_of_pairs(S, fault)
    twice = np.where((sa != sb) & (fault == "offdiag_doubled"), 2.0, 1.0).astype(np.float32)[:, None]
    h_all = np.asarray(khat, np.float32).reshape(K, 3)
    o = np.arange(L)
    half = np.float32(0.5)

    def terms(read, k, h, s, ia, ib):
        fa = [read(k, sa, c, s, ia) for c in range(NC)]
        fb = [read(k, sb, c, s, ib) for c in range(NC)]
        return _pair_terms(fa, fb, h, fused, fault)

    if bin_of is None:
        scale = np.float32(1.0 / float(norm))
        out = np.full((rows, NP, L, K), np.nan, np.float32)
        for k1, nb in _cuts(K, k_block):
            kk = np.arange(nb)
            hk = h_all[np.minimum(k1 + kk + 1, K - 1)] if fault == "khat_neighbour" else h_all[k1 + kk]
            h = [hk[:, c][:, None, None] for c in range(3)]
            for s0, ns in _cuts(n_seg, seg_block):
                read = _reader(seg[k1:k1 + nb, :, :, s0:s0 + ns], S, NC, fault)
                acc = [np.zeros((nb, NP, L), np.float32) for _ in range(rows)]
                for s in range(ns):
                    for r, t in enumerate(terms(read, kk, h, s, o, o)[:rows]):
                        acc[r] = acc[r] + t
                new = [acc[0] * scale] + ([acc[1] * scale, half * (acc[2] * scale)] if NC == 4 else [])
                for r, v in enumerate(new):
                    v = np.moveaxis(v * twice[None], 0, 2)                 # (P, L, nb)
                    out[r, :, :, k1:k1 + nb] = v if s0 == 0 else out[r, :, :, k1:k1 + nb] + v
        return out

    bins = np.asarray(bin_of, np.int64)
    count = np.bincount(bins, minlength=n_bins)
    start = np.concatenate([[0], np.cumsum(count)])
    scale = np.divide(1.0, 2.0 * count * float(norm), out=np.zeros(n_bins), where=count > 0)
    acc = np.zeros((rows, NP, L, n_bins))
    om = L - o if fault == "mirror_no_zero" else (L - o) % L
    for g0, nb in _cuts(K, k_block):
        for s0, ns in _cuts(n_seg, seg_block):
            read = _reader(seg[g0:g0 + nb, :, :, s0:s0 + ns], S, NC, fault)
            for b in np.unique(bins[g0:g0 + nb]):
                k_lo = (start[b] if fault == "bin_clip" else max(start[b], g0)) - g0
                k_hi = min(start[b + 1], g0 + nb) - g0
                tot = np.zeros((rows, NP, L))
                for k in range(k_lo, k_hi):
                    k = max(k, 0)                                          # (a row before the block: some other vector's)
                    hk = h_all[min(g0 + k + 1, K - 1) if fault == "khat_neighbour" else g0 + k]
                    for s in range(ns):
                        for side in (0,) if fault == "mirror_dropped" else (0, 1):
                            ia = om if side else o
                            ib = o if side and fault == "mirror_one_factor" else ia
                            d, l, t = terms(read, k, hk, s, ia, ib)
                            tot[0] += d * twice
                            if NC == 4:
                                tot[1] += l * twice
                                tot[2] += (half * t) * twice
                acc[:, :, :, b] += tot
    return (acc * scale).astype(np.float32)


# ---- bars -----------------------------------------------------------------------------------------------------------------
def _tr_bar(ref, scale, n):
    return WIDEN * scale * (U * (3.01 * ref["M"] + ((2 + n) / 2 + 0.01) * ref["PP"]) + B_TR * U * U * ref["A"])


def vector_bars(ref, n_seg, seg_block):
    """(1 or 3, P, L, K) bars of the per-vector form"""
    bs, nblk = P._blocks(n_seg, seg_block)
    bars = [WIDEN * g(bs + nblk + 1) * ref["scale"] * ref["D"]]
    if ref["A"] is not None:
        bars += [WIDEN * g(bs + nblk + 9) * ref["scale"] * ref["LAM"], _tr_bar(ref, ref["scale"], bs + nblk + 3)]
    return np.stack(bars)


def shell_bars(ref):
    bars = [WIDEN * g(3) * ref["scale"] * ref["D"]]
    if ref["A"] is not None:
        bars += [WIDEN * g(11) * ref["scale"] * ref["LAM"], _tr_bar(ref, ref["scale"], 5)]
    return np.stack(bars)


def worst(got, ref, bars):
    """per field: (fraction of the bar, index)"""
    return [fraction(got[r], ref["out"][r], bars[r]) for r in range(got.shape[0])]


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def species_segments(rng, k, S, NC, ns, L, families, relation=None):
    """(K, S, NC, ns, L) complex64: every species an independent draw of power_cases.current_segments on the same vectors (so a
    vector's family holds for all of its species); relation "i": species 1 = i x species 0, "neg": species 1 = - species 0 (both
    exact in float32)"""
    seg = np.stack([P.current_segments(rng, k, NC, ns, L, families) for _ in range(S)], axis=1)
    if relation == "i":
        seg[:, 1] = (1j * seg[:, 0].astype(np.complex128)).astype(np.complex64)
    elif relation == "neg":
        seg[:, 1] = -seg[:, 0]
    return seg


def _case(name, S, NC, ns, L, K=None, counts=None, k_block=0, seg_block=0, families=P.FAMILIES, relation=None):
    return dict(name=name, S=S, NC=NC, ns=ns, L=L, K=K, counts=counts, k_block=k_block, seg_block=seg_block, families=families,
                relation=relation)


# the grid-stride tails: the per-vector pass strides L beyond 64 x 256 lanes and its (vector, pair) units beyond 65535, the
# shell pass L beyond 1024 x 256 and its (bin, pair) units beyond 65535
VECTOR_CASES = [
    _case("S1_L1", 1, 4, 1, 1, K=3, families=("1e-2",)), _case("S1_density", 1, 1, 3, 63, K=4),
    _case("S2_L63", 2, 4, 1, 63, K=6), _case("S2_L64_ns3", 2, 4, 3, 64, K=6), _case("S2_density_L64", 2, 1, 3, 64, K=5),
    _case("S3_families", 3, 4, 3, 65, K=12), _case("S8_currents", 8, 4, 1, 33, K=6), _case("S8_density", 8, 1, 3, 17, K=3),
    _case("S2_L16385_tail", 2, 4, 1, 16385, K=1, families=("1e-4",)),
    _case("S8_units65556_tail", 8, 1, 1, 1, K=1821),
    _case("S3_cut_remainders", 3, 4, 7, 70, K=5, k_block=2, seg_block=3), _case("S2_cut_every_segment", 2, 4, 3, 33, K=6, k_block=4, seg_block=1),
    _case("S2_cut_density", 2, 1, 7, 65, K=5, k_block=3, seg_block=2),
    _case("S2_times_i", 2, 4, 3, 65, K=6, relation="i"), _case("S3_negated", 3, 4, 3, 33, K=6, seg_block=2, relation="neg"),
]
SHELL_CASES = [
    _case("S1_L1", 1, 1, 1, 1, counts=[1]), _case("S2_L63", 2, 4, 1, 63, counts=[2, 0, 3]),
    _case("S2_L64_ns3", 2, 4, 3, 64, counts=[6, 0, 6]), _case("S3_families", 3, 4, 3, 65, counts=[5, 7]),
    _case("S8_currents", 8, 4, 1, 33, counts=[0, 2, 4]), _case("S8_density", 8, 1, 3, 17, counts=[3]),
    _case("S2_L262145_tail", 2, 1, 1, 262145, counts=[1]),
    _case("S8_units65556_tail", 8, 1, 1, 1, counts=P._sparse_counts(1821, {0: 1, 3: 2, 1819: 1, 1820: 3})),
    _case("S3_straddle_two", 3, 4, 3, 33, counts=[0, 1, 2, 0, 4, 0], k_block=3, seg_block=2),
    _case("S2_straddle_three", 2, 4, 1, 33, counts=[0, 1, 2, 0, 4, 0], k_block=2),
    _case("S2_cut_density", 2, 1, 3, 65, counts=[2, 0, 5], k_block=3, seg_block=2),
    _case("S2_times_i", 2, 4, 3, 65, counts=[3, 3], relation="i"), _case("S3_negated", 3, 4, 3, 33, counts=[2, 4], k_block=4, relation="neg"),
]


def inputs(case):
    """(seg, k_vectors float32, khat float32, norm, bin_of or None, n_bins)"""
    shell = case["counts"] is not None
    rng = np.random.default_rng((3000 if shell else 0) + sum(map(ord, case["name"])))
    bin_of, n_bins = None, 0
    K = case["K"]
    if shell:
        counts = np.asarray(case["counts"], np.int64)
        bin_of, n_bins = np.repeat(np.arange(counts.size), counts).astype(np.int32), int(counts.size)
        K = bin_of.size
    k = P.family_vectors(rng, K, case["families"])
    seg = species_segments(rng, k, case["S"], case["NC"], case["ns"], case["L"], case["families"], case["relation"])
    return seg, k, P.khat32(k), float(case["ns"]) * 0.375 * float(case["L"]) ** 2, bin_of, n_bins


def reference(case, args):
    seg, k, _, norm, bin_of, n_bins = args
    if bin_of is None:
        ref = R.vector64(seg, k, norm)
        return ref, vector_bars(ref, case["ns"], case["seg_block"])
    ref = R.shell64(seg, k, bin_of, n_bins, norm)
    return ref, shell_bars(ref)


_REFERENCES = {}


def references():
    """kind ("vector", "shell") -> case name -> (case, inputs, float64 reference, bars); computed once and left unchanged"""
    if not _REFERENCES:
        for kind, cases in (("vector", VECTOR_CASES), ("shell", SHELL_CASES)):
            _REFERENCES[kind] = {}
            for c in cases:
                args = inputs(c)
                _REFERENCES[kind][c["name"]] = (c, args) + reference(c, args)
    return _REFERENCES


def run_model(c, args, fused=False, fault=None):
    seg, _, khat, norm, bin_of, n_bins = args
    return pair_model(seg, khat, norm, bin_of, n_bins, c["k_block"], c["seg_block"], fused, fault)


# exact items
EXACT_L = (64, 63)
VECTOR_CUTS = ((0, 0), (2, 3), (3, 1))                                     # (k_block, seg_block)
SHELL_CUTS = ((0, 0), (3, 3), (2, 1))                                      # bin 4 straddles two and three blocks
EXACT_S = 3


def exact_vector(L):
    """K = 5 (x, y, -z, 0, -x), S = 3, NC = 4, 4 segments; norm 2^14"""
    return P.gaussian_cells((5, EXACT_S, 4, 4, L)), P.axis_vectors(5), 2.0 ** 14


def exact_shell(L):
    """bins of 0, 1, 2, 0, 4, 0 vectors, S = 3, NC = 4, 4 segments; norm 2^14"""
    bin_of = np.repeat(np.arange(6), [0, 1, 2, 0, 4, 0]).astype(np.int32)
    return P.gaussian_cells((7, EXACT_S, 4, 4, L)), P.axis_vectors(7), bin_of, 6, 2.0 ** 14


# ---- a trajectory for the end-to-end tests ----------------------------------------------------------------------------------
def lagged_wave(n_atoms, n_frames, box, k0_index, bin0, lagging, lag, amp=1.5, seed=0, e_hat=(0.6, 0.0, 0.8)):
    """lattice_cases.travelling_wave with the atoms `lagging` behind the others by the phase `lag`: sites scattered over the
    box and displaced by u = A e cos(w0 t - k0.R - lag_a), so that the cross spectrum of the two sets carries the lag"""
    import lattice_cases
    rng = np.random.default_rng(seed)
    H = np.asarray(box, np.float32).astype(np.float64)
    sites = rng.uniform(0.0, 1.0, (n_atoms, 3)) @ H
    k0 = 2 * np.pi * (np.asarray(k0_index, np.float64) @ lattice_cases.inverse(box).T)
    w0 = 2 * np.pi * bin0 / n_frames
    e = np.asarray(e_hat, np.float64)
    behind = np.zeros(n_atoms)
    behind[np.asarray(lagging, int)] = lag
    ph = w0 * np.arange(n_frames)[:, None] - (sites @ k0 + behind)[None, :]
    pos = sites[None] + amp * np.cos(ph)[..., None] * e + 0.02 * rng.standard_normal((n_frames, n_atoms, 3))
    vel = -amp * w0 * np.sin(ph)[..., None] * e
    return pos.astype(np.float32), vel.astype(np.float32)
