"""Inputs, the per-element bound and a float32 twin of the vibrational density of states (psa_vdos: vdos.hip,
api_vdos.hip), shared by the host proof (tests/test_vdos_envelope_host.py), the GPU suite
(tests/test_gpu_vdos_perelement.py) and the tightened bars of tests/test_gpu_vdos.py.  Seeded; NumPy and SciPy only (the
float32 mean of displacement mode comes from oracle/psa_oracle.py, which is NumPy too).  The float64 reference is
tests/vdos64.py.

The bound, per element D[o, g, c].  From the arithmetic the head of vdos.hip states, nothing from the code; u = 2^-24.
  One series.  y[tau] = win[tau] (w_a (x - m)) is formed in float32: the subtraction, the weight and the window are one
  rounding each, 3 u of the sample (the reference takes the float32 data, mean, weights and window as they are).  The
  transform X = FFT(y) / L is float32: an FFT's error is c log2(L) u in norm, ||dX|| <= c log2(L) u ||X||.  Both kinds of
  error reach bin o in two ways: a part that follows the bin's own value (a rounding that is the same on every sample
  scales the whole series; a twiddle factor's error multiplies whatever passes through it, and through the butterflies
  of a loud line that is the line) and a part spread over all bins alike, of the size the norm statement gives per bin,
        |dX_a[o]| <= eta (|X_a[o]| + rms_a),     rms_a^2 = (1/L) sum_o |X_a[o]|^2,     eta = (3 + C_FFT log2 L) u.
  The second part is a root-mean-square statement, not a worst case (the worst case of one bin is sqrt(L) rms_a, and no
  bin of any family below comes near it); the constant that makes it hold is C_FFT, and that cannot be derived for a
  library FFT (tests/spectral_cases.py says the same of rocFFT).  It is measured here with the twin below, SciPy's
  complex64 FFT, over every case the GPU file runs and set so that the twin uses at most half of the bound everywhere:
  the margin the spectral stage took.  It is not fitted to GPU output.
  Two series per transform.  Z = X_a + i X_b is linear in both, so dZ obeys the same statement with
  rms_Z^2 = rms_a^2 + rms_b^2, and (|Z[o]|^2 + |Z[L-o]|^2) / 2 = |X_a[o]|^2 + |X_b[o]|^2 carries it to the pair.
  The sum.  D = K sum_{s,a} |X|^2, K = 1 / (n_seg U); the computed one has |X + dX|^2 = |X|^2 + 2 Re(conj X dX) + |dX|^2.
  With R[g, c] = K sum_{s,a} rms_a^2 -- the row's two-sided Parseval total divided by L, taken from the float64
  reference -- Cauchy-Schwarz over the atoms and segments gives K sum |X| rms <= sqrt(D R), and Minkowski
  K sum (|X| + rms)^2 <= (sqrt D + sqrt R)^2:
        |dD| <= 2 eta (D + sqrt(D R)) + eta^2 (sqrt D + sqrt R)^2.
  The power, the chunk sums, the reduce, the fold and the scale are float64 (the squares of float32 values are exact
  there): non-negative terms, at most three roundings per row of a (group, component) -- the sum of the two squares, the
  row's addition, its chunk's addition -- and eight for the fold and the scale: gamma64(3 rows + 8) D, with
  gamma64(n) = n 2^-53 / (1 - n 2^-53) and rows = pairs of the group x segments.  (5e-11 D at the largest case here.)
  The result is rounded to float32 once: u (D + |dD|).  Together
        bound = (1 + u) (2 eta (D + sqrt(D R)) + eta^2 (sqrt D + sqrt R)^2 + gamma64(3 rows + 8) D) + u D.
  The scale is per (group, component) and per element: a quiet group answers for itself, a floor bin answers to
  sqrt(D R) and not to the peak.  Both first-order terms are needed: with sqrt(D R) alone the twin on a line coherent
  over all atoms at L = 1000 takes 0.83 of the bound (0.42 at L = 513) where noise, quiet groups and offsets take 0.08
  to 0.24 -- on the line bin D >> R and the error follows D; with both it takes 0.07.  An empty group has D = R = 0:
  exactly zero.

C_FFT = 1: one rounding per radix-2 level, the textbook unit.  The twin's worst ratio to the bound per family, over the
tables below (tests/test_vdos_envelope_host.py asserts <= 0.5 on every case):
    noise 0.110   line 0.287   quiet_group 0.050   quiet_first 0.051   quiet_atoms 0.046   quiet_mix 0.042
    offset 0.038   positions 0.049   mass 0.040   noise + mass 0.043   positions + mass 0.040
The two largest are where nothing averages: the line at L = 513 in a group of 5 atoms and two segments (0.287), and one
pair in one segment (noise 0.110, line 0.185).  With many atoms and segments the roundings add up like a random walk
while Cauchy-Schwarz lets them add up in step, and the twin stays near 0.05.  No smaller constant is taken: the bound is
the derived one, and half of it is left to an FFT that is not SciPy's.  The GPU's ratios are in
tests/test_gpu_vdos_perelement.py and DESIGN.md; eta was not changed after they were seen.

Families, float32, seeded per case: "noise" (unit normal); "line" (noise plus 2e3 / sqrt(L) cos(2 pi (L // 4) t / L) on
every atom and component: the bin's amplitude is 10^3 times the floor's, coherent over the atoms); "quiet_group" (a group
of 32 atoms and one of 18 at 2^-12 of it, both inside the first 64-atom tile; "quiet_first": the quiet one listed
first); "quiet_atoms" (every third atom of the second group, from its lowest, at 2^-10); "quiet_mix" (the first group at
2^-12 and every third atom of the second at 2^-10); "offset" (noise + 50); "positions" (displacement mode: sites in
[40, 50) with 0.05 of motion, the float32 mean of oracle.psa_oracle.mean_positions); "mass" (weights 1 and sqrt(207)).

The twin.  vdos_model32 restates the pass in float32 as the header states it: groups to sorted pairs, blocks of whole
32-pair tiles x segments under the work budget, the groups of a block and their clipped pair ranges, the gather with its
64-frame tiles, SciPy's complex64 FFT of z = y_a + i y_b, float64 power summed per chunk of a (group, component)'s rows,
the chunks added in order, the fold and the float32 cast.  fault= plants one mistake (FAULTS).

Not in the tables: segments of one frame (psa_set_segments refuses L < 2; L = 1 is the run without segments on T = 1).
"""
import math
from bisect import bisect_left, bisect_right

import numpy as np
import scipy.fft

from vdos64 import parseval_sum, segment_count, vdos64

U = 2.0 ** -24
U64 = 2.0 ** -53
C_IN = 3.0
C_FFT = 1.0
OLD_BAR = 1e-5                      # rel_max bar of tests/test_gpu_vdos.py
TILE_PAIRS = 32                     # VDOS_TILE_PAIRS
TILE_FRAMES = 64                    # VDOS_TT
POWER_BINS = 256                    # bins per workgroup of the power pass
DEFAULT_BUDGET = 1 << 30            # PSA_OPT_VDOS_WORK_BYTES
FAULTS = ("pair_leak", "tile_group", "power32", "nyquist_twice", "dc_half", "tail_window", "last_segments_lost",
          "mean_after_weight", "chunk_gap")


# ---- the bound ------------------------------------------------------------------------------------------------------
def eta(L):
    return (C_IN + C_FFT * math.log2(L)) * U


def gamma64(n):
    assert n * U64 < 2.0 ** -20
    return n * U64 / (1.0 - n * U64)


def bound(ref, L, rows):
    """(F, G, 3) float64 bound on |got - ref| of the float64 reference ref (F, G, 3); rows (G,): pairs x segments of
    each group"""
    D = np.asarray(ref, np.float64)
    R = (parseval_sum(D, L) / L)[None]
    e = eta(L)
    g64 = np.array([gamma64(3 * int(r) + 8) for r in rows])[None, :, None]
    first = 2 * e * (D + np.sqrt(D * R)) + e * e * (np.sqrt(D) + np.sqrt(R)) ** 2 + g64 * D
    return (1 + U) * first + U * D


def group_rows(N, groups, n_seg):
    return [((N if g is None else len(g)) + 1) // 2 * n_seg for g in groups]


def ratio(got, ref, bar):
    """(worst |got - ref| / bar, its index (o, g, c)): an element with bar 0 must equal the reference (else inf); nan
    counts as inf"""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0, 0.0, err / bar)
    f = np.where(np.isnan(f), np.inf, f)
    if f.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(f)), f.shape)
    return float(f[i]), tuple(int(x) for x in i)


def check(got, data, groups, window=None, L=None, H=None, weights=None, mean=None, ref=None):
    """worst ratio of got (F, G, 3) float32 to the bound against vdos64 of the same arguments (ref: that reference, if
    the caller has it); asserts shape, type and that the rows of empty groups are exactly zero"""
    T, N = data.shape[:2]
    L = T if L is None else L
    H = L if H is None else H
    ref = vdos64(data, groups, window=window, L=L, H=H, weights=weights, mean=mean) if ref is None else ref
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float32, (got.shape, got.dtype, ref.shape)
    for gi, g in enumerate(groups):
        if g is not None and len(g) == 0:
            assert not got[:, gi, :].any(), f"group {gi} is empty: its rows must be exactly zero"
    return ratio(got, ref, bound(ref, L, group_rows(N, groups, segment_count(T, L, H))))[0]


# ---- the float32 twin -----------------------------------------------------------------------------------------------
def plan_pairs(N, groups, fault=None):
    """(pairs (P, 2) with -1 for no second atom, pair offsets of the non-empty groups, their numbers in the caller's list)"""
    lists = [np.arange(N) if g is None else np.sort(np.asarray(g, np.int64)) for g in groups]
    kept = [gi for gi, a in enumerate(lists) if a.size]
    pairs, off = [], [0]
    for j, gi in enumerate(kept):
        a = lists[gi]
        if a.size & 1:
            nxt = lists[kept[j + 1]][0] if fault == "pair_leak" and j + 1 < len(kept) else -1
            a = np.concatenate([a, [nxt]])
        pairs.append(a.reshape(-1, 2))
        off.append(off[-1] + a.size // 2)
    return (np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)), off, kept


def block_shape(P, L, n_seg, budget):
    """(pairs per block, segments per block) under the work budget: whole 32-pair tiles x segments"""
    unit = TILE_PAIRS * 3 * L * 8
    units = budget // unit
    assert units >= 1, (budget, unit)
    n_tiles = -(-P // TILE_PAIRS)
    ns, tiles = n_seg, 1
    if units >= n_seg:
        tiles = min(n_tiles, units // n_seg, 65535)
    else:
        ns = units
    return min(P, tiles * TILE_PAIRS), ns


def chunk_count(L, ng, rows):
    n_ot = min(-(-L // POWER_BINS), 1 << 12)
    return max(1, min(64, -(-2048 // (n_ot * 3 * ng)), rows))


def _series(data, atoms, weights, mean, fault):
    """(T, n, 3) float32: w (x - m) of the listed atoms, zeros for atom -1"""
    a = np.maximum(atoms, 0)
    x = np.ascontiguousarray(data[:, a, :], np.float32)
    w = None if weights is None else np.asarray(weights, np.float32)[a][None, :, None]
    m = None if mean is None else np.asarray(mean, np.float32)[a][None]
    if fault == "mean_after_weight":
        if w is not None:
            x = w * x
        if m is not None:
            x = x - m
    else:
        if m is not None:
            x = x - m
        if w is not None:
            x = w * x
    assert x.dtype == np.float32
    x[:, atoms < 0, :] = 0
    return x


def _sum_rows(p, f32):
    """sum over axis 1 of p (3, n, L): float64, or in float32 one row after the other"""
    if not f32:
        return p.sum(axis=1)
    if p.shape[1] == 0:
        return np.zeros((3, p.shape[2]), np.float32)
    return np.cumsum(p, axis=1, dtype=np.float32)[:, -1]


def vdos_model32(data, groups, window=None, L=None, H=None, weights=None, mean=None, budget=DEFAULT_BUDGET, fault=None):
    """(L // 2 + 1, G, 3) float32 (the arguments of vdos64, and the work budget in bytes); fault: one of FAULTS
      pair_leak           an odd group's last pair takes the next group's first atom as its imaginary part
      tile_group          in a gather tile that holds pairs of two groups, the rows go to the group of its first pair
      power32             the power, the chunk sums and the accumulator are float32
      nyquist_twice       even L: the Nyquist bin, whose fold partner is itself, is counted again on top of the fold
      dc_half             bin 0 is taken once: the fold's partner L - 0 is left out
      tail_window         the window index restarts at each 64-frame tile
      last_segments_lost  a ragged last segment block is dropped
      mean_after_weight   w x - m
      chunk_gap           the last row of every chunk is skipped when the rows are not divisible by the chunks"""
    assert fault is None or fault in FAULTS, fault
    data = np.asarray(data)
    T, N = data.shape[:2]
    L = T if L is None else L
    H = L if H is None else H
    win = None if window is None else np.asarray(window, np.float32)
    n_seg, F = segment_count(T, L, H), L // 2 + 1
    seg_u = 1.0 if win is None else float(np.dot(win.astype(np.float64), win.astype(np.float64))) / L
    out = np.zeros((F, len(groups), 3), np.float32)
    pairs, off, group_of = plan_pairs(N, groups, fault)
    P, n_groups = len(pairs), len(group_of)
    if P == 0:
        return out
    Pb, ns = block_shape(P, L, n_seg, budget)
    f32 = fault == "power32"
    acc = np.zeros((n_groups, 3, L), np.float32 if f32 else np.float64)
    wt = None
    if win is not None:
        wt = win[np.arange(L) % TILE_FRAMES] if fault == "tail_window" else win
    pair_group = np.repeat(np.arange(n_groups), np.diff(off))
    for p0 in range(0, P, Pb):
        nb = min(Pb, P - p0)
        g_first = bisect_right(off, p0) - 1
        g_end = bisect_left(off, p0 + nb)
        ng = g_end - g_first
        owner = pair_group[p0:p0 + nb].copy()
        if fault == "tile_group":
            for t0 in range(0, nb, TILE_PAIRS):
                owner[t0:t0 + TILE_PAIRS] = owner[t0]
        ya = _series(data, pairs[p0:p0 + nb, 0], weights, mean, fault)
        yb = _series(data, pairs[p0:p0 + nb, 1], weights, mean, fault)
        for s0 in range(0, n_seg, ns):
            bs = min(ns, n_seg - s0)
            if fault == "last_segments_lost" and bs < ns:
                continue
            n_chunks = chunk_count(L, ng, nb * bs)
            # the work buffer (3, nb, bs, L): row (c, pair, segment), the window applied per part
            frames = (s0 + np.arange(bs))[:, None] * H + np.arange(L)[None, :]
            re, im = ya[frames], yb[frames]                                   # (bs, L, nb, 3)
            if wt is not None:
                re, im = wt[None, :, None, None] * re, wt[None, :, None, None] * im
            work = np.empty((3, nb, bs, L), np.complex64)
            work.real, work.imag = re.transpose(3, 2, 0, 1), im.transpose(3, 2, 0, 1)
            Z = scipy.fft.fft(work, axis=-1)
            assert Z.dtype == np.complex64
            if f32:
                power = Z.real * Z.real + Z.imag * Z.imag
            else:
                power = Z.real.astype(np.float64) ** 2 + Z.imag.astype(np.float64) ** 2
            for gl in range(ng):
                g = g_first + gl
                if fault == "tile_group":
                    mine = np.flatnonzero(owner == g)
                else:
                    mine = np.arange(max(off[g], p0) - p0, min(off[g + 1], p0 + nb) - p0)
                rows = power[:, mine].reshape(3, -1, L)
                n_rows = rows.shape[1]
                total = acc[g].copy()
                for ch in range(n_chunks):
                    r_begin, r_end = n_rows * ch // n_chunks, n_rows * (ch + 1) // n_chunks
                    if fault == "chunk_gap" and n_rows % n_chunks and r_end > r_begin:
                        r_end -= 1
                    total = total + _sum_rows(rows[:, r_begin:r_end], f32)
                acc[g] = total
    o = np.arange(F)
    fold = acc[:, :, o] + acc[:, :, (L - o) % L]
    if fault == "dc_half":
        fold[:, :, 0] = acc[:, :, 0]
    if fault == "nyquist_twice" and L % 2 == 0:
        fold[:, :, L // 2] += acc[:, :, L // 2]
    scale = 0.5 / (float(L) * float(L) * float(n_seg) * seg_u)
    res = (scale * fold.astype(np.float64)).astype(np.float32)
    for g in range(n_groups):
        out[:, group_of[g], :] = res[g].T
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------
def window(kind, L):
    """float32 (L,): boxcar, or the periodic Hann window in the arithmetic of scipy.signal.get_window("hann", L); the GPU
    suite hands the array itself to psa_amd.Segments"""
    if kind == "boxcar":
        return np.ones(L, np.float32)
    assert kind == "hann", kind
    return (0.5 + 0.5 * np.cos(np.linspace(-np.pi, np.pi, L + 1)[:L])).astype(np.float32)


BASE = dict(T=256, N=300, L=64, H=32, window="hann")
BASE_GROUPS = (tuple(range(0, 90, 2)), tuple(range(1, 223, 2)))               # 45 and 111 atoms: 23 + 56 pairs
QUIET_GROUPS = (tuple(range(0, 32)), tuple(range(32, 50)))                    # 32 loud atoms, 18 quiet: one 64-atom tile
UNIT = TILE_PAIRS * 3 * BASE["L"] * 8                                         # bytes of one tile x one segment at L = 64
FAMILIES = ("noise", "line", "quiet_group", "quiet_first", "quiet_atoms", "quiet_mix", "offset", "positions", "mass")


def case(name, family="noise", groups=BASE_GROUPS, budget=None, disp=False, mass=False, **shape):
    """one case: T, N, L, H (L None: no segments, one boxcar segment of all frames), window "hann" | "boxcar", groups (a
    tuple of atom tuples, None: all atoms as one group), budget (bytes, None: the default), disp, mass"""
    c = dict(BASE, name=name, family=family, groups=groups, budget=budget, disp=disp or family == "positions",
             mass=mass or family == "mass")
    c.update(shape)
    if c["L"] is None:
        c["H"] = c["window"] = None
    return c


def picked(N, sizes, seed):
    """disjoint groups of the given sizes from a seeded shuffle of the N atoms, each listed in the shuffle's order (unsorted)"""
    perm = np.random.default_rng(seed).permutation(N)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    assert cuts[-1] <= N
    return tuple(tuple(int(a) for a in perm[cuts[i]:cuts[i + 1]]) for i in range(len(sizes)))


def with_last(N, n, seed):
    """one unsorted group of n atoms that holds atom N - 1 (not in the first place unless n = 1)"""
    rest = [int(a) for a in np.random.default_rng(seed).permutation(N - 1)[:n - 1]]
    return (tuple(rest[:1] + [N - 1] + rest[1:]),)


def both(cases):
    """every case on "noise" and on "line" """
    return [dict(c, name=f"{c['name']}_{f}", family=f) for c in cases for f in ("noise", "line")]


ATOM_COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129)
ATOM_CASES = both([case(f"atoms{n}", groups=with_last(300, n, 40 + n)) for n in ATOM_COUNTS] +
                  [case("all_N299", groups=None, N=299), case("all_N300", groups=None)])

EIGHT_ODD = (5, 7, 9, 11, 13, 15, 17, 19)                                     # 3 .. 10 pairs: tile 0 holds seven groups
GROUP_SIZES = {"g1_1": (1, 1), "g3_62": (3, 62), "g63_2_64": (63, 2, 64), "empty_between": (5, 0, 7, 0, 0, 9),
               "empty_around": (0, 5, 0, 7, 0, 0, 9, 0), "eight_odd": EIGHT_ODD,
               "on_tile": (64, 40), "pair_before_tile": (62, 40), "pair_after_tile": (66, 40)}
GROUP_CASES = both([case(n, groups=picked(300, s, 60 + i)) for i, (n, s) in enumerate(GROUP_SIZES.items())])

SEGMENT_LENGTHS = (2, 3, 63, 64, 65, 100, 255, 256, 257, 513)                 # H = L
LENGTH_T = {257: 600, 513: 1100}
LENGTH_CASES = both([case(f"L{L}", L=L, H=L, T=LENGTH_T.get(L, 256)) for L in SEGMENT_LENGTHS] +
                    [case(f"whole_T{T}", L=None, T=T) for T in (1, 2, 100, 257)])

HOP_CASES = both([case("H1_T100", H=1, T=100), case("H21", H=21), case("H64", H=64), case("H80_gaps", H=80),
                  case("H192_two", H=192), case("H32_T250_rest", T=250)])

# budgets at the base shape (79 pairs = 3 tiles, 7 segments): (1 tile, 1 segment); (1 tile, 3 + 3 + 1 segments); (2 tiles,
# 7 segments) with a group boundary inside the first block, on the second block's first pair and on the first's last
BUDGET_CASES = both([case("one_unit", budget=UNIT), case("ns3_of_7", budget=3 * UNIT + 5),
                     case("two_tiles_inside", budget=14 * UNIT + 5),
                     case("two_tiles_first_pair", budget=14 * UNIT, groups=picked(300, (128, 30), 71)),
                     case("two_tiles_last_pair", budget=20 * UNIT, groups=picked(300, (126, 40), 72))])

# chunks of the power pass: 1; 21; 64 (loud group: 128 rows, two per chunk, quiet group: 72 rows); 29 at n_ot = 3 with groups
# of 6 .. 20 rows
CHUNK_CASES = both([case("chunks1", groups=picked(300, (2,), 81), T=64, H=64), case("chunks21", groups=picked(300, (5,), 82)),
                    case("chunks64", groups=QUIET_GROUPS, T=288),
                    case("chunks29_L513", groups=picked(300, EIGHT_ODD, 83), L=513, H=513, T=1100)])
CHUNK_COUNTS = {"chunks1": 1, "chunks21": 21, "chunks64": 64, "chunks29_L513": 29}

FAMILY_CASES = ([case(f"family_{f}", family=f, groups=QUIET_GROUPS if f in ("quiet_group", "quiet_first") else BASE_GROUPS)
                 for f in FAMILIES] +
                [case("chunks64_quiet_group", family="quiet_group", groups=QUIET_GROUPS, T=288),
                 # 150 pairs x 187 segments, one tile x one segment per block: 28050 rows added one after the other
                 case("many_rows_line", family="line", groups=None, T=250, H=1, budget=UNIT)])
MODE_CASES = [case(f"{'positions' if d else ''}{'_' if d and m else ''}{'mass' if m else ''}_{w}",
                   family="positions" if d else "noise", disp=d, mass=m, window=w)
              for d, m in ((True, False), (False, True), (True, True)) for w in ("boxcar", "hann")]
TABLES = {"atoms": ATOM_CASES, "groups": GROUP_CASES, "lengths": LENGTH_CASES, "hops": HOP_CASES, "budgets": BUDGET_CASES,
          "chunks": CHUNK_CASES, "families": FAMILY_CASES, "modes": MODE_CASES}
ALL_CASES = {c["name"]: c for table in TABLES.values() for c in table}
assert len(ALL_CASES) == sum(len(t) for t in TABLES.values())


def _sorted_group(c, gi):
    return np.sort(np.asarray(c["groups"][gi], np.int64))


def inputs(c):
    """dict(data (T, N, 3) float32, groups (list of int arrays, None: all atoms), window (L,) float32 or None, L, H,
    weights (N,) float32 or None, mean (N, 3) float32 or None, budget)"""
    T, N, L, fam = c["T"], c["N"], c["L"], c["family"]
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    x = rng.standard_normal((T, N, 3))
    Ls = T if L is None else L
    if fam == "line":
        x += (2e3 / math.sqrt(Ls)) * np.cos(2 * np.pi * ((Ls // 4) * np.arange(T) % Ls) / Ls)[:, None, None]
    elif fam in ("quiet_group", "quiet_first", "quiet_mix", "quiet_atoms"):
        if fam in ("quiet_group", "quiet_first"):
            x[:, _sorted_group(c, 1), :] *= 2.0 ** -12
        if fam == "quiet_mix":
            x[:, _sorted_group(c, 0), :] *= 2.0 ** -12
        if fam in ("quiet_atoms", "quiet_mix"):
            x[:, _sorted_group(c, 1)[::3], :] *= 2.0 ** -10
    elif fam == "offset":
        x += 50.0
    elif fam == "positions":
        x = (40.0 + 10.0 * rng.random((1, N, 3))) + 0.05 * x
    elif fam not in ("noise", "mass"):
        raise KeyError(fam)
    data = x.astype(np.float32)
    groups = [None] if c["groups"] is None else [np.asarray(g, np.int64) for g in c["groups"]]
    if fam == "quiet_first":
        groups = groups[::-1]
    mean = None
    if c["disp"]:
        from oracle import psa_oracle as O
        mean = O.mean_positions(data)
        assert mean.dtype == np.float32
    weights = np.where(np.arange(N) % 2 == 1, np.float32(np.sqrt(207.0)), np.float32(1.0)).astype(np.float32) if c["mass"] else None
    return dict(data=data, groups=groups, window=None if L is None else window(c["window"], L), L=L, H=c["H"], weights=weights,
                mean=mean, budget=DEFAULT_BUDGET if c["budget"] is None else c["budget"])


def model_args(inp):
    return dict(groups=inp["groups"], window=inp["window"], L=inp["L"], H=inp["H"], weights=inp["weights"], mean=inp["mean"])


_REFERENCES = {}


def reference(name):
    """(case, inputs, float64 reference (F, G, 3), bound (F, G, 3)) of a case of the tables: computed once, left unchanged"""
    if name not in _REFERENCES:
        c = ALL_CASES[name]
        inp = inputs(c)
        ref = vdos64(inp["data"], **model_args(inp))
        T, N = inp["data"].shape[:2]
        L = T if inp["L"] is None else inp["L"]
        n_seg = segment_count(T, L, L if inp["H"] is None else inp["H"])
        bar = bound(ref, L, group_rows(N, inp["groups"], n_seg))
        for a in (inp["data"], ref, bar):
            a.setflags(write=False)
        _REFERENCES[name] = (c, inp, ref, bar)
    return _REFERENCES[name]
