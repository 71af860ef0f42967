"""Input families of the bond-order tests, the allowance of the per-atom X derived from the arithmetic stated at
psa_bond_order in include/psa_hip.h and from nothing in the code, and a NumPy twin of that arithmetic with the planted faults
the host test holds outside the allowance.

The allowance on X_l 2^-24 = n^2 q_l^2, u = 2^-24.  X_l 2^-24 = n + 2 sum_{b<c} t_l(b, c) 2^-24, and a pair's t_l 2^-24 differs
from P_l of the true cosine by three things.
  (1) The cosine.  angle_cases' tol_c without the rounding of the table's edge,
          tol_c = (|delta d_b| / r_b + |delta d_c| / r_c) (1 + 2^-10) + 8.5 u
      (the legs' errors, the 8.5 u of the float32 chain); the clamp only moves towards the true value.  |P_l'| <= l (l + 1) / 2
      on [-1, 1], so P_l moves by at most l (l + 1) / 2 tol_c.
  (2) The recurrence, rho_l.  The stated step P_{k+1} = fma(A_k, fl(cos P_k), -fl(B_k P_{k-1})) with A_k, B_k rounded once
      is the exact step plus a local error eta_k: the product cos P_k is rounded (u |P_k|), A_k carries u relative (u A_k
      |P_k|), the product B_k P_{k-1} is rounded and B_k carries u (2 u B_k |P_{k-1}|), the fma is rounded (u |P_{k+1}|):
          |eta_k| <= u M (2 A_k + 2 B_k + 1),   M = 1 + 2^-10 >= every |P_k| met (1 + rho, second order included)
      -- P_0 and P_1 are exact.  The recurrence is linear, so the error of P_l is exactly sum_j eta_{j-1} G(l, j; cos) with
      G(., j; c) the solution of the exact recurrence that starts G(j-1) = 0, G(j) = 1: a polynomial in c of degree l - j.
          rho_l = sum_{j=2..l} u M (2 A_{j-1} + 2 B_{j-1} + 1) max_{[-1,1]} |G(l, j; c)|
      the maximum taken in float64 on 20001 points and raised by 2 % (Markov: a polynomial of degree <= 10 moves by at
      most 100 max|G| 10^-4 between neighbours of that grid).  RHO tabulates it: 5.1 u at l = 2, 27 u at 4, 64 u at 6, 263 u at l = 12, a
      running bound, not a fit (for orientation: the twin's recurrence over 2 10^5 random cosines is off by up to 1.2, 7.4, 14.6
      and 41 u at l = 2, 4, 6, 12).
  (3) The rounding to an integer, 2^-25.
A centre's allowance is twice the sum over its pairs of l (l + 1) / 2 tol_c + rho_l + 2^-25 (plus 10^-9 for the float64
reference).  The clamp of X to [0, n^2 2^24] only moves towards the true value.  A centre with a LEG-BORDERLINE neighbour
(angle_cases' definition: |x - 1| within the tolerance of the pair chain) may have another shell in float32 and is
excluded from the per-atom comparison; every test first asserts that their share is at most 10^-3.  The tests hold X,
never q: the root amplifies without limit at q -> 0."""
import math

import numpy as np

import angle64 as A
import angle_cases as Q
import order64 as O
import pair64 as R
import pair_cases as P

U32 = 2.0 ** -24
SHIFT = 24
ONE = 1 << SHIFT
CAPACITY = A.CAPACITY
MAX_L = 12
EXCLUDED_CAP = 1e-3
FAMILIES = Q.FAMILIES
family = Q.family


def coefficients():
    """(A_k, B_k), k = 0 .. 12, float32 of the float64 quotients (the route uses 1 .. 11; 12: the fault that is off by one)"""
    k = np.arange(MAX_L + 1, dtype=np.float64)
    return ((2.0 * k + 1.0) / (k + 1.0)).astype(np.float32), (k / (k + 1.0)).astype(np.float32)


def _rho():
    a, b = (t.astype(np.float64) for t in coefficients())                  # (exact or rounded: the same to the 2 %)
    c = np.linspace(-1.0, 1.0, 20001)
    big = 1.0 + 2.0 ** -10
    rho = {1: 0.0}
    for l in range(2, MAX_L + 1):
        total = 0.0
        for j in range(2, l + 1):
            prev, cur = np.zeros_like(c), np.ones_like(c)                  # G(j - 1), G(j)
            for k in range(j, l):
                prev, cur = cur, a[k] * c * cur - b[k] * prev
            total += U32 * big * (2.0 * a[j - 1] + 2.0 * b[j - 1] + 1.0) * 1.02 * float(np.abs(cur).max())
        rho[l] = total
    return rho


RHO = _rho()                                                               # per l: what the recurrence itself may add to P_l


# ---- input families beside angle_cases' ---------------------------------------------------------------------------------
def fcc_block(n_frames=2):
    """256 atoms of fcc, a = 21.72 / 4, in the cubic box, frozen: 12 neighbours at a / sqrt 2 = 3.84 (the second shell: 5.43)"""
    a = float(np.float32(21.72)) / 4.0
    basis = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    cell = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 1, 3)
    pos = ((cell + basis[None]).reshape(-1, 3) * a).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(pos, (n_frames,) + pos.shape))


def bcc_block(n_frames=2):
    """128 atoms of bcc, a = 21.72 / 4: 8 neighbours at 4.70, 6 more at 5.43 (the third shell: 7.68)"""
    a = float(np.float32(21.72)) / 4.0
    basis = np.array([[0, 0, 0], [.5, .5, .5]])
    cell = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 1, 3)
    pos = ((cell + basis[None]).reshape(-1, 3) * a).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(pos, (n_frames,) + pos.shape))


def shell(name):
    """the legs of a known shell, unit length"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    even = lambda v: [list(np.roll(v, s)) for s in range(3)]                # noqa: E731
    signs = lambda v: [[x * sx, y * sy, z * sz] for x, y, z in v for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]   # noqa: E731
    sets = {
        "fcc": signs(even([1.0, 1.0, 0.0])),
        "hcp": [[1, 0, 0], [-1, 0, 0], [.5, 3 ** .5 / 2, 0], [-.5, 3 ** .5 / 2, 0], [.5, -3 ** .5 / 2, 0], [-.5, -3 ** .5 / 2, 0]]
               + [[x, y, z] for z in ((2.0 / 3.0) ** .5, -(2.0 / 3.0) ** .5) for x, y in ((0.0, 3 ** -.5), (.5, -.5 * 3 ** -.5), (-.5, -.5 * 3 ** -.5))],
        "bcc": signs([[1.0, 1.0, 1.0]]),
        "sc": signs(even([1.0, 0.0, 0.0])),
        "tetrahedron": [[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]],
        "icosahedron": signs(even([0.0, 1.0, g])),
    }
    v = np.unique(np.round(np.array(sets[name], np.float64), 12), axis=0)
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


# ---- the reference and its allowance --------------------------------------------------------------------------------------
def reference(positions, box, groups, r_cut, step, ls):
    """dict: `xq` (n_o, n_a, n_l) float64 = n^2 q_l^2 by tests/order64.py (NaN: left out), `n` (n_o, n_a), `why` (n_o, n_a)
    (0 counted, 1 truncated, 2 isolated, 3 undefined), `allowed` like xq, `excluded` (n_o, n_a) bool: a centre with a
    leg-borderline neighbour"""
    S = len(groups)
    xq, count, why = O.per_atom(positions, box, groups, r_cut, step, ls)
    allowed, excluded = np.zeros_like(xq), np.zeros(count.shape, bool)
    atoms, spec = A.species_of(groups)
    n = atoms.size
    if n == 0:
        return dict(xq=xq, n=count, why=why, allowed=allowed, excluded=excluded)
    rc = A.cutoffs(r_cut, S)
    e64 = P.sigma_error(positions, box)
    aH = np.abs(R.box64(box)[0])
    cut = rc[spec[:, None], spec[None, :]]
    off = ~np.eye(n, dtype=bool)
    slope = np.array([l * (l + 1) / 2.0 for l in ls])
    fixed = np.array([RHO[l] for l in ls]) + 2.0 ** -25
    for o, f in enumerate(range(0, np.shape(positions)[0], step)):
        e, d, r = A.frame_pairs(positions[f], box, atoms)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(cut > 0.0, r / cut, np.inf)
            tol = np.where(cut > 0.0, P.tolerance(e.reshape(-1, 3), d.reshape(-1, 3), r.ravel(), box, np.where(cut > 0.0, cut, 1.0).ravel(),
                                                  e64).reshape(n, n), 0.0)
        dd = (U32 + e64 + 3.0 * U32 * np.abs(e)) @ aH
        dd = np.sqrt((dd * dd).sum(axis=2))                                  # |delta d|_2 of every leg
        excluded[o] = ((np.abs(x - 1.0) <= tol) & off).any(axis=1)
        near = (r < cut) & off
        for a in np.flatnonzero(why[o] == 0):
            nb = np.flatnonzero(near[a])
            j, k = np.triu_indices(nb.size, 1)
            rel = dd[a, nb] / r[a, nb] if nb.size > 1 else np.zeros(nb.size)
            tol_c = (rel[j] + rel[k]) * (1.0 + 2.0 ** -10) + 8.5 * U32
            allowed[o, a] = 2.0 * (slope * tol_c.sum() + fixed * j.size) + 1e-9
    return dict(xq=xq, n=count, why=why, allowed=allowed, excluded=excluded)


def check(x, n, ref, what=""):
    """the route's x (n_o, n_a, n_l) int64 and n inside the allowance of `reference` at every centre that is not excluded, left
    out where the reference leaves out; prints the largest |delta X| 2^-24 per order as a share of its allowance"""
    x, keep = np.asarray(x, np.int64), ~ref["excluded"]
    if not np.array_equal(np.asarray(n)[keep], ref["n"][keep]):
        print(f"{what}: neighbour counts differ")
        return False
    out_ref = ref["why"] != 0
    if not np.array_equal((x[..., 0] < 0)[keep], out_ref[keep]) or np.any((x < 0) != (x[..., :1] < 0)):
        print(f"{what}: other centres left out")
        return False
    both = keep & ~out_ref
    delta = np.abs(x[both].astype(np.float64) / ONE - ref["xq"][both])
    share = (delta / ref["allowed"][both]).max(axis=0) if delta.size else np.zeros(x.shape[-1])
    print(f"{what}: {int(both.sum())} centres compared, {int(ref['excluded'].sum())} excluded; largest |dX| 2^-24 per order "
          f"{np.round(delta.max(axis=0) if delta.size else share, 9)} = {np.round(share, 4)} of the allowance")
    return bool(np.all(delta <= ref["allowed"][both]))


def excluded_share(ref):
    return float(ref["excluded"].sum()) / max(ref["excluded"].size, 1)


# ---- the bins ---------------------------------------------------------------------------------------------------------
def exact_bin(x, n, n_q):
    """the largest i in [0, n_q - 1] with i^2 n^2 2^24 <= x n_q^2, in Python integers"""
    return min(n_q - 1, math.isqrt(int(x) * n_q * n_q // (int(n) * int(n) * ONE)))


def histogram_of(x, n, sizes, n_q):
    """(hist (S, n_l, n_q), left out (S,)) int64 of the integer bin rule applied to x (n_o, n_a, n_l) and n (n_o, n_a)"""
    start = np.concatenate([[0], np.cumsum(sizes)])
    hist, out = np.zeros((len(sizes), x.shape[2], n_q), np.int64), np.zeros(len(sizes), np.int64)
    for s in range(len(sizes)):
        for o in range(x.shape[0]):
            for a in range(start[s], start[s + 1]):
                if x[o, a, 0] < 0:
                    out[s] += 1
                    continue
                for j in range(x.shape[2]):
                    hist[s, j, exact_bin(x[o, a, j], n[o, a], n_q)] += 1
    return hist, out


def edge_samples(n_q):
    """(x, n) around every edge of the bins for a few n: the least X of bin i, the one below it, 0 and n^2 2^24"""
    xs, ns = [], []
    for n in (1, 2, 3, 12, 13, 64):
        full = n * n * ONE
        for i in range(n_q + 1):
            least = -((-i * i * full) // (n_q * n_q))                       # ceil: the least X with i^2 n^2 2^24 <= X n_q^2
            for v in (least - 1, least, least + 1):
                if 0 <= v <= full:
                    xs.append(v), ns.append(n)
    return np.array(xs, np.int64), np.array(ns, np.int64)


def bins_model(x, n, n_q, fault=None):
    """the stated bin of x at n neighbours, by the kernel's bisection in int64.  Fault "float_root_bin": floor(n_q sqrt(q^2))
    in float32"""
    x, n = np.asarray(x, np.int64), np.asarray(n, np.int64)
    if fault == "float_root_bin":
        q = np.sqrt(x.astype(np.float32) / (n * n * ONE).astype(np.float32))
        return np.minimum((q * np.float32(n_q)).astype(np.int64), n_q - 1)
    n2, rhs = n * n * ONE, x * n_q * n_q
    left, right = np.zeros_like(x), np.full_like(x, n_q)
    while np.any(right - left > 1):
        mid = (left + right) >> 1
        go, live = mid * mid * n2 <= rhs, right - left > 1
        left, right = np.where(live & go, mid, left), np.where(live & ~go, mid, right)
    return left


# ---- a NumPy twin of the stated arithmetic, with the planted faults -----------------------------------------------------
FAULTS = ("no_n_term", "pairs_once", "divide_by_n", "l_off_by_one", "theta_not_cos", "first_64", "float_root_bin")


def legendre32(cos, l_max):
    """P_0 .. P_l_max of float32 cosines by the stated chain: list of float32 arrays"""
    a, b = coefficients()
    cos = np.asarray(cos, np.float32)
    p = [np.ones_like(cos), cos]
    for k in range(1, l_max):
        p.append(P._fma32(a[k], (cos * p[k]).astype(np.float32), -(b[k] * p[k - 1]).astype(np.float32)))
    return p


def model(positions, box, groups, r_cut, step, ls, n_q, fault=None):
    """(hist (S, n_l, n_q), truncated, isolated, undefined (S,), x (n_o, n_a, n_l), n (n_o, n_a)) int64 as the stated float32 and
    integer arithmetic gives them.  Faults: FAULTS"""
    S, n_l = len(groups), len(ls)
    rc = A.cutoffs(r_cut, S)
    atoms, spec = A.species_of(groups)
    n = atoms.size
    origins = range(0, np.shape(positions)[0], step)
    hist, left_out = np.zeros((S, n_l, n_q), np.int64), np.zeros((3, S), np.int64)
    x, count = np.full((len(origins), n, n_l), -1, np.int64), np.zeros((len(origins), n), np.int64)
    if n == 0:
        return hist, left_out[0], left_out[1], left_out[2], x, count
    c = P.fractions_model(positions, box)
    h = R.box64(box)[0].astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(rc > 0.0, 1.0 / rc, 0.0).astype(np.float32)[spec[:, None], spec[None, :]]
    orders = [l + 1 for l in ls] if fault == "l_off_by_one" else list(ls)
    for o, fr in enumerate(origins):
        f = c[fr][atoms]
        e = (f[None, :, :] - f[:, None, :]).astype(np.float32)
        e = e - np.rint(e)
        d = np.stack([P._fma32(e[..., 2], h[2, k], P._fma32(e[..., 1], h[1, k], e[..., 0] * h[0, k])) for k in range(3)], -1)
        r2 = P._fma32(d[..., 2], d[..., 2], P._fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
        near = (np.sqrt(r2) * inv < np.float32(1.0)) & (inv > 0) & ~np.eye(n, dtype=bool)
        for a in range(n):
            nb = np.flatnonzero(near[a])
            count[o, a] = nb.size
            if nb.size > CAPACITY:
                left_out[0, spec[a]] += 1
                if fault != "first_64":
                    continue
                nb = nb[:CAPACITY]
            if nb.size == 0:
                left_out[1, spec[a]] += 1
                continue
            m = nb.size
            j, k = np.triu_indices(m, 1)
            cos, bad = Q._cos32(d[a, nb[j]], d[a, nb[k]]) if j.size else (np.zeros(0, np.float32), np.zeros(0, bool))
            if bad.any():
                left_out[2, spec[a]] += 1
                continue
            if fault == "theta_not_cos":
                cos = np.arccos(cos).astype(np.float32)
            p = legendre32(cos, max(orders))
            for col, l in enumerate(orders):
                t = np.rint(p[l].astype(np.float64) * ONE).astype(np.int64).sum()
                total = (0 if fault == "no_n_term" else m * ONE) + (1 if fault == "pairs_once" else 2) * int(t)
                if fault == "divide_by_n":
                    total *= m
                x[o, a, col] = min(max(total, 0), m * m * ONE)
            bins = bins_model(x[o, a], np.full(n_l, m), n_q, fault)
            hist[spec[a], np.arange(n_l), bins] += 1
    return hist, left_out[0], left_out[1], left_out[2], x, count
