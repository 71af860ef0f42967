"""Input families of the local-order tests, the allowances derived from the arithmetic stated at psa_local_order in
include/psa_hip.h and from nothing in the code, and a NumPy twin of that arithmetic with the planted faults the host test holds
outside the allowance.

The allowances.  v = Q 2^-40 = sum_b Yt_lm(d_b) is held as a vector over m in [-l, l] in the 2-norm.
  (1) Per leg.  sum_m |grad Yt_lm|^2 = l (l + 1) on the sphere, so a direction that is off by |delta d^| moves the vector
      (Yt_lm)_m by sqrt(l (l + 1)) |delta d^| (1 + 2^-10) (the factor: the second order); |delta d^| <= |delta d| / r with
      order_cases' |delta d| of the float32 leg.  The rounding to a multiple of 2^-40 moves the real and the imaginary part of
      every m by 2^-41: sqrt(2 (2 l + 1)) 2^-41 in the 2-norm.  The float64 chain itself (some 3 l operations of relative 2^-53
      each, on a result with |Yt_lm| <= 1) and the float64 reference: 1e-12 per leg.
          E(a) = sum_b [sqrt(l (l + 1)) |delta d_b| / r_b (1 + 2^-10) + sqrt(2 (2 l + 1)) 2^-41 + 1e-12]
  (2) Propagated.  S = |v|^2: 2 |v| E + E^2.  q-bar = (v(a) / n + sum_b v(b) / n_b) / (n + 1):
          Ebar(a) = (E(a) / n + sum_b E(b) / n_b) / (n + 1);     qbar2: 2 |q-bar| Ebar + Ebar^2
      W is a trilinear form whose coefficient tensor has Frobenius norm 1 (sum (3j)^2 = 1), so by Cauchy-Schwarz
      |W(u, v, w)| <= |u| |v| |w|: C_l = 1 bounds the norm of the form for every l (the norm itself, max |w_l| over unit
      vectors, is smaller; it is not needed), and W(v + dv) - W(v) is at most 3 |v|^2 E + 3 |v| E^2 + E^3.
      D = Re <v(a), v(b)>: |v(a)| E(b) + |v(b)| E(a) + E(a) E(b); A, B as S.
  (3) The float64 sums of the route (n + 2 roundings of the gather, 2 l + 1 of a norm, the 3j sum's) are below 1e-13 relative
      and are covered by 1e-12 absolute on every compared value of order one, scaled with the value's magnitude.
The tests hold v, qbar2, W and S, never w: the quotient amplifies without limit as q -> 0.  The route returns w = W / S^(3/2),
so W is held as w S_ref^(3/2), whose distance from W_ref is at most that of W plus |w| |S^(3/2) - S_ref^(3/2)| <= 1.5
sqrt(S_ref + dS) dS with |w| <= C_l = 1.
Excluded from a comparison: a centre with a LEG-BORDERLINE neighbour (angle_cases' definition), directly or through a neighbour
(its q-bar reads that neighbour's shell); for xi also a centre with a bond whose |D| or |D^2 - thr^2 A B| lies inside its
allowance.  Every test first asserts that the excluded share is at most 10^-3."""
import numpy as np

import angle64 as A
import angle_cases as Q
import order_cases as C
import pair64 as R
import pair_cases as P
import qlm64 as L

U32 = 2.0 ** -24
SHIFT = 40
ONE = float(1 << SHIFT)
CAPACITY = A.CAPACITY
EXCLUDED_CAP = 1e-3
FAMILIES = Q.FAMILIES
family = Q.family
fcc_block, bcc_block, shell = C.fcc_block, C.bcc_block, C.shell
FLOOR = 1e-12


# ---- input families beside angle_cases' and order_cases' ----------------------------------------------------------------------
def hcp_block(n_frames=2):
    """(positions, box): 64 atoms of hcp, a = 3.0, as 4 x 2 x 2 orthorhombic cells (a, sqrt 3 a, sqrt(8/3) a) of four atoms,
    frozen: 12 neighbours at 3.0 (the second shell: 4.24)"""
    a = 3.0
    cell = np.array([a, 3.0 ** 0.5 * a, (8.0 / 3.0) ** 0.5 * a])
    basis = np.array([[0, 0, 0], [.5, .5, 0], [.5, 5.0 / 6.0, .5], [0, 1.0 / 3.0, .5]])
    reps = (4, 2, 2)
    grid = np.stack(np.meshgrid(*[np.arange(k) for k in reps], indexing="ij"), -1).reshape(-1, 1, 3)
    pos = ((grid + basis[None]).reshape(-1, 3) * cell).astype(np.float32)
    box = np.diag(cell * np.array(reps)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(pos, (n_frames,) + pos.shape)), box


def icosahedral_cluster(r=3.0):
    """one frame: a centre and the 12 vertices of an icosahedron of radius r around it, in the cubic box"""
    H = np.asarray(Q.CUBIC, np.float32).astype(np.float64)
    centre = np.array([0.5, 0.5, 0.5]) @ H
    return np.concatenate([centre[None], centre[None] + r * shell("icosahedron")]).astype(np.float32)[None]


# ---- the reference and its allowance --------------------------------------------------------------------------------------
def reference(positions, box, groups, r_cut, step, ls, solid_l=None, threshold=0.7):
    """dict of qlm64.per_atom plus, per order j: `E`[j], `Ebar`[j] (n_o, n_a) the 2-norm allowances of v and q-bar; `excluded`
    (n_o, n_a) bool; `xi` (n_o, n_a) the reference's bond counts (-1: left out) and `xi_loose` (n_o, n_a) bool, a centre with
    a borderline bond"""
    ls = list(ls)
    solid_l = ls[-1] if solid_l is None else solid_l
    ref = L.per_atom(positions, box, groups, r_cut, step, ls, solid_l, threshold)
    S = len(groups)
    n_o, n_a = ref["n"].shape
    ref.update(ls=ls, solid_l=solid_l, threshold=threshold, E=[np.zeros((n_o, n_a)) for _ in ls], Ebar=[np.zeros((n_o, n_a)) for _ in ls],
               excluded=np.zeros((n_o, n_a), bool), xi=np.full((n_o, n_a), -1, np.int64), xi_loose=np.zeros((n_o, n_a), bool))
    if n_a == 0:
        return ref
    atoms, spec = A.species_of(groups)
    rc = A.cutoffs(r_cut, S)
    e64 = P.sigma_error(positions, box)
    aH = np.abs(R.box64(box)[0])
    cut = rc[spec[:, None], spec[None, :]]
    off = ~np.eye(n_a, dtype=bool)
    js = ls.index(solid_l)
    for o, f in enumerate(range(0, np.shape(positions)[0], step)):
        e, d, r = A.frame_pairs(positions[f], box, atoms)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(cut > 0.0, r / cut, np.inf)
            tol = np.where(cut > 0.0, P.tolerance(e.reshape(-1, 3), d.reshape(-1, 3), r.ravel(), box, np.where(cut > 0.0, cut, 1.0).ravel(),
                                                  e64).reshape(n_a, n_a), 0.0)
        dd = (U32 + e64 + 3.0 * U32 * np.abs(e)) @ aH
        dd = np.sqrt((dd * dd).sum(axis=2))                                  # |delta d|_2 of every leg
        direct = ((np.abs(x - 1.0) <= tol) & off).any(axis=1)
        nbs, why, n = ref["lists"][o], ref["why"][o], ref["n"][o]
        for a, nb in enumerate(nbs):
            ref["excluded"][o, a] = direct[a] or bool(direct[nb].any())
            if nb.size and nb.size <= CAPACITY and not np.any(r[a, nb] == 0.0):
                rel = (dd[a, nb] / r[a, nb]).sum() * (1.0 + 2.0 ** -10)
                for j, l in enumerate(ls):
                    ref["E"][j][o, a] = (l * (l + 1)) ** 0.5 * rel + nb.size * ((2.0 * (2 * l + 1)) ** 0.5 * 2.0 ** -41 + FLOOR)
        for a, nb in enumerate(nbs):
            if why[a]:
                continue
            for j in range(len(ls)):
                E = ref["E"][j][o]
                ref["Ebar"][j][o, a] = (E[a] / nb.size + (E[nb] / n[nb]).sum()) / (nb.size + 1)
            E, v = ref["E"][js][o], ref["v"][js][o]
            na, count = float(np.linalg.norm(v[a])), 0
            for b in nb:
                D, AB = ref["bonds"][o][(a, int(b))]
                nb_ = float(np.linalg.norm(v[b]))
                dD = na * E[b] + nb_ * E[a] + E[a] * E[b] + FLOOR * (1.0 + na * nb_)
                dA, dB = 2.0 * na * E[a] + E[a] ** 2, 2.0 * nb_ * E[b] + E[b] ** 2
                dG = 2.0 * abs(D) * dD + dD * dD + threshold ** 2 * (na ** 2 * dB + nb_ ** 2 * dA + dA * dB) + FLOOR * (1.0 + AB)
                g = D * D - threshold ** 2 * AB
                # the decision D > 0 and g > 0 can move only where one condition is within reach and the other not surely false
                if (abs(g) <= dG and D > -dD) or (abs(D) <= dD and g > -dG):
                    ref["xi_loose"][o, a] = True
                count += int(D > 0.0 and g > 0.0)
            ref["xi"][o, a] = count
    return ref


def excluded_share(ref):
    return float(ref["excluded"].sum()) / max(ref["excluded"].size, 1)


def loose_share(ref):
    return float((ref["xi_loose"] & ~ref["excluded"]).sum()) / max(ref["excluded"].size, 1)


def full_vector(q, l):
    """(..., l + 1, 2) int64 or float64, m = 0 .. l -> (..., 2 l + 1) complex over m = -l .. l, times 2^-40"""
    pos = (np.asarray(q, np.float64)[..., 0] + 1j * np.asarray(q, np.float64)[..., 1]) / ONE
    sign = (-1.0) ** np.arange(1, l + 1)
    return np.concatenate([(np.conj(pos[..., 1:]) * sign)[..., ::-1], pos], axis=-1)


def check_q(q, ref, origin, what=""):
    """Q (n_a, columns, 2) int64 of one origin inside E, the left-out centres marked; prints the largest share"""
    q, keep, ok, at, shares = np.asarray(q, np.int64), ~ref["excluded"][origin], True, 0, []
    own = np.isin(ref["why"][origin], (1, 2, 3))
    if not np.array_equal((q[:, 0, 1] != 0)[keep], own[keep]):
        print(f"{what}: other centres marked as left out")
        return False
    for j, l in enumerate(ref["ls"]):
        both = keep & ~own
        delta = np.linalg.norm(full_vector(q[both, at:at + l + 1], l) - ref["v"][j][origin][both], axis=-1)
        shares.append(float((delta / ref["E"][j][origin][both]).max()) if delta.size else 0.0)
        ok = ok and bool(np.all(delta <= ref["E"][j][origin][both]))
        at += l + 1
    print(f"{what}: Q of {int((keep & ~own).sum())} centres, largest |dv| as a share of the allowance per order {np.round(shares, 4)}")
    return ok


def check(got, ref, what=""):
    """the route's per-atom `qbar2`, `w`, `wbar` (n_o, n_a, n_l), `xi`, `n` (n_o, n_a) inside the allowances of `reference` at every
    centre that is not excluded, left out where the reference leaves out; prints the largest shares"""
    keep, out_ref = ~ref["excluded"], ref["why"] != 0
    qbar2, w, wbar, xi, n = (np.asarray(got[k]) for k in ("qbar2", "w", "wbar", "xi", "n"))
    if not np.array_equal(n[keep], ref["n"][keep]):
        print(f"{what}: neighbour counts differ")
        return False
    if not (np.array_equal((xi < 0)[keep], out_ref[keep]) and np.array_equal(np.isnan(qbar2[..., 0])[keep], out_ref[keep])):
        print(f"{what}: other centres left out")
        return False
    both, ok, shares = keep & ~out_ref, True, []
    for j, l in enumerate(ref["ls"]):
        row = []
        for vec, E, val in ((ref["v"][j], ref["E"][j], w[..., j]), (ref["vbar"][j], ref["Ebar"][j], wbar[..., j])):
            v, E, val = vec[both], E[both], val[both]
            norm = np.linalg.norm(v, axis=-1)
            S = norm ** 2
            dS = 2.0 * norm * E + E * E + FLOOR * (1.0 + S)
            if vec is ref["vbar"][j]:
                dq = np.abs(qbar2[..., j][both] - S)
                row.append(float((dq / dS).max()) if dq.size else 0.0)
                ok = ok and bool(np.all(dq <= dS))
            W = np.array([L.w_form(x, l) for x in v])
            dW = 3.0 * S * E + 3.0 * norm * E * E + E ** 3 + 1.5 * np.sqrt(S + dS) * dS + FLOOR * (1.0 + norm ** 3)
            held = S > dS                                                    # (a vector inside its own allowance of 0: nothing to hold)
            dw = np.abs(np.where(held, val, 0.0) * S ** 1.5 - np.where(held, W, 0.0))
            row.append(float((dw / dW).max()) if dw.size else 0.0)
            ok = ok and bool(np.all(dw <= dW)) and not np.any(np.isnan(val[held]))
        shares.append(row)
    tight = both & ~ref["xi_loose"]
    ok_xi = np.array_equal(xi[tight], ref["xi"][tight])
    print(f"{what}: {int(both.sum())} centres compared, {int(ref['excluded'].sum())} excluded, {int((both & ref['xi_loose']).sum())} with a "
          f"borderline bond; per order shares of the allowance (W, qbar2, Wbar) {np.round(shares, 4).tolist()}; xi equal: {ok_xi}")
    return ok and ok_xi


# ---- the bins ---------------------------------------------------------------------------------------------------------
def exact_q_bin(qbar2, n_q):
    """the largest i < n_q with i^2 <= fl(qbar2 n_q^2), the product rounded once as stated, the comparison in exact integers"""
    from fractions import Fraction
    rhs = Fraction(float(np.float64(qbar2) * np.float64(n_q * n_q)))
    i = 0
    while i + 1 < n_q and (i + 1) ** 2 <= rhs:
        i += 1
    return i


def q_bin(qbar2, n_q):
    """the stated bisection, float64"""
    rhs = np.float64(qbar2) * np.float64(n_q * n_q)
    left, right = 0, n_q
    while right - left > 1:
        mid = (left + right) >> 1
        left, right = (mid, right) if np.float64(mid * mid) <= rhs else (left, mid)
    return left


def w_bin(w, n_w, w_range):
    """the stated bin of w: floor(fl(fl(w + R) c)), c = fl(n_w / fl(2 R)); -1: outside or not a number"""
    u = (np.float64(w) + np.float64(w_range)) * (np.float64(n_w) / (np.float64(2.0) * np.float64(w_range)))
    return int(u) if 0.0 <= u < n_w else -1


def rows_of(got, sizes, n_l, n_q, n_w, w_range):
    """(S, R) int64: the histograms and counters that the two bin rules give for the per-atom values of `got`, in the layout of
    psa_local_order's hist; the left-out centres by their kind in got["why"] where present, else all under `truncated`..`incomplete`
    summed into one number that the caller compares with the sum of the four"""
    qbar2, w, wbar, xi = (np.asarray(got[k]) for k in ("qbar2", "w", "wbar", "xi"))
    start = np.concatenate([[0], np.cumsum(sizes)])
    at_w, at_wb, at_xi = n_l * n_q, n_l * n_q + n_l * n_w, n_l * n_q + 2 * n_l * n_w
    at_out = at_xi + CAPACITY + 1
    rows = np.zeros((len(sizes), at_out + 4 + 4 * n_l), np.int64)
    for s in range(len(sizes)):
        for o in range(xi.shape[0]):
            for a in range(start[s], start[s + 1]):
                if xi[o, a] < 0:
                    rows[s, at_out] += 1                                     # (the four kinds together)
                    continue
                rows[s, at_xi + xi[o, a]] += 1
                for j in range(n_l):
                    rows[s, j * n_q + q_bin(qbar2[o, a, j], n_q)] += 1
                    for which, (val, base) in enumerate(((w[o, a, j], at_w), (wbar[o, a, j], at_wb))):
                        if np.isnan(val):
                            rows[s, at_out + 4 + (2 * which + 1) * n_l + j] += 1
                        elif w_bin(val, n_w, w_range) < 0:
                            rows[s, at_out + 4 + 2 * which * n_l + j] += 1
                        else:
                            rows[s, base + j * n_w + w_bin(val, n_w, w_range)] += 1
    return rows


def fold_left_out(hist, n_l, n_q, n_w):
    """the route's rows with the four left-out counters summed into the first, as `rows_of` files them"""
    rows = np.asarray(hist).astype(np.int64).copy()
    at = n_l * n_q + 2 * n_l * n_w + CAPACITY + 1
    rows[:, at] = rows[:, at:at + 4].sum(axis=1)
    rows[:, at + 1:at + 4] = 0
    return rows


def identities(hist, sizes, n_o, n_l, n_q, n_w):
    """every identity of the definition that the counts alone can show"""
    rows = np.asarray(hist).astype(np.int64)
    at_w, at_wb, at_xi = n_l * n_q, n_l * n_q + n_l * n_w, n_l * n_q + 2 * n_l * n_w
    at_out = at_xi + CAPACITY + 1
    total, left = n_o * np.asarray(sizes, np.int64), rows[:, at_out:at_out + 4].sum(axis=1)
    ok = np.array_equal(rows[:, at_xi:at_out].sum(axis=1) + left, total)
    for j in range(n_l):
        ok = ok and np.array_equal(rows[:, j * n_q:(j + 1) * n_q].sum(axis=1) + left, total)
        for which, base in enumerate((at_w, at_wb)):
            extra = rows[:, at_out + 4 + 2 * which * n_l + j] + rows[:, at_out + 4 + (2 * which + 1) * n_l + j]
            ok = ok and np.array_equal(rows[:, base + j * n_w:base + (j + 1) * n_w].sum(axis=1) + extra + left, total)
    return bool(ok)


# ---- a NumPy twin of the stated arithmetic, with the planted faults -----------------------------------------------------
FAULTS = ("centre_left_out", "divide_by_n", "neighbour_not_normalised", "negative_m_dropped", "no_sign_in_minus_m", "wrong_3j_m3",
          "no_positive_d", "first_64")


def norms():
    """N_lm at [l, m] as the host forms it"""
    out = np.zeros((13, 13))
    for l in range(13):
        for m in range(l + 1):
            prod = np.float64(1.0)
            for k in range(l - m + 1, l + m + 1):
                prod = prod * np.float64(k)
            out[l, m] = (-1.0 if m & 1 else 1.0) * np.sqrt(np.float64(1.0) / prod)
    return out


NORMS = norms()


def harmonics_model(d32, ls):
    """t_lm of float32 legs (n, 3) by the stated float64 chain: per order (n, l + 1, 2) int64"""
    d = np.asarray(d32, np.float32).astype(np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    r = np.sqrt(z * z + (y * y + x * x))
    ux, uy, uz = x / r, y / r, z / r
    l_max = max(ls)
    out = {l: np.zeros((d.shape[0], l + 1, 2), np.int64) for l in ls}
    cr, ci, pmm = np.ones_like(ux), np.zeros_like(ux), 1.0
    for m in range(l_max + 1):
        if m:
            cr, ci = cr * ux + (-(ci * uy)), cr * uy + ci * ux
            pmm = pmm * (2 * m - 1)
        p2, p1 = np.zeros_like(ux), np.zeros_like(ux)
        for l in range(m, l_max + 1):
            if l == m:
                p = np.full_like(ux, pmm)
            elif l == m + 1:
                p = (pmm * (2 * m + 1)) * uz
            else:
                p = ((2 * l - 1) * (uz * p1) + (-((l + m - 1) * p2))) / (l - m)
            p2, p1 = p1, p
            if l in out:
                s = NORMS[l, m] * p1
                out[l][:, m, 0] = np.rint((s * cr) * ONE).astype(np.int64)
                out[l][:, m, 1] = np.rint((s * ci) * ONE).astype(np.int64)
    return out


def _comp(v, m, fault=None):
    """v_m of (l + 1, 2) float64 rows m = 0 .. l: v_{-m} = (-1)^m conj v_m"""
    am = abs(m)
    a, b = v[am, 0], v[am, 1]
    if m < 0:
        flip = (am & 1) and fault != "no_sign_in_minus_m"
        return (-a, b) if flip else (a, -b)
    return a, b


def w_model(v, l, table, fault=None):
    """W_l of (l + 1, 2) float64 by the stated order: the dense table's terms dealt to 64 partial sums, a butterfly"""
    side = 2 * l + 1
    part = np.zeros(64)
    for t in range(side * side):
        m1, m2 = t // side - l, t % side - l
        m3 = -(m1 + m2)
        if abs(m3) > l:
            continue
        if fault == "wrong_3j_m3":
            m3 = -m3
        (ar, ai), (br, bi), (cr, ci) = _comp(v, m1, fault), _comp(v, m2, fault), _comp(v, m3, fault)
        pr, pi = ar * br + (-(ai * bi)), ar * bi + ai * br
        part[t % 64] = part[t % 64] + table[m1 + l, m2 + l] * (pr * cr + (-(pi * ci)))
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[np.arange(64) ^ o]
    return float(part[0])


def norm2_model(v, fault=None):
    s = np.float64(0.0)
    for m in range(v.shape[0]):
        t = v[m, 0] * v[m, 0] + v[m, 1] * v[m, 1]
        s = s + (2.0 * t if m and fault != "negative_m_dropped" else t)
    return float(s)


def model(positions, box, groups, r_cut, step, ls, solid_l=None, threshold=0.7, fault=None):
    """dict(qbar2, w, wbar (n_o, n_a, n_l) float64, xi, n (n_o, n_a), q: per origin (n_a, columns, 2) int64) as the stated float32
    neighbour chain, the float64 harmonics and the integer sums give them.  Faults: FAULTS"""
    from psa_amd import wigner_3j_table
    ls = list(ls)
    solid_l = ls[-1] if solid_l is None else solid_l
    S, n_l = len(groups), len(ls)
    rc = A.cutoffs(r_cut, S)
    atoms, spec = A.species_of(groups)
    n = atoms.size
    origins = range(0, np.shape(positions)[0], step)
    cols = sum(l + 1 for l in ls)
    out = dict(qbar2=np.full((len(origins), n, n_l), np.nan), w=np.full((len(origins), n, n_l), np.nan),
               wbar=np.full((len(origins), n, n_l), np.nan), xi=np.full((len(origins), n), -1, np.int64),
               n=np.zeros((len(origins), n), np.int64), q=[np.zeros((n, cols, 2), np.int64) for _ in origins])
    if n == 0:
        return out
    c = P.fractions_model(positions, box)
    h = R.box64(box)[0].astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(rc > 0.0, 1.0 / rc, 0.0).astype(np.float32)[spec[:, None], spec[None, :]]
    tables = {l: wigner_3j_table(l) for l in ls}
    thr2 = np.float64(threshold) * np.float64(threshold)
    for o, fr in enumerate(origins):
        f = c[fr][atoms]
        e = (f[None, :, :] - f[:, None, :]).astype(np.float32)
        e = e - np.rint(e)
        d = np.stack([P._fma32(e[..., 2], h[2, k], P._fma32(e[..., 1], h[1, k], e[..., 0] * h[0, k])) for k in range(3)], -1)
        r2 = P._fma32(d[..., 2], d[..., 2], P._fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
        near = (np.sqrt(r2) * inv < np.float32(1.0)) & (inv > 0) & ~np.eye(n, dtype=bool)
        nbs, marked, q = [], np.zeros(n, bool), out["q"][o]
        for a in range(n):
            nb = np.flatnonzero(near[a])
            out["n"][o, a] = nb.size
            if nb.size > CAPACITY and fault == "first_64":
                nb = nb[:CAPACITY]
            nbs.append(nb)
            if nb.size > CAPACITY or nb.size == 0 or not np.all(d[a, nb].astype(np.float64).any(axis=1)):
                marked[a], q[a, 0, 1] = True, -1
                continue
            t, at = harmonics_model(d[a, nb], ls), 0
            for l in ls:
                q[a, at:at + l + 1] = t[l].sum(axis=0)
                at += l + 1
        for a in range(n):
            nb = nbs[a]
            if marked[a] or marked[nb].any():
                continue
            m, at = np.float64(nb.size), 0
            for j, l in enumerate(ls):
                va = q[a, at:at + l + 1].astype(np.float64) * (1.0 / ONE)
                total = np.zeros_like(va) if fault == "centre_left_out" else va / m
                for b in nb:
                    total = total + (q[b, at:at + l + 1].astype(np.float64) * (1.0 / ONE)) / (m if fault == "neighbour_not_normalised"
                                                                                              else np.float64(nbs[b].size))
                vbar = total / (m if fault == "divide_by_n" else m + 1.0)
                A2, B2 = norm2_model(va, fault), norm2_model(vbar, fault)
                out["qbar2"][o, a, j] = B2
                for key, v, s in (("w", va, A2), ("wbar", vbar, B2)):
                    if s != 0.0:
                        out[key][o, a, j] = w_model(v, l, tables[l], fault) / (s * np.sqrt(s))
                if l == solid_l:
                    xi = 0
                    for b in nb:
                        vb = q[b, at:at + l + 1].astype(np.float64) * (1.0 / ONE)
                        D = np.float64(0.0)
                        for k in range(l + 1):
                            t = va[k, 0] * vb[k, 0] + va[k, 1] * vb[k, 1]
                            D = D + (2.0 * t if k else t)
                        xi += int((D > 0.0 or fault == "no_positive_d") and D * D > thr2 * (A2 * norm2_model(vb)))
                    out["xi"][o, a] = xi
                at += l + 1
    return out
