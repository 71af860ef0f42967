"""Inputs of the bond-persistence tests, the allowance of the counts derived from the arithmetic stated at
psa_bond_persistence in include/psa_hip.h and from nothing in the code, and a NumPy twin of that arithmetic with the planted
faults the host test holds outside the allowance.

The allowance.  Every test of the route is the pair chain of pair_cases.py with dr = a radius R (r_cut at the origin, r_break
at a later frame): x = |d| / R carries at most `pair_cases.tolerance`.  A BOND EVENT is one such test of a pair the reference
lists, or could list, at an origin: its listing at o, its aliveness at o + v.  An event is BORDERLINE when |x - 1| <= that
tolerance; every other event falls the same way in the route as in the reference.  So per lag j and origin o:

    bonds[j, al, be]     may differ by the pairs whose listing is borderline
    alive[j, al, be]     by those, and by the listed (or borderline-listed) pairs whose aliveness at o + tau_j is borderline
    unbroken[j, al, be]  by the first, and by the pairs with a borderline aliveness at a visited frame that are not surely dead
                         at another one
    lost[j, al, m]       a centre with a borderline event among its pairs lies somewhere in [m_lo, m_hi], m_lo its surely
                         listed pairs that are surely dead, m_hi its possibly listed pairs that are not surely alive: every
                         bin of that range may differ by one for it
    truncated[j, al]     by the centres whose count can cross the capacity (sure <= 64 < sure + borderline); such a centre
                         widens everything it feeds: all of its possible pairs in the three pair counts, lost[0 .. 64]

The condition on the inputs: the borderline share of the bond events stays at or below BORDERLINE_CAP in the reference alone
(`reference` returns both numbers; the host test asserts it).  The identities among the counts hold exactly."""
import numpy as np

import angle64 as A
import angle_cases as Q
import pair64 as R
import pair_cases as P

CAPACITY = A.CAPACITY
BORDERLINE_CAP = 2e-3
KEYS = ("bonds", "alive", "unbroken", "lost", "truncated")
HYSTERESIS = 1.2


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def lags_of(n_frames, sample_step=1):
    """the lags (0, 1, 2, 7, T - 1) that a trajectory of T frames holds; with sample_step 2, where a lag must be even, the
    even ones of them, 6 and the last even frame in their place"""
    want = {0, 1, 2, 7, n_frames - 1} if sample_step == 1 else {0, 2, 6, 2 * ((n_frames - 1) // 2)}
    return sorted(t for t in want if 0 <= t <= n_frames - 1)


def species(kind, n_atoms):
    """"one", "two" (angle_cases.two_species) or "three" (angle_cases.three_species: one of them empty)"""
    return {"one": lambda: [np.arange(n_atoms)], "two": lambda: Q.two_species(n_atoms), "three": lambda: Q.three_species(n_atoms)}[kind]()


def cutoffs(kind, r_cut, matrix):
    """a scalar, or angle_cases.matrix_cutoff with its zero entry"""
    S = {"one": 1, "two": 2, "three": 3}[kind]
    return Q.matrix_cutoff(r_cut, S) if matrix else float(r_cut)


def breaks(r_cut, factor):
    """r_break = factor r_cut, entry by entry (a zero stays a zero)"""
    return np.asarray(r_cut, np.float64) * factor if np.ndim(r_cut) else float(r_cut) * factor


def walk_split():
    """angle_cases.walk_case with the centre of the sphere (and the four far atoms) as one species and the sphere's 65 atoms
    as the other: the truncated centre makes bonds[0, 1] differ from bonds[1, 0]"""
    pos, box, _, r_cut = Q.walk_case()
    return pos, box, [np.array([0, 66, 67, 68, 69]), np.arange(1, 66)], r_cut


def dimer(distances, box=Q.CUBIC):
    """two atoms `distances[f]` apart along x at frame f, far from every boundary: (T, 2, 3) float32"""
    H = np.asarray(box, np.float32).astype(np.float64)
    at = np.array([0.3, 0.4, 0.5]) @ H
    return np.asarray([[at, at + np.array([d, 0.0, 0.0])] for d in distances], np.float32)


# ---- the allowance ----------------------------------------------------------------------------------------------------------
class Frames:
    """per frame of a trajectory the (n, n) distances of the listed atoms and the numerator of their tolerance (what |d|
    carries: pair_cases.tolerance with dr = 1), computed once and shared by every reference over the same atoms"""

    def __init__(self, positions, box, groups):
        self.atoms, self.spec = A.species_of(groups)
        self.n, self.T = self.atoms.size, np.shape(positions)[0]
        self.r, self.tol = [], []
        e64 = P.sigma_error(positions, box) if self.n else 0.0
        for frame in positions:
            if self.n == 0:
                break
            e, d, r = A.frame_pairs(frame, box, self.atoms)
            self.r.append(r)
            self.tol.append(P.tolerance(e.reshape(-1, 3), d.reshape(-1, 3), r.ravel(), box, 1.0, e64).reshape(self.n, self.n))

    def test(self, f, radius):
        """(below: r < R by the definition, edge: borderline, sure: below and not borderline) of every ordered pair at frame f
        against the (n, n) radii; a radius of 0 is no bond"""
        on = radius > 0.0
        safe = np.where(on, radius, 1.0)
        edge = on & (np.abs(self.r[f] / safe - 1.0) <= self.tol[f] / safe)
        below = on & (self.r[f] < radius)
        return below, edge, below & ~edge


def reference(positions, box, groups, r_cut, r_break, lags, step=1, sample_step=1, continuous=True, frames=None):
    """dict: the reference counts of KEYS (int64, by the definition), `<key>_allowed` of the same shapes, `events` and
    `borderline` (the bond events and the borderline ones among them), `most` the most neighbours of a centre"""
    S = len(groups)
    fr = Frames(positions, box, groups) if frames is None else frames
    n, T, spec, n_l = fr.n, np.shape(positions)[0], fr.spec, len(lags)
    out = dict(bonds=np.zeros((n_l, S, S), np.int64), alive=np.zeros((n_l, S, S), np.int64), unbroken=np.zeros((n_l, S, S), np.int64),
               lost=np.zeros((n_l, S, CAPACITY + 1), np.int64), truncated=np.zeros((n_l, S), np.int64), events=0, borderline=0, most=0)
    for k in KEYS:
        out[k + "_allowed"] = np.zeros_like(out[k])
    if n == 0:
        return out
    rc, rb = A.cutoffs(r_cut, S), A.cutoffs(r_cut if r_break is None else r_break, S)
    cut, brk = rc[spec[:, None], spec[None, :]], rb[spec[:, None], spec[None, :]]
    off = ~np.eye(n, dtype=bool)
    hot = (spec[:, None] == np.arange(S)[None, :]).astype(np.int64)         # (n, S)
    per_pair = lambda m: hot.T @ m.astype(np.int64) @ hot                   # noqa: E731  (S, S): rows by centre, columns by neighbour
    later = {}                                                              # frame -> its test against r_break

    def broken(f):
        if f not in later:
            later[f] = fr.test(f, brk)
        return later[f]
    for j, lag in enumerate(int(t) for t in lags):
        steps = list(range(sample_step, lag + 1, sample_step)) if continuous else []
        for o in range(0, T - lag, step):
            near, edge, sure = (m & off for m in fr.test(o, cut))
            maybe = sure | edge
            count, n_sure, n_maybe = near.sum(axis=1), sure.sum(axis=1), maybe.sum(axis=1)
            out["most"] = max(out["most"], int(count.max()))
            gone, crossing = n_sure > CAPACITY, (n_sure <= CAPACITY) & (n_maybe > CAPACITY)
            up, up_edge, up_sure = broken(o + lag)
            whole, any_edge, any_dead = np.ones((n, n), bool), np.zeros((n, n), bool), np.zeros((n, n), bool)
            for v in steps:
                b, e, s = broken(o + v)
                whole &= b
                any_edge |= e
                any_dead |= ~b & ~e
                out["events"] += int(maybe.sum())
                out["borderline"] += int((maybe & e).sum())
            out["events"] += 2 * int(maybe.sum())
            out["borderline"] += int(edge.sum()) + int((maybe & up_edge).sum())
            # the reference's own counts
            kept = near & (count <= CAPACITY)[:, None]
            out["bonds"][j] += per_pair(kept)
            out["alive"][j] += per_pair(kept & up)
            if continuous:
                out["unbroken"][j] += per_pair(kept & whole)
            rows = np.flatnonzero(count <= CAPACITY)
            np.add.at(out["lost"][j], (spec[rows], (kept & ~up).sum(axis=1)[rows]), 1)
            out["truncated"][j] += np.bincount(spec[count > CAPACITY], minlength=S)
            # what may differ
            live = ~gone[:, None]
            loose = np.where(crossing[:, None], maybe, edge) & live          # pairs that may be listed or not
            out["bonds_allowed"][j] += per_pair(loose)
            out["alive_allowed"][j] += per_pair(loose | (maybe & up_edge & live))
            if continuous:
                out["unbroken_allowed"][j] += per_pair(loose | (maybe & any_edge & ~any_dead & live))
            out["truncated_allowed"][j] += np.bincount(spec[crossing], minlength=S)
            m_lo, m_hi = (sure & ~up & ~up_edge).sum(axis=1), (maybe & ~up_sure).sum(axis=1)
            moving = ~gone & (crossing | edge.any(axis=1) | (maybe & up_edge).any(axis=1))
            for a in np.flatnonzero(moving):
                lo, hi = (0, CAPACITY) if crossing[a] else (int(m_lo[a]), min(int(m_hi[a]), CAPACITY))
                out["lost_allowed"][j, spec[a], lo:hi + 1] += 1
    return out


def check(got, ref, what=""):
    """the counts of a route (a dict with KEYS) inside the allowance of `reference`; prints what moved"""
    moved = {k: int(np.abs(np.asarray(got[k]).astype(np.int64) - ref[k]).sum()) for k in KEYS}
    print(f"{what}: {ref['borderline']} borderline of {ref['events']} bond events, most neighbours {ref['most']}; counts moved: {moved}")
    return all(np.all(np.abs(np.asarray(got[k]).astype(np.int64) - ref[k]) <= ref[k + "_allowed"]) for k in KEYS)


def identities(got, sizes, n_frames, lags, step, continuous=True):
    """the exact identities of the definition that the counts alone can show"""
    g = {k: np.asarray(got[k]).astype(np.int64) for k in KEYS}
    n_o = np.array([R.n_origins(n_frames, int(t), step) for t in lags], np.int64)
    m = np.arange(CAPACITY + 1)
    ok = np.array_equal(g["lost"].sum(axis=2) + g["truncated"], n_o[:, None] * np.asarray(sizes, np.int64)[None, :])
    ok = ok and np.array_equal((g["lost"] * m).sum(axis=2), (g["bonds"] - g["alive"]).sum(axis=2))
    ok = ok and np.all(g["alive"] <= g["bonds"])
    if continuous:
        ok = ok and np.all(g["unbroken"] <= g["alive"])
    else:
        ok = ok and not g["unbroken"].any()
    for j, lag in enumerate(lags):
        if int(lag) == 0:
            ok = ok and np.array_equal(g["alive"][j], g["bonds"][j]) and (not continuous or np.array_equal(g["unbroken"][j], g["bonds"][j]))
            ok = ok and not g["lost"][j, :, 1:].any()
    if not g["truncated"].any():
        ok = ok and all(np.array_equal(g[k], g[k].transpose(0, 2, 1)) for k in ("bonds", "alive", "unbroken"))
    return bool(ok)


# ---- a NumPy twin of the stated arithmetic, with the planted faults -----------------------------------------------------
FAULTS = ("break_is_cut", "all_origins", "continuous_is_intermittent", "first_64", "lost_from_count", "transposed", "sample_step_ignored")


def lengths32(positions, box, groups):
    """per frame sqrt(r2) (n, n) float32 of the stated chain: e[a, b] = c(b) - c(a), e - rint(e), d = e h, r2"""
    atoms, _ = A.species_of(groups)
    c = P.fractions_model(positions, box)
    h = R.box64(box)[0].astype(np.float32)
    out = []
    for f in range(c.shape[0]):
        at = c[f][atoms]
        e = (at[None, :, :] - at[:, None, :]).astype(np.float32)
        e = e - np.rint(e)
        d = [P._fma32(e[..., 2], h[2, k], P._fma32(e[..., 1], h[1, k], e[..., 0] * h[0, k])) for k in range(3)]
        out.append(np.sqrt(P._fma32(d[2], d[2], P._fma32(d[1], d[1], d[0] * d[0]))))
    return out


def _bits(rows):
    """per row of a boolean (n, 64) array the uint64 whose bit i is column i"""
    return (rows.astype(np.uint64) << np.arange(CAPACITY, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def _packed(near, *layers):
    """(the columns of each row's neighbours, ascending, -1 padding (n, 64) int32; per layer its values at them (n, 64) bool)"""
    n = near.shape[0]
    order = np.argsort(~near, axis=1, kind="stable")[:, :CAPACITY]
    held = np.take_along_axis(near, order, axis=1)
    pad = ((0, 0), (0, CAPACITY - order.shape[1]))
    lists = np.pad(np.where(held, order, -1).astype(np.int32), pad, constant_values=-1)
    return (lists,) + tuple(np.pad(np.take_along_axis(m, order, axis=1) & held, pad) for m in layers)


def model(positions, box, groups, r_cut, r_break, lags, step=1, sample_step=1, continuous=True, fault=None, masks=False, lengths=None):
    """dict of KEYS (int64) as the stated float32 arithmetic gives them; with `masks` also alive_masks, unbroken_masks
    (n_lags, n_o(0), n_a) uint64 and lists (n_o(0), n_a, 64) int32 (-1 padding).  Faults: FAULTS"""
    S, T = len(groups), np.shape(positions)[0]
    atoms, spec = A.species_of(groups)
    n, n_l, one = atoms.size, len(lags), np.float32(1.0)
    n_o0 = R.n_origins(T, 0, step)
    out = dict(bonds=np.zeros((n_l, S, S), np.int64), alive=np.zeros((n_l, S, S), np.int64), unbroken=np.zeros((n_l, S, S), np.int64),
               lost=np.zeros((n_l, S, CAPACITY + 1), np.int64), truncated=np.zeros((n_l, S), np.int64))
    if masks:
        out.update(alive_masks=np.zeros((n_l, n_o0, n), np.uint64), unbroken_masks=np.zeros((n_l, n_o0, n), np.uint64),
                   lists=np.full((n_o0, n, CAPACITY), -1, np.int32))
    if n == 0:
        return out
    rc, rb = A.cutoffs(r_cut, S), A.cutoffs(r_cut if r_break is None or fault == "break_is_cut" else r_break, S)
    with np.errstate(divide="ignore"):
        inv_c = np.where(rc > 0.0, 1.0 / rc, 0.0).astype(np.float32)[spec[:, None], spec[None, :]]
        inv_b = np.where(rb > 0.0, 1.0 / rb, 0.0).astype(np.float32)[spec[:, None], spec[None, :]]
    s = lengths32(positions, box, groups) if lengths is None else lengths
    off = ~np.eye(n, dtype=bool)
    hot = (spec[:, None] == np.arange(S)[None, :]).astype(np.int64)
    per_pair = lambda m: hot.T @ m.astype(np.int64) @ hot                   # noqa: E731
    listed = lambda f: (s[f] * inv_c < one) & (inv_c > 0) & off             # noqa: E731
    up_at = lambda f: s[min(f, T - 1)] * inv_b < one                        # noqa: E731  (min: fault "all_origins" alone reaches beyond)
    every = 1 if fault == "sample_step_ignored" else sample_step
    if masks:
        for k, o in enumerate(range(0, T, step)):
            out["lists"][k] = _packed(listed(o))[0]
    for j, lag in enumerate(int(t) for t in lags):
        for k, o in enumerate(range(0, T if fault == "all_origins" else T - lag, step)):
            near = listed(o)
            count = near.sum(axis=1)
            if fault == "first_64":
                near &= np.cumsum(near, axis=1) <= CAPACITY
            else:
                near &= (count <= CAPACITY)[:, None]
            up = near & up_at(o + lag)
            whole = near.copy()
            for v in range(every, lag + 1, every) if continuous else []:
                whole &= up_at(o + v)
            if fault == "continuous_is_intermittent":
                whole = up
            if not continuous:
                whole[:] = False
            out["bonds"][j] += per_pair(near)
            out["alive"][j] += per_pair(up)
            out["unbroken"][j] += per_pair(whole)
            rows = np.flatnonzero(count <= CAPACITY) if fault != "first_64" else np.arange(n)
            m = (near & ~up).sum(axis=1)
            if fault == "lost_from_count":
                m = np.maximum(near.sum(axis=1) - listed(min(o + lag, T - 1)).sum(axis=1), 0)
            np.add.at(out["lost"][j], (spec[rows], m[rows]), 1)
            out["truncated"][j] += np.bincount(spec[count > CAPACITY], minlength=S)
            if masks and k < n_o0:
                out["alive_masks"][j, k], out["unbroken_masks"][j, k] = (_bits(m) for m in _packed(near, up, whole)[1:])
    if fault == "transposed":
        for key in ("bonds", "alive", "unbroken"):
            out[key] = out[key].transpose(0, 2, 1).copy()
    return out
