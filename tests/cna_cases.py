"""Inputs of the common-neighbour tests, the comparison the GPU test makes, the centres that comparison leaves out, a NumPy twin
of the arithmetic stated at psa_common_neighbours in include/psa_hip.h with the planted faults the host test holds outside the
comparison, and the pure-integer route from the engine's own neighbour lists.

The comparison.  Everything after the adjacency is integers, so the route must give the float64 reference's numbers exactly
wherever the adjacency is the same.  A pair's float32 test can differ from r < r_cut only when x = |d| / r_cut lies within
`pair_cases.tolerance` of 1 (the leg tolerance of angle_cases: the pair chain with dr = r_cut).  A centre DEPENDS on the pairs
(a, b) for every listed atom b -- its own bonds and every near miss just outside --, and on the pairs among its neighbours.  A
centre with such a pair inside the tolerance is EXCLUDED: its per-atom rows are not compared.  The counts are compared through
the per-atom rows: the route's counts must be the sums of its own rows, exactly, and its rows the reference's on every centre
that is not excluded; where no centre is excluded (the families of these tests) the counts are compared directly as well."""
import numpy as np

import angle64 as A
import angle_cases as Q
import cna64 as R
import order_cases
import pair64
import pair_cases as P
import persist_cases as C
import qlm_cases

CAPACITY = R.CAPACITY
NO_BOND = R.NO_BOND
EXCLUDED_CAP = 1e-3                                                       # order_cases.EXCLUDED_CAP
COUNTS = ("signature_counts", "signature_outside", "type_counts", "truncated")
ROWS = ("types", "n", "bond_signatures")
species, cutoffs, walk_split = C.species, C.cutoffs, C.walk_split


# ---- sums of the per-atom rows --------------------------------------------------------------------------------------------
def aggregate(n, types, words, groups):
    """the counts of a call from its per-atom rows n, types (n_o, n_a) and words (n_o, n_a, 64)"""
    S = len(groups)
    _, spec = A.species_of(groups)
    n_o = np.shape(types)[0]
    out = dict(signature_counts=np.zeros((S,) + R.TABLE, np.uint64), signature_outside=np.zeros(S, np.uint64),
               type_counts=np.zeros((n_o, S, len(R.TYPES)), np.uint64), truncated=np.zeros(S, np.uint64))
    for al in range(S):
        of = spec == al
        t = np.asarray(types)[:, of]
        out["truncated"][al] = int((t < 0).sum())
        for code in range(len(R.TYPES)):
            out["type_counts"][:, al, code] = (t == code).sum(axis=1)
        w = np.asarray(words)[:, of].ravel()
        w = w[w != NO_BOND].astype(np.int64)
        j, k, l = w & 255, (w >> 8) & 255, w >> 16
        inside = (j < R.TABLE[0]) & (k < R.TABLE[1]) & (l < R.TABLE[2])
        np.add.at(out["signature_counts"][al], (j[inside], k[inside], l[inside]), 1)
        out["signature_outside"][al] = int((~inside).sum())
    return out


def result_of(frames, groups):
    """the dict `Engine.common_neighbours(per_atom=True)` returns, from per origin (n, types, words)"""
    n_a = sum(len(g) for g in groups)
    n = np.array([f[0] for f in frames], np.int32).reshape(len(frames), n_a)
    types = np.array([f[1] for f in frames], np.int32).reshape(len(frames), n_a)
    words = np.array([f[2] for f in frames], np.uint32).reshape(len(frames), n_a, CAPACITY)
    return dict(aggregate(n, types, words, groups), types=types, n=n, bond_signatures=words)


# ---- the reference, the centres left out, what the inputs hold ------------------------------------------------------------------
class Reference:
    """every frame of a trajectory by tests/cna64.py, once: per frame (n, types, words), the excluded centres (n_a,) bool and
    the features of the common-neighbour graphs (bonds, branching bonds), the least |x - 1| and |r - r_cut| of a pair; `result(step)` the call's expected dict over the
    origins 0, step, ...; `excluded(step)` (n_o, n_a)"""

    def __init__(self, positions, box, groups, r_cut):
        self.groups, self.frames, self.left_out, self.bonds, self.branching, self.closest = groups, [], [], 0, 0, np.inf
        self.closest_r = np.inf                                            # closest: of |x - 1|; closest_r: of |r - r_cut|
        S = len(groups)
        rc = A.cutoffs(r_cut, S)
        atoms, spec = A.species_of(groups)
        n = atoms.size
        e64 = P.sigma_error(positions, box) if n else 0.0
        for fr in positions:
            count, types, words, around = R.frame(fr, box, groups, r_cut)
            self.frames.append((count, types, words))
            if n == 0:
                self.left_out.append(np.zeros(0, bool))
                continue
            e, d, r = A.frame_pairs(fr, box, atoms)
            cut = rc[spec[:, None], spec[None, :]]
            on = (cut > 0.0) & ~np.eye(n, dtype=bool)
            safe = np.where(on, cut, 1.0)
            tol = P.tolerance(e.reshape(-1, 3), d.reshape(-1, 3), r.ravel(), box, safe.ravel(), e64).reshape(n, n)
            x = r / safe
            edge = on & (np.abs(x - 1.0) <= tol)
            self.closest = min(self.closest, float(np.abs(x - 1.0)[on].min()) if on.any() else np.inf)
            self.closest_r = min(self.closest_r, float(np.abs(r - cut)[on].min()) if on.any() else np.inf)
            out = edge.any(axis=1)
            for a in np.flatnonzero(~out):
                nb = sorted(around[a])
                out[a] = bool(edge[np.ix_(nb, nb)].any())
            self.left_out.append(out)
            for a in range(n):                                             # the features, on the centres that are counted
                if count[a] > CAPACITY:
                    continue
                for b in around[a]:
                    common = around[a] & around[b]
                    self.bonds += 1
                    self.branching += any(len(around[c] & common) >= 3 for c in common)

    def result(self, step=1):
        return with_groups(result_of(self.frames[::step], self.groups), self.groups)

    def excluded(self, step=1):
        return np.array(self.left_out[::step], bool).reshape(len(self.frames[::step]), -1)


def distinct_signatures(res):
    """the distinct words among the bonds of a result with per-atom rows"""
    w = np.asarray(res["bond_signatures"]).ravel()
    return np.unique(w[w != NO_BOND]).size


def check(got, ref, excluded=None, what=""):
    """the comparison: got's counts are the sums of its own rows, and its rows are ref's on every centre not excluded (the counts
    too where none is); prints what differs"""
    shape = np.shape(ref["types"])
    out = np.zeros(shape, bool) if excluded is None else np.asarray(excluded, bool)
    bad = []
    if any(got[k] is None for k in ROWS):
        return False
    if got["types"].shape != shape or got["n"].shape != shape or got["bond_signatures"].shape != shape + (CAPACITY,):
        print(f"{what}: shapes {got['types'].shape}, {got['n'].shape}, {got['bond_signatures'].shape}")
        return False
    own = aggregate(got["n"], got["types"], got["bond_signatures"], ref["groups"])
    for k in COUNTS:
        if not np.array_equal(np.asarray(got[k]), own[k]):
            bad.append(f"{k} is not the sum of the rows")
        if not out.any() and not np.array_equal(np.asarray(got[k]), ref[k]):
            bad.append(f"{k} differs from the reference")
    # n counts on beyond the capacity, and n <= 64 <=> the rows are held
    if not np.array_equal((np.asarray(got["n"]) > CAPACITY), np.asarray(got["types"]) < 0):
        bad.append("types = -1 and n > 64 name different centres")
    for k in ROWS:
        if not np.array_equal(np.asarray(got[k])[~out], np.asarray(ref[k])[~out]):
            bad.append(f"{k} differs on {int((np.asarray(got[k])[~out] != np.asarray(ref[k])[~out]).sum())} cells")
    if bad:
        print(f"{what}: " + "; ".join(bad))
    return not bad


def with_groups(res, groups):
    res = dict(res)
    res["groups"] = groups
    return res


# ---- the twin ---------------------------------------------------------------------------------------------------------------
FAULTS = ("longest_path", "bonds_twice", "self_common", "first_component", "bit63_dropped", "half_round_twice", "one_cutoff",
          "bcc_at_12", "first_64")


def near32(positions, box, groups, r_cut, step=1):
    """per origin the (n, n) bool matrix of the float32 chain (cluster_cases.twin_lists' arithmetic): x < 1 and a cut-off > 0"""
    S = len(groups)
    rc = A.cutoffs(r_cut, S)
    atoms, spec = A.species_of(groups)
    n = atoms.size
    c = P.fractions_model(positions, box)
    h = pair64.box64(box)[0].astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(rc > 0.0, 1.0 / rc, 0.0).astype(np.float32)[spec[:, None], spec[None, :]]
    out = []
    for fr in range(0, np.shape(positions)[0], step):
        f = c[fr][atoms]
        e = (f[None, :, :] - f[:, None, :]).astype(np.float32)
        e = e - np.rint(e)
        d = np.stack([P._fma32(e[..., 2], h[2, k], P._fma32(e[..., 1], h[1, k], e[..., 0] * h[0, k])) for k in range(3)], -1)
        r2 = P._fma32(d[..., 2], d[..., 2], P._fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
        out.append((np.sqrt(r2) * inv < np.float32(1.0)) & (inv > 0) & ~np.eye(n, dtype=bool))
    return out


def _longest_path(nodes, rows):
    """the most bonds of a simple path within the piece `nodes` (a mask); pieces of more than 7 members: its bonds"""
    members = [i for i in range(64) if nodes >> i & 1]
    if len(members) > 7:
        return sum(bin(rows[i] & nodes).count("1") for i in members) // 2
    best = 0

    def walk(at, seen, length):
        nonlocal best
        best = max(best, length)
        for v in members:
            if rows[at] >> v & 1 and not seen >> v & 1:
                walk(v, seen | 1 << v, length + 1)
    for u in members:
        walk(u, 1 << u, 0)
    return best


def centre_model(rows, n, fault=None):
    """(types code, the n words) of a centre from its adjacency rows (Python ints, bit j of rows[i]: b_i - b_j bonded), by the
    masks of the stated evaluation: j a popcount, the flood that pops every common neighbour once"""
    if fault == "bit63_dropped":
        rows = [r & ((1 << 63) - 1) for r in rows]
    sigs = []
    for i in range(n):
        C = rows[i] | (1 << i if fault == "self_common" else 0)
        rem, frontier, k2, e2, pieces, piece, paths = C, 0, 0, 0, [], 0, []
        while rem:
            if not frontier:
                if piece:
                    pieces.append(e2), paths.append(_longest_path(piece, rows) if fault == "longest_path" else 0)
                e2, piece, frontier = 0, 0, rem & -rem
            at = (frontier & -frontier).bit_length() - 1
            frontier &= ~(1 << at)
            rem &= ~(1 << at)
            piece |= 1 << at
            to = rows[at] & C
            deg = bin(to).count("1")
            k2, e2 = k2 + deg, e2 + deg
            frontier |= to & rem
        if piece:
            pieces.append(e2), paths.append(_longest_path(piece, rows) if fault == "longest_path" else 0)
        k = k2 if fault == "bonds_twice" else k2 // 2
        if fault == "half_round_twice" and n % 2 == 0:                     # the pairs half a ring apart counted once more
            k += sum(1 for u in range(n // 2) if C >> u & 1 and C >> (u + n // 2) & 1 and rows[u] >> (u + n // 2) & 1)
        halves = [e // 2 for e in pieces]
        l = 0 if not halves else halves[0] if fault == "first_component" else max(paths) if fault == "longest_path" else max(halves)
        sigs.append((bin(C).count("1"), k, l))
    if fault == "bcc_at_12":                                               # bcc looked for among the centres of 12, like the other types
        kind = R.classify(sigs)
        kind = 0 if kind == 3 else 3 if len(sigs) == 12 and all(s in ((6, 6, 6), (4, 4, 4)) for s in sigs) else kind
    else:
        kind = R.classify(sigs)
    return kind, [R.pack(*s) for s in sigs]


def model(positions, box, groups, r_cut, step=1, fault=None):
    """the dict of a call as the stated arithmetic gives it.  Faults: FAULTS"""
    S = len(groups)
    rc = A.cutoffs(r_cut, S)
    if fault == "one_cutoff":
        rc = np.full_like(rc, rc.max())
    frames = []
    for near in near32(positions, box, groups, rc, step):
        n_a = near.shape[0]
        count, types, words = near.sum(axis=1).astype(np.int32), np.zeros(n_a, np.int32), np.full((n_a, CAPACITY), NO_BOND, np.uint32)
        for a in range(n_a):
            nb = np.flatnonzero(near[a])
            if nb.size > CAPACITY:
                if fault != "first_64":
                    types[a] = -1
                    continue
                nb = nb[:CAPACITY]
            sub = near[np.ix_(nb, nb)]
            rows = [sum(1 << int(j) for j in np.flatnonzero(r)) for r in sub]
            types[a], w = centre_model(rows, nb.size, fault)
            words[a, :nb.size] = w
        frames.append((count, types, words))
    return with_groups(result_of(frames, groups), groups)


# ---- from the engine's own lists ----------------------------------------------------------------------------------------------
def from_lists(count, lists):
    """(types, words) of one origin from psa_debug_neighbour_lists' (count (n_a,), lists (n_a, 64)), integers only: u and v are
    bonded when either lists the other.  A truncated atom's list holds its first 64: a pair of two truncated atoms could not be
    decided and is refused"""
    held = [set(int(b) for b in lists[a, :min(int(count[a]), CAPACITY)]) for a in range(len(count))]
    cut = [int(count[a]) > CAPACITY for a in range(len(count))]

    def bonded(u, v):
        assert not (cut[u] and cut[v]), "a pair of two truncated atoms"
        return v in held[u] or u in held[v]
    return R.analyse([sorted(h) for h in held], count, bonded)


# ---- closed forms: what the counts must be, from the lattices alone -----------------------------------------------------------
def closed_inputs(name):
    """(positions, box, groups, r_cut) of a closed form; the nearest pair lies 10 % or more from the cut-off"""
    if name == "fcc":
        return order_cases.fcc_block(), Q.CUBIC, [np.arange(256)], 4.64
    if name == "bcc":
        return order_cases.bcc_block(), Q.CUBIC, [np.arange(128)], 6.55
    if name == "hcp":
        pos, box = qlm_cases.hcp_block()
        return pos, box, [np.arange(64)], 3.6
    if name == "ico":
        return qlm_cases.icosahedral_cluster(), Q.CUBIC, [np.arange(13)], 3.5
    pos, groups = Q.diamond(2)
    return pos, Q.CUBIC, groups, 2.8


# name: (atoms, the type of every atom, per atom the signatures and how many bonds have each)
CLOSED = {"fcc": (256, 1, {(4, 2, 1): 12}), "bcc": (128, 3, {(6, 6, 6): 8, (4, 4, 4): 6}), "hcp": (64, 2, {(4, 2, 1): 6, (4, 2, 2): 6}),
          "diamond": (512, 0, {(0, 0, 0): 4})}


def closed_form_holds(name, res):
    """does the result of a call with per-atom rows on `closed_inputs(name)` hold the closed form?"""
    t, w = np.asarray(res["types"]), np.asarray(res["bond_signatures"])
    table = np.asarray(res["signature_counts"]).sum(axis=0)
    if res["signature_outside"].any() or res["truncated"].any():
        return False
    if name == "ico":                                                      # the centre is ico with 12 x (5,5,5), the 12 vertices other
        return (t.tolist() == [[4] + [0] * 12] and np.all(w[0, 0, :12] == R.pack(5, 5, 5)) and np.all(w[0, 0, 12:] == NO_BOND)
                and res["type_counts"][0, 0].tolist() == [12, 0, 0, 0, 1] and int(table[5, 5, 5]) == 24 and np.all(w[0, 1:, 0] == R.pack(5, 5, 5)) and   # (a vertex's bond to the centre too)
                 np.all(res["n"][0] == [12] + [6] * 12))
    atoms, kind, sigs = CLOSED[name]
    n_o = t.shape[0]
    ok = t.shape == (n_o, atoms) and np.all(t == kind) and int(res["type_counts"][:, :, kind].sum()) == n_o * atoms
    ok = ok and int(table.sum()) == n_o * atoms * sum(sigs.values()) and np.all(np.asarray(res["n"]) == sum(sigs.values()))
    for s, per in sigs.items():
        ok = ok and int(table[s]) == n_o * atoms * per and np.all((w == R.pack(*s)).sum(axis=2) == per)
    return bool(ok)
