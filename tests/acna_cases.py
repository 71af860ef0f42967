"""Inputs of the adaptive common-neighbour tests, the comparison the GPU test makes, the centres that comparison leaves out, and
a NumPy float32 twin of the arithmetic stated at psa_adaptive_common_neighbours in include/psa_hip.h with the planted faults
the host test holds outside the comparison.

The comparison.  Everything after the adjacency is integers, so the route must give the float64 reference's numbers exactly
wherever its decisions are the reference's.  The route's counts must be the sums of its own rows, exactly; its rows (types, n,
nearest, bond_signatures) the reference's on every centre that is not excluded, its cut-off the reference's within the
relative error derived below; where no centre is excluded the counts are compared directly too.  Truncated centres stay in
the comparison.

A centre is EXCLUDED when a decision of its own lies within tolerance in the reference, evaluated wherever n permits the test,
whether or not test B runs.  u = 2^-24; t(p) is `pair_cases.tolerance` of the pair p at dr = 1, the absolute tolerance of its
float32 length (the chain's roundings and the root among it):
  * a candidate or a near miss b of a with |r_ab / r_cut - 1| <= t(ab) / r_cut;
  * the members' boundary: rho_12 - rho_11 <= t(11) + t(12) (n >= 13), rho_14 - rho_13 <= t(13) + t(14) (n >= 15) -- the rank
    compares r2 exactly, and r2's relative error is twice the length's, so the lengths' tolerances decide;
  * a member pair (u, v) with |d_uv / r_loc - 1| <= t(uv) / r_loc + E_loc, the pair's tolerance at dr = r_loc plus the relative
    error of r_loc.  E_loc counted from the definition: L is a sum of positive lengths, so its relative error is at most the
    largest of the members' t(k) / rho_k, plus one rounding of every root (u, on every term: u), plus every add on a partial sum
    below L (test A: 11 adds, 11 u; test B: 7 + 5 + 1 = 13 adds, 13 u), the weight (B: its own rounding and the product's, 2 u
    on a part of L), the scale (its own rounding and the product's, 2 u), the reciprocal (u):
        E_loc(A) = max t / rho + (1 + 11 + 2 + 1) u = max t / rho + 15 u      E_loc(B) = max t / rho + (1 + 13 + 2 + 2 + 1) u = max t / rho + 19 u
    each times (1 + 2^-20) for the second order.  (t already holds the root's rounding: it is counted twice, on the safe side
    of an exclusion that the cap below keeps from hiding anything.)
  * the rank labels: the rows are indexed by rank, so two members next to each other in rank, of the ranks the centre's rows
    hold (0 .. 11; 0 .. 13 where test B ran last), with rho_{k+1} - rho_k <= t(k) + t(k + 1) may carry each other's label.
The share of excluded centres of a case may not exceed EXCLUDED_CAP; the inputs are chosen so that the reference excludes none.
`Reference.margin` is the least relative distance of any such decision from its edge, the tolerance taken off;
`Reference.clearance` the least ratio of a decision's distance to its tolerance: 4.57 on thermal fcc (seed 12; at seed 8 a
rank label lay inside the tolerance and one centre was excluded, above the cap), 4.92 on bcc, 2.70 on hcp, 1.80 on the gas --
of the gas seeds 0 .. 63 none reaches 3 (the best, 10 and 42, 2.9), the short legs of a gas making t / rho large, so its seed
11 stays.  The host test asserts these figures (test_acna_host.CLEARANCE).

The planted faults.  Eight of the nine lie outside this comparison on one of its four inputs.  The ninth, a tie dropped in
the rank, cannot: the thermal inputs hold no two candidates with the same r2 bit for bit.  It lies outside the closed form of
the perfect fcc lattice (`closed_form_holds`), where the 12 nearest are exactly tied."""
import numpy as np

import acna64 as R
import angle64 as A
import angle_cases as Q
import cna64
import order_cases
import pair64
import pair_cases as P
import persist_cases as C
import qlm_cases

CAPACITY = R.CAPACITY
NO_BOND = R.NO_BOND
MEMBERS_A, MEMBERS = R.MEMBERS_A, R.MEMBERS
EXCLUDED_CAP = order_cases.EXCLUDED_CAP
U32 = 2.0 ** -24
COUNTS = ("signature_counts", "signature_outside", "type_counts", "truncated", "short")
ROWS = ("types", "n", "nearest", "bond_signatures")
species, cutoffs, walk_split = C.species, C.cutoffs, C.walk_split
K12, K14, W32 = np.float32(R.K / 12.0), np.float32(R.K / 14.0), np.float32(R.WEIGHT)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def thermal(block, sigma, frames, seed):
    """`frames` frames of the lattice `block` (N, 3) with Gaussian noise of `sigma` added in float64, rounded to float32"""
    rng = np.random.default_rng(seed)
    return (np.asarray(block, np.float32).astype(np.float64)[None] + sigma * rng.standard_normal((frames,) + np.shape(block))).astype(np.float32)


# name: the four inputs of the comparison (the seeds and what they hold: DESIGN section 7)
CASES = ("fcc", "bcc", "hcp", "gas")


def case(name):
    """(positions (T, N, 3) float32, box, r_cut)"""
    if name == "fcc":
        return thermal(order_cases.fcc_block()[0], 0.30, 3, 12), Q.CUBIC, 6.0
    if name == "bcc":
        return thermal(order_cases.bcc_block()[0], 0.30, 4, 4), Q.CUBIC, 6.5
    if name == "hcp":
        pos, box = qlm_cases.hcp_block()
        return thermal(pos[0], 0.24, 6, 1), box, 4.6
    pos, box, _ = Q.family("triclinic257", seed=11)
    return pos, box, 6.5


OWN_TYPE = {"fcc": 1, "bcc": 3, "hcp": 2}


# ---- sums of the per-atom rows --------------------------------------------------------------------------------------------
def aggregate(n, types, words, groups):
    """the counts of a call from its per-atom rows n, types (n_o, n_a) and words (n_o, n_a, 14)"""
    S = len(groups)
    _, spec = A.species_of(groups)
    n_o = np.shape(types)[0]
    out = dict(signature_counts=np.zeros((S,) + cna64.TABLE, np.uint64), signature_outside=np.zeros(S, np.uint64),
               type_counts=np.zeros((n_o, S, len(cna64.TYPES)), np.uint64), truncated=np.zeros(S, np.uint64), short=np.zeros(S, np.uint64))
    for al in range(S):
        of = spec == al
        t = np.asarray(types)[:, of]
        out["truncated"][al] = int((t < 0).sum())
        out["short"][al] = int((np.asarray(n)[:, of] < MEMBERS_A).sum())
        for code in range(len(cna64.TYPES)):
            out["type_counts"][:, al, code] = (t == code).sum(axis=1)
        w = np.asarray(words)[:, of].ravel()
        w = w[w != NO_BOND].astype(np.int64)
        j, k, l = w & 255, (w >> 8) & 255, w >> 16
        inside = (j < cna64.TABLE[0]) & (k < cna64.TABLE[1]) & (l < cna64.TABLE[2])
        np.add.at(out["signature_counts"][al], (j[inside], k[inside], l[inside]), 1)
        out["signature_outside"][al] = int((~inside).sum())
    return out


def result_of(frames, groups):
    """the dict `Engine.adaptive_common_neighbours(per_atom=True)` returns, from per origin (n, types, cutoffs, nearest, words)"""
    n_a, n_o = sum(len(g) for g in groups), len(frames)
    n = np.array([f[0] for f in frames], np.int32).reshape(n_o, n_a)
    types = np.array([f[1] for f in frames], np.int32).reshape(n_o, n_a)
    cuts = np.array([f[2] for f in frames], np.float64).reshape(n_o, n_a)
    near = np.array([f[3] for f in frames], np.int32).reshape(n_o, n_a, MEMBERS)
    words = np.array([f[4] for f in frames], np.uint32).reshape(n_o, n_a, MEMBERS)
    return dict(aggregate(n, types, words, groups), types=types, n=n, cutoffs=cuts, nearest=near, bond_signatures=words, groups=groups)


# ---- the reference, the centres left out, what the inputs hold ------------------------------------------------------------------
class Reference:
    """every frame of a trajectory by tests/acna64.py, once: per frame the rows, the excluded centres (n_a,) bool, E_loc of the
    cut-off (n_a,); `margin`, `clearance` (see the module's docstring); `ran_b` the centres on which test B ran, `few` those
    with 12 or 13 candidates; `result(step)` the call's expected dict over the origins 0, step, ...; `excluded(step)`,
    `cut_tolerance(step)` (n_o, n_a)"""

    def __init__(self, positions, box, groups, r_cut):
        self.groups, self.frames, self.left_out, self.e_loc = groups, [], [], []
        self.margin, self.ran_b, self.few, self.clearance = np.inf, 0, 0, np.inf
        S = len(groups)
        rc = A.cutoffs(r_cut, S)
        atoms, spec = A.species_of(groups)
        n = atoms.size
        e64 = P.sigma_error(positions, box) if n else 0.0
        big = 1.0 + 2.0 ** -20
        for fr in positions:
            count, types, cuts, nearest, words, r, near = R.frame(fr, box, groups, r_cut)
            self.frames.append((count, types, cuts, nearest, words))
            out, e_loc = np.zeros(n, bool), np.zeros(n)
            if n == 0:
                self.left_out.append(out), self.e_loc.append(e_loc)
                continue
            e, d, _ = A.frame_pairs(fr, box, atoms)
            t = P.tolerance(e.reshape(-1, 3), d.reshape(-1, 3), r.ravel(), box, 1.0, e64).reshape(n, n)
            cut = rc[spec[:, None], spec[None, :]]
            on = (cut > 0.0) & ~np.eye(n, dtype=bool)
            safe = np.where(on, cut, 1.0)
            x = np.abs(r / safe - 1.0)
            out |= (on & (x <= t / safe)).any(axis=1)
            self.margin = min(self.margin, float((x - t / safe)[on].min()) if on.any() else np.inf)
            self.clearance = min(self.clearance, float((x / (t / safe))[on].min()) if on.any() else np.inf)
            for a in range(n):
                if not MEMBERS_A <= count[a] <= CAPACITY:
                    continue
                self.few += count[a] < MEMBERS
                self.ran_b += int(nearest[a, MEMBERS_A] >= 0)
                cand = np.flatnonzero(near[a])
                order = cand[np.argsort(r[a, cand], kind="stable")]
                rho, ta = r[a, order], t[a, order]
                for test, m, roundings in (("A", MEMBERS_A, 15), ("B", MEMBERS, 19)):
                    if count[a] < m:
                        continue
                    if count[a] > m:                                       # the members' boundary
                        gap, tol = rho[m] - rho[m - 1], ta[m] + ta[m - 1]
                        out[a] |= gap <= tol
                        self.margin = min(self.margin, float((gap - tol) / rho[m]))
                        self.clearance = min(self.clearance, float(gap / tol))
                    if test == "A" or nearest[a, MEMBERS_A] >= 0:         # the rank labels, of the ranks the rows hold
                        gaps, tols = np.diff(rho[:m]), ta[:m - 1] + ta[1:m]
                        out[a] |= bool((gaps <= tols).any())
                        self.margin = min(self.margin, float(((gaps - tols) / rho[1:m]).min()))
                        self.clearance = min(self.clearance, float((gaps / tols).min()))
                    r_loc = R.local_cutoff(rho, test)
                    err = (float((ta[:m] / rho[:m]).max()) + roundings * U32) * big
                    mem = order[:m]
                    u, v = np.triu_indices(m, 1)
                    duv, tuv = r[mem[u], mem[v]], t[mem[u], mem[v]]
                    edge = np.abs(duv / r_loc - 1.0) - (tuv / r_loc * big + err)
                    out[a] |= bool((edge <= 0.0).any())
                    self.margin = min(self.margin, float(edge.min()))
                    self.clearance = min(self.clearance, float((np.abs(duv / r_loc - 1.0) / (tuv / r_loc * big + err)).min()))
                    if (test == "B") == (nearest[a, MEMBERS_A] >= 0):    # the test that ran last: its cut-off's tolerance
                        e_loc[a] = err
            self.left_out.append(out), self.e_loc.append(e_loc)

    def result(self, step=1):
        return result_of(self.frames[::step], self.groups)

    def excluded(self, step=1):
        return np.array(self.left_out[::step], bool).reshape(len(self.frames[::step]), -1)

    def cut_tolerance(self, step=1):
        return np.array(self.e_loc[::step], np.float64).reshape(len(self.frames[::step]), -1)


def distinct_signatures(res):
    w = np.asarray(res["bond_signatures"]).ravel()
    return np.unique(w[w != NO_BOND]).size


def check(got, ref, excluded=None, cut_tolerance=None, what=""):
    """the comparison: got's counts are the sums of its own rows, and its rows are ref's on every centre not excluded (the counts
    too where none is), its cut-offs ref's within `cut_tolerance` (relative; None: 32 u); prints what differs"""
    shape = np.shape(ref["types"])
    out = np.zeros(shape, bool) if excluded is None else np.asarray(excluded, bool)
    bad = []
    if any(got.get(k) is None for k in ROWS + ("cutoffs",)):
        return False
    shapes = {"types": shape, "n": shape, "cutoffs": shape, "nearest": shape + (MEMBERS,), "bond_signatures": shape + (MEMBERS,)}
    if any(np.shape(got[k]) != s for k, s in shapes.items()):
        print(f"{what}: shapes {[np.shape(got[k]) for k in shapes]}")
        return False
    own = aggregate(got["n"], got["types"], got["bond_signatures"], ref["groups"])
    for k in COUNTS:
        if not np.array_equal(np.asarray(got[k]), own[k]):
            bad.append(f"{k} is not the sum of the rows")
        if not out.any() and not np.array_equal(np.asarray(got[k]), ref[k]):
            bad.append(f"{k} differs from the reference")
    if not np.array_equal((np.asarray(got["n"]) > CAPACITY), np.asarray(got["types"]) < 0):
        bad.append("types = -1 and n > 64 name different centres")
    for k in ROWS:
        if not np.array_equal(np.asarray(got[k])[~out], np.asarray(ref[k])[~out]):
            bad.append(f"{k} differs on {int((np.asarray(got[k])[~out] != np.asarray(ref[k])[~out]).sum())} cells")
    g, w = np.asarray(got["cutoffs"], np.float64)[~out], np.asarray(ref["cutoffs"], np.float64)[~out]
    tol = np.full(shape, 32.0 * U32)[~out] if cut_tolerance is None else np.asarray(cut_tolerance)[~out]
    if not np.array_equal(np.isnan(g), np.isnan(w)) or np.any(np.abs(g - w)[~np.isnan(w)] > (tol * w)[~np.isnan(w)]):
        bad.append("cutoffs differ")
    if bad:
        print(f"{what}: " + "; ".join(bad))
    return not bad


# ---- the twin ---------------------------------------------------------------------------------------------------------------
FAULTS = ("first_12", "mean_of_all", "r_cut_itself", "bcc_first", "no_weight", "thirteen", "leg_difference", "tie_dropped", "bonds_of_a")


def _sum32(values):
    """float32 adds in the order given, each rounded once"""
    s = np.float32(values[0])
    for v in values[1:]:
        s = np.float32(s + np.float32(v))
    return s


def geometry32(positions, box, groups, r_cut, step=1):
    """per origin (d (n, n, 3), r2 (n, n) float32 of the stated chain, the candidates (n, n) bool)"""
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
        out.append((d, r2, (np.sqrt(r2) * inv < np.float32(1.0)) & (inv > 0) & ~np.eye(n, dtype=bool)))
    return out


def _ranked(cand, s, fault):
    """the candidates by rank slot: slot rank(i) takes candidate i, in ascending i"""
    if fault == "first_12":
        return cand
    slots = np.full(cand.size, cand[0])
    for i in range(cand.size):
        rank = int((s < s[i]).sum()) + (0 if fault == "tie_dropped" else int((s[:i] == s[i]).sum()))
        slots[rank] = cand[i]                                              # a dropped tie: the later one overwrites, a slot stays stale
    return slots


def _test32(a, order, m, d, r2, test, r_cut, fault):
    """(type, r_loc, the m members, their signatures) of one test in float32"""
    members = [int(b) for b in order[:m]]
    rho = np.sqrt(r2[a, order]).astype(np.float32)
    if fault == "mean_of_all":
        r_loc = np.float32(_sum32(rho) * np.float32(R.K / rho.size))
    elif test == "A":
        r_loc = np.float32(_sum32(rho[:m]) * (np.float32(R.K / m) if fault == "thirteen" else K12))
    else:
        first = _sum32(rho[:8]) if fault == "no_weight" else np.float32(_sum32(rho[:8]) * W32)
        r_loc = np.float32(np.float32(first + _sum32(rho[8:MEMBERS])) * K14)
    if fault == "r_cut_itself":
        r_loc = np.float32(np.max(r_cut))
    inv = np.float32(1.0) / r_loc

    def bonded(u, v):
        if fault == "leg_difference":
            q = (d[a, v] - d[a, u]).astype(np.float32)
            s = P._fma32(q[2], q[2], P._fma32(q[1], q[1], q[0] * q[0]))
        else:
            s = r2[u, v]
        return bool(np.float32(np.sqrt(s)) * inv < np.float32(1.0))
    sigs = [cna64.signature([c for c in members if c != b and bonded(b, c)], bonded) for b in members]
    return cna64.classify(sigs), r_loc, members, sigs


def model(positions, box, groups, r_cut, step=1, fault=None):
    """the dict of a call as the stated arithmetic gives it.  Faults: FAULTS"""
    frames = []
    m_a = 13 if fault == "thirteen" else MEMBERS_A
    for d, r2, near in geometry32(positions, box, groups, r_cut, step):
        n_a = near.shape[0]
        count, types, cuts = near.sum(axis=1).astype(np.int32), np.zeros(n_a, np.int32), np.full(n_a, np.nan)
        nearest, words = np.full((n_a, MEMBERS), -1, np.int32), np.full((n_a, MEMBERS), NO_BOND, np.uint32)
        for a in range(n_a):
            if count[a] > CAPACITY:
                types[a] = -1
                continue
            if count[a] < MEMBERS_A:
                continue
            cand = np.flatnonzero(near[a])
            order = _ranked(cand, r2[a, cand], fault)
            can_b = cand.size >= MEMBERS
            if fault == "bcc_first" and can_b:
                done = _test32(a, order, MEMBERS, d, r2, "B", r_cut, fault)
                if done[0] != 3:
                    done = _test32(a, order, m_a, d, r2, "A", r_cut, fault)
            else:
                done = first = _test32(a, order, min(m_a, cand.size), d, r2, "A", r_cut, fault)
                if done[0] == 0 and can_b:
                    done = _test32(a, order, MEMBERS, d, r2, "B", r_cut, fault)
                    if fault == "bonds_of_a":
                        done = (done[0],) + first[1:]
            types[a], cuts[a], members, sigs = done
            nearest[a, :len(members)] = members
            words[a, :len(members)] = [cna64.pack(*s) for s in sigs]
        frames.append((count, types, cuts, nearest, words))
    return result_of(frames, groups)


# ---- closed forms: what the counts must be, from the lattices alone -----------------------------------------------------------
def closed_inputs(name):
    """(positions, box, groups, r_cut) of a closed form"""
    if name == "fcc":
        return order_cases.fcc_block(), Q.CUBIC, [np.arange(256)], 7.0
    if name == "bcc":
        return order_cases.bcc_block(), Q.CUBIC, [np.arange(128)], 8.3
    if name == "hcp":
        pos, box = qlm_cases.hcp_block()
        return pos, box, [np.arange(64)], 4.6
    if name == "ico":
        return qlm_cases.icosahedral_cluster(), Q.CUBIC, [np.arange(13)], 3.5
    pos, groups = Q.diamond(2)
    return pos, Q.CUBIC, groups, 2.8


# name: (atoms, candidates, the type of every atom, per atom the signatures and how many bonds have each)
CLOSED = {"fcc": (256, 42, 1, {(4, 2, 1): 12}), "bcc": (128, 26, 3, {(6, 6, 6): 8, (4, 4, 4): 6}),
          "hcp": (64, None, 2, {(4, 2, 1): 6, (4, 2, 2): 6}), "diamond": (512, 4, 0, {})}


def closed_form_holds(name, res):
    """does the result of a call with per-atom rows on `closed_inputs(name)` hold the closed form?"""
    t, w, n = np.asarray(res["types"]), np.asarray(res["bond_signatures"]), np.asarray(res["n"])
    table = np.asarray(res["signature_counts"]).sum(axis=0)
    if res["signature_outside"].any() or res["truncated"].any():
        return False
    if name == "ico":                                                      # the centre is ico, the 12 vertices have 6 candidates: short
        return (t.tolist() == [[4] + [0] * 12] and np.all(w[0, 0, :12] == cna64.pack(5, 5, 5)) and np.all(w[0, 0, 12:] == NO_BOND)
                and np.all(w[0, 1:] == NO_BOND) and res["type_counts"][0, 0].tolist() == [12, 0, 0, 0, 1] and int(table.sum()) == 12
                and int(table[5, 5, 5]) == 12 and n[0].tolist() == [12] + [6] * 12 and res["short"].tolist() == [12]
                and sorted(res["nearest"][0, 0, :12].tolist()) == list(range(1, 13)) and np.all(res["nearest"][0, 1:] == -1)
                and np.all(np.isnan(res["cutoffs"][0, 1:])))
    atoms, cands, kind, sigs = CLOSED[name]
    n_o, bonds = t.shape[0], sum(sigs.values())
    ok = t.shape == (n_o, atoms) and np.all(t == kind) and int(res["type_counts"][:, :, kind].sum()) == n_o * atoms
    ok = ok and int(table.sum()) == n_o * atoms * bonds and (cands is None or np.all(n == cands))
    ok = ok and int(np.sum(res["short"])) == (n_o * atoms if name == "diamond" else 0)
    ok = ok and np.all((np.asarray(res["nearest"]) >= 0).sum(axis=2) == bonds) and np.all((w != NO_BOND).sum(axis=2) == bonds)
    for s, per in sigs.items():
        ok = ok and int(table[s]) == n_o * atoms * per and np.all((w == cna64.pack(*s)).sum(axis=2) == per)
    return bool(ok)
