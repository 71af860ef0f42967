"""float64 reference of the adaptive common-neighbour tests, by the definition at psa_adaptive_common_neighbours in
include/psa_hip.h and nothing else: the minimum image of every ordered pair by the image SEARCH of tests/pair64.py
(angle64.frame_pairs), candidates by r < r_cut, a stable sort of the candidates by distance, K exact, the members' bonds by
r_uv < r_loc, signatures and types by the plain graph code of tests/cna64.py -- no rank counting, no mask, no rounds, nothing
shared with the route."""
import numpy as np

import angle64 as A
import cna64 as R

CAPACITY = A.CAPACITY
NO_BOND = R.NO_BOND
MEMBERS_A, MEMBERS = 12, 14
K = (1.0 + np.sqrt(2.0)) / 2.0
WEIGHT = 2.0 / np.sqrt(3.0)


def local_cutoff(rho, test):
    """r_A of the 12 ascending distances `rho`, or r_B of the 14"""
    if test == "A":
        return K * float(np.sum(rho[:MEMBERS_A])) / MEMBERS_A
    return K * (float(np.sum(rho[:8])) * WEIGHT + float(np.sum(rho[8:MEMBERS]))) / MEMBERS


def run_test(members, r, r_loc):
    """(type code, the signatures of the bonds centre-member in the members' order) of one test on the pair distances r"""
    bonded = lambda u, v: r[u, v] < r_loc                                    # noqa: E731
    sigs = [R.signature([c for c in members if c != b and bonded(b, c)], bonded) for b in members]
    return R.classify(sigs), sigs


def centre(a, cand, r):
    """(type, r_loc, the members by rank, their signatures) of centre a with the candidates `cand` (ascending list positions,
    12 to 64 of them)"""
    order = cand[np.argsort(r[a, cand], kind="stable")]
    members = [int(b) for b in order[:MEMBERS_A]]
    r_loc = local_cutoff(r[a, order], "A")
    kind, sigs = run_test(members, r, r_loc)
    if kind == 0 and cand.size >= MEMBERS:
        members = [int(b) for b in order[:MEMBERS]]
        r_loc = local_cutoff(r[a, order], "B")
        kind, sigs = run_test(members, r, r_loc)
    return kind, r_loc, members, sigs


def frame(frame_positions, box, groups, r_cut):
    """(n (n_a,) int32, types (n_a,) int32, cutoffs (n_a,) float64, nearest (n_a, 14) int32, words (n_a, 14) uint32, the pair
    distances r (n_a, n_a), the candidates (n_a, n_a) bool) of one frame by the definition"""
    S = len(groups)
    rc = A.cutoffs(r_cut, S)
    atoms, spec = A.species_of(groups)
    n_a = atoms.size
    types, cuts = np.zeros(n_a, np.int32), np.full(n_a, np.nan)
    nearest, words = np.full((n_a, MEMBERS), -1, np.int32), np.full((n_a, MEMBERS), NO_BOND, np.uint32)
    if n_a == 0:
        return np.zeros(0, np.int32), types, cuts, nearest, words, np.zeros((0, 0)), np.zeros((0, 0), bool)
    _, _, r = A.frame_pairs(frame_positions, box, atoms)
    near = (r < rc[spec[:, None], spec[None, :]]) & ~np.eye(n_a, dtype=bool)
    count = near.sum(axis=1).astype(np.int32)
    for a in range(n_a):
        if count[a] > CAPACITY:
            types[a] = -1
        elif count[a] >= MEMBERS_A:
            types[a], cuts[a], members, sigs = centre(a, np.flatnonzero(near[a]), r)
            nearest[a, :len(members)] = members
            words[a, :len(members)] = [R.pack(*s) for s in sigs]
    return count, types, cuts, nearest, words, r, near
