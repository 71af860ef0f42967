"""float64 reference of the common-neighbour tests, by the definition of include/psa_hip.h and nothing else: the minimum image
of every ordered pair by the image SEARCH of tests/pair64.py, neighbours and the bonds among them by r < r_cut, signatures by
plain graph code over sets (a depth-first search for the components) -- no bit mask, no rounds, nothing shared with the route."""
import numpy as np

import angle64 as A

CAPACITY = A.CAPACITY
NO_BOND = 0xFFFFFFFF
TYPES = ("other", "fcc", "hcp", "bcc", "ico")
TABLE = (8, 16, 16)


def pack(j, k, l):
    """the word of bond_signatures: j | k << 8 | l << 16, k and l clamped to 255"""
    return int(j) | min(int(k), 255) << 8 | min(int(l), 255) << 16


def signature(common, bonded):
    """(j, k, l) of a bond whose common neighbours are `common` (a list), `bonded(u, v)` saying which of them are bonded: their
    number, the bonds among them, the bonds of the largest connected component of that graph"""
    edges = [(u, v) for i, u in enumerate(common) for v in common[i + 1:] if bonded(u, v)]
    around = {u: set() for u in common}
    for u, v in edges:
        around[u].add(v), around[v].add(u)
    seen, largest = set(), 0
    for u in common:
        if u in seen:
            continue
        piece, stack = {u}, [u]
        while stack:
            for v in around[stack.pop()]:
                if v not in piece:
                    piece.add(v), stack.append(v)
        seen |= piece
        largest = max(largest, sum(1 for a, b in edges if a in piece))
    return len(common), len(edges), largest


def classify(sigs):
    """the type code of a centre whose bonds have the signatures `sigs` (a list of triples)"""
    n = len(sigs)
    of = lambda s: sum(1 for t in sigs if tuple(t) == s)                     # noqa: E731
    if n == 12 and of((4, 2, 1)) == 12:
        return 1
    if n == 12 and of((4, 2, 1)) == 6 and of((4, 2, 2)) == 6:
        return 2
    if n == 14 and of((6, 6, 6)) == 8 and of((4, 4, 4)) == 6:
        return 3
    if n == 12 and of((5, 5, 5)) == 12:
        return 4
    return 0


def analyse(lists, count, bonded):
    """per-atom results of one origin from every centre's neighbours `lists[a]` (ascending list positions; of a truncated centre
    whatever is known), the true counts and the adjacency: (types (n_a,) int32, words (n_a, 64) uint32)"""
    n_a = len(lists)
    types, words = np.zeros(n_a, np.int32), np.full((n_a, CAPACITY), NO_BOND, np.uint32)
    for a in range(n_a):
        if count[a] > CAPACITY:
            types[a] = -1
            continue
        nb = [int(b) for b in lists[a]]
        sigs = [signature([c for c in nb if c != b and bonded(b, c)], bonded) for b in nb]
        types[a] = classify(sigs)
        for i, s in enumerate(sigs):
            words[a, i] = pack(*s)
    return types, words


def frame(frame_positions, box, groups, r_cut):
    """(n (n_a,) int32, types, words, per atom the set of its neighbours) of one frame by the definition"""
    S = len(groups)
    rc = A.cutoffs(r_cut, S)
    atoms, spec = A.species_of(groups)
    if atoms.size == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, CAPACITY), np.uint32), []
    _, _, r = A.frame_pairs(frame_positions, box, atoms)
    near = (r < rc[spec[:, None], spec[None, :]]) & ~np.eye(atoms.size, dtype=bool)
    around = [set(np.flatnonzero(row).tolist()) for row in near]
    count = near.sum(axis=1).astype(np.int32)
    types, words = analyse([sorted(s) for s in around], count, lambda u, v: v in around[u])
    return count, types, words, around
