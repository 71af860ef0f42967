"""Support of the cluster tests: a host union-find (NumPy and pure Python only) that turns `count`, `list`, `solid`, `masks` and
`link` into the labels, the sizes and every statistic of the definition in psa_amd/clusters.py; `model`, the exact twin of the
whole call -- qlm_cases.model for Q, n and xi, the twin's neighbour lists and bond masks by the same loops --; graph families;
and a few deliberate faults that show the tests can fail.  Everything is integers: every comparison is exact."""
import numpy as np

import angle64 as A
import pair64 as R
import pair_cases as P
import qlm_cases as C

CAPACITY = C.CAPACITY
ROW_WORDS = CAPACITY + 1 + 4
FAULTS = ("largest_member", "both_lists", "left_out_solid", "overflow_off_by_one", "link_ignored")


# ---- the union-find -----------------------------------------------------------------------------------------------------
def solid_of(xi, min_connections, fault=None):
    """(…) bool: xi >= min_connections; a left-out centre (xi = -1) is never solid"""
    xi = np.asarray(xi)
    return (xi >= min_connections) | ((xi < 0) if fault == "left_out_solid" else False)


def edges_of(count, lists, solid, masks=None, link=0, fault=None):
    """the set of joined pairs (a, b), a < b, of one origin: both solid, b in a's list or a in b's; with link 1 the mask bit of
    the list position that holds the pair must be set"""
    n_a = len(count)
    use = link == 1 and fault != "link_ignored"
    held = set()
    for a in range(n_a):
        for s in range(int(count[a])):
            b = int(lists[a][s])
            if use and not (int(masks[a]) >> s) & 1:
                continue
            held.add((a, b))
    out = set()
    for a, b in held:
        if a == b or not (solid[a] and solid[b]):
            continue
        if fault == "both_lists" and (b, a) not in held:
            continue
        out.add((min(a, b), max(a, b)))
    return out


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def labels_of(n_a, solid, edges, fault=None):
    """(n_a,) int64: the smallest member of every solid atom's component, -1 for the others"""
    parent = list(range(n_a))
    for a, b in edges:
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    lab = np.array([_find(parent, a) if solid[a] else -1 for a in range(n_a)], np.int64)
    if fault == "largest_member":
        for root in np.unique(lab[lab >= 0]):
            lab[lab == root] = np.flatnonzero(lab == root).max()
    return lab


def statistics(labels, n_sizes, fault=None):
    """every statistic of the definition from labels (n_o, n_a): the dict `Engine.debug_cluster_labels` returns"""
    labels = np.asarray(labels, np.int64)
    n_o, n_a = labels.shape
    out = dict(size_counts=np.zeros(n_sizes + 2, np.uint64), large_atoms=0, n_solid=np.zeros(n_o, np.int32), n_clusters=np.zeros(n_o, np.int32),
               largest=np.zeros(n_o, np.int32), largest_label=np.full(n_o, -1, np.int32), labels=labels.astype(np.int32),
               size_atoms=np.zeros((n_o, n_a), np.int32))
    exact = n_sizes - 1 if fault == "overflow_off_by_one" else n_sizes
    for o in range(n_o):
        lab = labels[o]
        names, sizes = np.unique(lab[lab >= 0], return_counts=True)
        size_of = dict(zip(names.tolist(), sizes.tolist()))
        out["size_atoms"][o] = [size_of.get(int(x), 0) for x in lab]
        out["n_solid"][o], out["n_clusters"][o] = int((lab >= 0).sum()), names.size
        if names.size:
            out["largest"][o] = sizes.max()
            out["largest_label"][o] = names[sizes == sizes.max()].min()
        for s in sizes.tolist():
            if s <= exact:
                out["size_counts"][s] += np.uint64(1)
            else:
                out["size_counts"][n_sizes + 1] += np.uint64(1)
                out["large_atoms"] += s
    return out


def components(count, lists, solid, masks=None, link=0, n_sizes=256, fault=None):
    """the graph passes on the host: count (n_o, n_a), lists (n_o, n_a, 64), solid (n_o, n_a), masks (n_o, n_a) or None (all
    ones) -> the dict of `statistics`"""
    count, lists, solid = np.asarray(count), np.asarray(lists), np.asarray(solid).astype(bool)
    n_o, n_a = count.shape
    masks = np.full((n_o, n_a), 2 ** 64 - 1, np.uint64) if masks is None else np.asarray(masks, np.uint64)
    labels = np.full((n_o, n_a), -1, np.int64)
    for o in range(n_o):
        labels[o] = labels_of(n_a, solid[o], edges_of(count[o], lists[o], solid[o], masks[o], link, fault), fault)
    return statistics(labels, n_sizes, fault)


def closure_labels(n_a, solid, edges):
    """the same labels by brute force: the transitive closure of the adjacency matrix by repeated squaring"""
    reach = np.eye(n_a, dtype=bool)
    for a, b in edges:
        reach[a, b] = reach[b, a] = True
    for _ in range(max(1, int(np.ceil(np.log2(max(n_a, 2)))))):
        reach = reach | ((reach.astype(np.int64) @ reach.astype(np.int64)) > 0)
    return np.array([int(np.flatnonzero(reach[a]).min()) if solid[a] else -1 for a in range(n_a)], np.int64)


def same_partition(a, b):
    """do two label rows name the same partition (and the same non-members)?"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = set(zip(a[a >= 0].tolist(), b[b >= 0].tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


# ---- graphs --------------------------------------------------------------------------------------------------------------
def graph(n_a, adjacency):
    """(count (1, n_a) int32, lists (1, n_a, 64) int32) of {a: [b, ...]}: what a lists, in the order given"""
    count, lists = np.zeros((1, n_a), np.int32), np.full((1, n_a, CAPACITY), -1, np.int32)
    for a, nb in adjacency.items():
        count[0, a] = len(nb)
        lists[0, a, :len(nb)] = nb
    return count, lists


def random_graph(n_a, seed, degree=3.0, symmetric=True):
    """a random graph of mean degree `degree` (no list beyond 64), symmetric lists or each edge listed by one end only"""
    rng = np.random.default_rng(seed)
    adjacency = {a: [] for a in range(n_a)}
    for _ in range(int(degree * n_a / 2)):
        a, b = (int(x) for x in rng.integers(0, n_a, 2))
        if a == b or b in adjacency[a] or a in adjacency[b] or len(adjacency[a]) >= CAPACITY or len(adjacency[b]) >= CAPACITY:
            continue
        adjacency[a].append(b)
        if symmetric:
            adjacency[b].append(a)
    count, lists = graph(n_a, adjacency)
    return count, lists, (rng.uniform(size=(1, n_a)) < 0.8)


def chain(n_a, end="low", order=None):
    """the chain 0 - 1 - ... - n_a - 1 (`order`: the columns that stand for them), every edge listed by its low or its high end"""
    order = np.arange(n_a) if order is None else np.asarray(order)
    adjacency = {int(order[i]): [int(order[i + 1])] for i in range(n_a - 1)} if end == "low" else \
        {int(order[i + 1]): [int(order[i])] for i in range(n_a - 1)}
    return graph(n_a, adjacency)


# ---- the twin of the whole call ------------------------------------------------------------------------------------------
def twin_lists(positions, box, groups, r_cut, step):
    """per origin the list of every centre's neighbours (all of them, ascending) by qlm_cases.model's float32 chain"""
    S = len(groups)
    rc = A.cutoffs(r_cut, S)
    atoms, spec = A.species_of(groups)
    n = atoms.size
    c = P.fractions_model(positions, box)
    h = R.box64(box)[0].astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(rc > 0.0, 1.0 / rc, 0.0).astype(np.float32)[spec[:, None], spec[None, :]]
    out = []
    for fr in range(0, np.shape(positions)[0], step):
        f = c[fr][atoms]
        e = (f[None, :, :] - f[:, None, :]).astype(np.float32)
        e = e - np.rint(e)
        d = np.stack([P._fma32(e[..., 2], h[2, k], P._fma32(e[..., 1], h[1, k], e[..., 0] * h[0, k])) for k in range(3)], -1)
        r2 = P._fma32(d[..., 2], d[..., 2], P._fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
        near = (np.sqrt(r2) * inv < np.float32(1.0)) & (inv > 0) & ~np.eye(n, dtype=bool)
        out.append([np.flatnonzero(near[a]) for a in range(n)])
    return out


def bond_mask(q, a, nb, l, thr2):
    """the ballot of the solid-like bonds of centre a over its list nb, by qlm_cases.model's loop; q (n_a, l + 1, 2) int64"""
    va = q[a].astype(np.float64) * (1.0 / C.ONE)
    A2, mask = C.norm2_model(va), 0
    for s, b in enumerate(nb):
        vb = q[b].astype(np.float64) * (1.0 / C.ONE)
        D = np.float64(0.0)
        for k in range(l + 1):
            t = va[k, 0] * vb[k, 0] + va[k, 1] * vb[k, 1]
            D = D + (2.0 * t if k else t)
        if D > 0.0 and D * D > thr2 * (A2 * C.norm2_model(vb)):
            mask |= 1 << s
    return mask


def model(positions, box, groups, r_cut, step, solid_l=6, threshold=0.7, min_connections=7, link=0, n_sizes=256, fault=None):
    """what `Engine.solid_clusters(..., per_atom=True)` returns, by the twin: the dict of `statistics` plus connections (xi), n,
    bond_masks, count / lists (the graph) and species_rows (S, 69) with the four left-out kinds summed into the first"""
    got = C.model(positions, box, groups, r_cut, step, [solid_l], solid_l, threshold)
    xi, n = got["xi"], got["n"]
    n_o, n_a = xi.shape
    lists_of = twin_lists(positions, box, groups, r_cut, step) if n_a else [[] for _ in range(n_o)]
    thr2 = np.float64(threshold) * np.float64(threshold)
    count, lists = np.zeros((n_o, n_a), np.int32), np.full((n_o, n_a, CAPACITY), -1, np.int32)
    masks = np.zeros((n_o, n_a), np.uint64)
    for o in range(n_o):
        for a in range(n_a):
            nb = lists_of[o][a]
            assert nb.size == n[o, a]
            count[o, a] = min(nb.size, CAPACITY)
            lists[o, a, :count[o, a]] = nb[:CAPACITY]
            if xi[o, a] >= 0:
                masks[o, a] = bond_mask(got["q"][o], a, nb, solid_l, thr2)
                assert bin(int(masks[o, a])).count("1") == xi[o, a]
    solid = solid_of(xi, min_connections, fault)
    count_used = np.where(n > CAPACITY, 0, count)                           # a truncated centre is never solid: its list is not read
    out = components(count_used, lists, solid, masks, link, n_sizes, fault)
    sizes = [len(g) for g in groups]
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    rows = np.zeros((len(groups), ROW_WORDS), np.int64)
    for s in range(len(groups)):
        part = xi[:, start[s]:start[s + 1]].ravel()
        rows[s, :CAPACITY + 1] = np.bincount(part[part >= 0], minlength=CAPACITY + 1)
        rows[s, CAPACITY + 1] = (part < 0).sum()
    out.update(connections=xi.astype(np.int32), n=n.astype(np.int32), bond_masks=masks, count=count, lists=lists, species_rows=rows, solid=solid)
    return out


def fold_left_out(rows):
    """the route's species rows with the four left-out counters summed into the first, as `model` files them"""
    rows = np.asarray(rows).astype(np.int64).copy()
    rows[:, CAPACITY + 1] = rows[:, CAPACITY + 1:].sum(axis=1)
    rows[:, CAPACITY + 2:] = 0
    return rows


def identities(res):
    """the identities of the definition on a dict of the engine's or the twin's (with size_atoms where it is there)"""
    counts = np.asarray(res["size_counts"]).astype(np.int64)
    n_sizes = counts.size - 2
    ok = counts[0] == 0
    ok = ok and int((np.arange(1, n_sizes + 1) * counts[1:n_sizes + 1]).sum()) + int(res["large_atoms"]) == int(np.asarray(res["n_solid"], np.int64).sum())
    ok = ok and int(counts.sum()) == int(np.asarray(res["n_clusters"], np.int64).sum())
    if res.get("size_atoms") is not None and np.asarray(res["size_atoms"]).size:
        ok = ok and np.array_equal(np.asarray(res["size_atoms"]).max(axis=1), res["largest"])
    return bool(ok)


KEYS = ("size_counts", "large_atoms", "n_solid", "n_clusters", "largest", "largest_label", "labels", "size_atoms")


def differs(a, b, keys=KEYS):
    """the keys under which two results differ"""
    return [k for k in keys if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
