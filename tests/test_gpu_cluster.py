"""The solid-like clusters on the GPU (psa_solid_clusters, psa_debug_cluster_labels, their Engine methods and the calculator
method).  Everything is integers and every comparison is exact: the graph passes alone against the host union-find of
tests/cluster_cases.py -- tile and item edges, deep chains listed from either end and permuted, a star, a full clique, joined
chains, singletons, nothing solid, solid atoms among non-solid neighbours, lists that are not symmetric, masks that cut a
chain, the last exact slot and the overflow slot of the size histogram, three graphs in one call, every refusal --; the whole
call against the twin (cluster_cases.model) on random walks with one and two species and both links; agreement with
psa_local_order and psa_debug_neighbour_lists; known structures; budgets, repeats and permutations bit for bit; no trace in
later calls; the calculator."""
import functools

import numpy as np
import pytest

import angle_cases as Q
import cluster_cases as K
import qlm_cases as C
import scratch_cases as S
from engine_state import reset

pytestmark = pytest.mark.gpu

PER_ORIGIN = 1040 + 16 * 7 + 20                                            # work bytes per atom and origin, solid_l = 6
ATOM_KEYS = ("labels", "size_atoms", "connections", "n", "bond_masks")


@pytest.fixture(autouse=True)
def _clean(engine):
    reset(engine)
    yield
    reset(engine)


@pytest.fixture(scope="module", autouse=True)
def _forget(engine):
    yield
    engine.invalidate()


def _resident(engine, pos):
    from psa_amd import _hip
    engine.ensure_resident(_hip.SLOT_POSITIONS, pos)


def _listing(kind, groups):
    return None if kind == "one" else [np.asarray(g, np.int32) for g in groups]


# ---- 1. the graph passes alone ------------------------------------------------------------------------------------------------
def _graph_held(engine, count, lists, solid, masks=None, link=0, n_sizes=256, what=""):
    want = K.components(count, lists, solid, masks, link, n_sizes)
    got = engine.debug_cluster_labels(count, lists, solid, masks, link, n_sizes)
    assert got["labels"].dtype == np.int32 and got["size_counts"].dtype == np.uint64 and got["size_counts"].shape == (n_sizes + 2,)
    assert K.differs(got, want) == [], what
    assert K.identities(got), what
    return got


@pytest.mark.parametrize("n_a", [1, 63, 64, 65, 255, 256, 257])
def test_random_graphs_at_the_tile_and_item_edges(engine, n_a):
    count, lists, solid = K.random_graph(n_a, 100 + n_a)
    got = _graph_held(engine, count, lists, solid, what=f"random {n_a}")
    assert n_a < 63 or (got["n_clusters"][0] >= 2 and (got["labels"] < 0).any() and got["largest"][0] >= 3)


@pytest.mark.parametrize("how", ["low", "high", "permuted"])
def test_deep_chains(engine, how):
    """0 - 1 - ... - 4096 listed from one end: deep trees, and the find-step bound (n_a) must not trip"""
    n_a = 4097
    order = np.random.default_rng(5).permutation(n_a) if how == "permuted" else None
    count, lists = K.chain(n_a, "high" if how == "high" else "low", order)
    got = _graph_held(engine, count, lists, np.ones((1, n_a), bool), n_sizes=4096, what=how)
    assert got["n_clusters"][0] == 1 and got["largest"][0] == n_a and got["largest_label"][0] == 0 and got["large_atoms"] == n_a


def test_star_clique_and_joined_chains(engine):
    star = {64: list(range(64)), **{a: [64] for a in range(64)}}           # the hub is the last column: 64 leaves
    got = _graph_held(engine, *K.graph(65, star), np.ones((1, 65), bool), what="star")
    assert got["labels"].tolist() == [[0] * 65]
    clique = {a: [b for b in range(65) if b != a] for a in range(65)}       # every list is full
    got = _graph_held(engine, *K.graph(65, clique), np.ones((1, 65), bool), what="clique")
    assert got["size_atoms"].tolist() == [[65] * 65]
    two = {a: [a + 1] for a in range(499)}
    two.update({a: [a + 1] for a in range(500, 999)})
    two[999] = [499]                                                        # one edge between the last columns of two chains of 500
    got = _graph_held(engine, *K.graph(1000, two), np.ones((1, 1000), bool), n_sizes=1000, what="joined chains")
    assert got["n_clusters"][0] == 1 and got["size_counts"][1000] == 1
    del two[999]
    got = _graph_held(engine, *K.graph(1000, two), np.ones((1, 1000), bool), n_sizes=500, what="two chains")
    assert got["largest_label"][0] == 0 and got["size_counts"][500] == 2 and sorted(set(got["labels"][0].tolist())) == [0, 500]


def test_degenerate_graphs(engine):
    count, lists, _ = K.random_graph(130, 3)
    none = _graph_held(engine, count, lists, np.zeros((1, 130), bool), what="no solid atom")
    assert none["n_solid"][0] == 0 and none["largest"][0] == 0 and none["largest_label"][0] == -1 and np.all(none["labels"] == -1)
    empty = K.graph(70, {})
    single = _graph_held(engine, *empty, np.ones((1, 70), bool), what="singletons")
    assert single["size_counts"][1] == 70 and single["largest_label"][0] == 0 and single["labels"][0].tolist() == list(range(70))
    solid = np.zeros((1, 130), bool)
    solid[0, ::3] = True
    adjacency = {a: [b for b in (a - 1, a + 1) if 0 <= b < 130] for a in range(130)}     # a solid atom's neighbours are not solid
    lone = _graph_held(engine, *K.graph(130, adjacency), solid, what="non-solid neighbours")
    assert lone["n_clusters"][0] == lone["n_solid"][0] == 44 and lone["largest"][0] == 1


def test_lists_that_are_not_symmetric(engine):
    for n_a, seed in ((65, 1), (257, 2)):
        count, lists, solid = K.random_graph(n_a, seed, symmetric=False)
        got = _graph_held(engine, count, lists, solid, what=f"one-sided {n_a}")
        assert got["largest"][0] >= 3
        both = K.components(count, lists, solid, fault="both_lists")
        assert K.differs(got, both) != []                                   # (an edge that one end lists does join)


def test_masks_cut_a_chain(engine):
    n_a = 90
    adjacency = {a: [b for b in (a - 1, a + 1) if 0 <= b < n_a] for a in range(n_a)}
    count, lists = K.graph(n_a, adjacency)
    masks = np.full((1, n_a), 2 ** 64 - 1, np.uint64)
    for a, b in ((29, 30), (59, 60)):                                       # both ends' bits of the two cut bonds
        masks[0, a] &= ~np.uint64(1 << adjacency[a].index(b))
        masks[0, b] &= ~np.uint64(1 << adjacency[b].index(a))
    solid = np.ones((1, n_a), bool)
    cut = _graph_held(engine, count, lists, solid, masks, 1, what="masks, link 1")
    assert cut["n_clusters"][0] == 3 and cut["size_counts"][30] == 3 and sorted(set(cut["labels"][0].tolist())) == [0, 30, 60]
    whole = _graph_held(engine, count, lists, solid, masks, 0, what="masks, link 0")
    assert whole["n_clusters"][0] == 1


@functools.lru_cache(maxsize=None)
def _sized_graph():
    """clusters of 1, 4, 5 and 4097 atoms (chains), one after the other"""
    adjacency, at = {}, 0
    for size in (1, 4, 5, 4097):
        adjacency.update({a: [a + 1] for a in range(at, at + size - 1)})
        at += size
    return K.graph(at, adjacency), at


@pytest.mark.parametrize("n_sizes", [1, 4, 4096])
def test_size_histogram_slots(engine, n_sizes):
    (count, lists), n_a = _sized_graph()
    got = _graph_held(engine, count, lists, np.ones((1, n_a), bool), n_sizes=n_sizes, what=f"n_sizes {n_sizes}")
    want = {1: ([0, 1, 3], 4 + 5 + 4097), 4: ([0, 1, 0, 0, 1, 2], 5 + 4097), 4096: (None, 4097)}[n_sizes]
    assert got["large_atoms"] == want[1] and (want[0] is None or got["size_counts"].tolist() == want[0])
    assert got["size_counts"][n_sizes + 1] == {1: 3, 4: 2, 4096: 1}[n_sizes] and got["largest_label"][0] == 10
    off = K.components(count, lists, np.ones((1, n_a), bool), n_sizes=n_sizes, fault="overflow_off_by_one")
    assert n_sizes == 4096 or K.differs(got, off) != []


def test_three_graphs_in_one_call(engine):
    """an origin's labels never leave its own rows"""
    parts = [K.random_graph(130, seed) for seed in (7, 8, 9)]
    count, lists, solid = (np.concatenate([p[i] for p in parts]) for i in range(3))
    got = _graph_held(engine, count, lists, solid, n_sizes=8, what="three origins")
    for o, p in enumerate(parts):
        alone = engine.debug_cluster_labels(*p, None, 0, 8)
        assert np.array_equal(alone["labels"][0], got["labels"][o]) and alone["largest"][0] == got["largest"][o]
    assert len({tuple(got["labels"][o].tolist()) for o in range(3)}) == 3


def test_graph_refusals(engine):
    from psa_amd import _hip
    count, lists, solid = K.random_graph(65, 4)

    def refused(word, c=count, l=lists, s=solid, **kw):
        with pytest.raises(_hip.PsaHipError, match=word):
            engine.debug_cluster_labels(c, l, s, **kw)
    bad = lists.copy()
    a = int(np.flatnonzero(count[0] > 0)[0])
    bad[0, a, 0] = 65
    refused(r"list\[0\]\[%d\]\[0\] = 65 is outside" % a, l=bad)
    bad[0, a, 0] = -1
    refused("= -1 is outside", l=bad)
    bad[0, a, 0] = a
    refused("self-loop", l=bad)
    for n in (-1, 65):
        wrong = count.copy()
        wrong[0, 3] = n
        refused(r"count\[0\]\[3\] = %d is outside \[0, 64\]" % n, c=wrong)
    refused("link is 0 .* got 2", link=2)
    refused("link is 0 .* got -1", link=-1)
    refused(r"n_sizes is in \[1, 4096\], got 0", n_sizes=0)
    refused(r"n_sizes is in \[1, 4096\], got 4097", n_sizes=4097)
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 65 * 1060 - 1)
    refused(f"need {65 * 1060} bytes")
    reset(engine)
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        refused("sharded context")
    finally:
        engine.comm_destroy()
    assert engine.debug_cluster_labels(count, lists, solid)["n_solid"][0] == solid.sum()


# ---- 2. end to end against the twin -------------------------------------------------------------------------------------------
def _family(name):
    """the first three frames of a family of qlm_cases: three origins"""
    pos, box, r_cut = C.family(name)
    return np.ascontiguousarray(pos[:3]), box, r_cut


@functools.lru_cache(maxsize=None)
def _twin(name, kind, thr, min_connections, link):
    pos, box, r_cut = _family(name)
    groups = [np.arange(pos.shape[1])] if kind == "one" else Q.two_species(pos.shape[1])
    return pos, box, r_cut, groups, K.model(pos, box, groups, r_cut, 1, 6, thr, min_connections, link, 16)


def _solid_call(engine, box, rc, thr, min_connections, link, listing, n_sizes=16, per_atom=True, step=1):
    return engine.solid_clusters(box, rc, 6, thr, min_connections, link, n_sizes, listing, step, per_atom)


def _two_clusters(m):
    return any((np.unique(row[row >= 0], return_counts=True)[1] >= 2).sum() >= 2 for row in m["labels"]) and bool((m["labels"] < 0).any())


# The pairs (0.5, 3) and (0.3, 2) with both links are the cases as set.  On the first three frames the twin gives 1, 9 and 0
# solid atoms of cubic37 for (0.5, 3) and one cluster for (0.3, 2) with link 0 in every family: those cases do not hold two
# clusters of two atoms or more in any origin (they are compared all the same, and asserted to be what this says), and the
# pairs under them, from the same families, take their place for that property: cubic37 (0.6, 1) link 0 and (0.35, 3) link 1,
# triclinic130 and triclinic257 (0.4, 3) link 0.
SINGLE = {("cubic37", 0.5, 3, 0), ("cubic37", 0.5, 3, 1), ("cubic37", 0.3, 2, 0), ("triclinic130", 0.3, 2, 0), ("triclinic257", 0.3, 2, 0)}
CASES = [(name, thr, mc, link) for name in ("cubic37", "triclinic130", "triclinic257") for thr, mc in ((0.5, 3), (0.3, 2)) for link in (0, 1)]
CASES += [("cubic37", 0.6, 1, 0), ("cubic37", 0.35, 3, 1), ("triclinic130", 0.4, 3, 0), ("triclinic257", 0.4, 3, 0)]


@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("name,thr,mc,link", CASES)
def test_against_the_twin(engine, name, thr, mc, link, kind):
    pos, box, r_cut, groups, want = _twin(name, kind, thr, mc, link)
    assert _two_clusters(want) == ((name, thr, mc, link) not in SINGLE) and not (want["connections"] < 0).any()    # before the GPU is touched
    _resident(engine, pos)
    got = _solid_call(engine, box, r_cut, thr, mc, link, _listing(kind, groups))
    assert K.differs(got, want, K.KEYS + ("connections", "n", "bond_masks")) == []
    assert np.array_equal(K.fold_left_out(got["species_rows"]), want["species_rows"]) and K.identities(got)
    assert got["species_rows"].shape == (len(groups), 69) and got["labels"].shape == (3, pos.shape[1])


@pytest.mark.parametrize("name", ["cubic37", "triclinic257"])
def test_default_parameters_give_none_solid(engine, name):
    pos, box, r_cut, groups, want = _twin(name, "one", 0.7, 7, 0)
    assert not want["n_solid"].any()
    _resident(engine, pos)
    got = engine.solid_clusters(box, r_cut, n_sizes=16, per_atom=True)
    assert K.differs(got, want, K.KEYS + ("connections", "n", "bond_masks")) == [] and np.all(got["labels"] == -1) and not got["size_counts"].any()
    assert got["largest_label"].tolist() == [-1] * 3


# ---- 3. agreement with what exists ------------------------------------------------------------------------------------------
def test_agreement_with_local_order_and_the_lists(engine):
    from psa_amd import local_order
    pos, box, r_cut = _family("triclinic130")
    groups = Q.two_species(130)
    listing = _listing("two", groups)
    _resident(engine, pos)
    got = _solid_call(engine, box, r_cut, 0.4, 3, 1, listing)
    hist, _, _, _, xi, n = engine.local_order(box, r_cut, (6,), 10, 10, local_order.w3j_blocks((6,)), listing, 1, 0.2, 6, 0.4, True)
    assert np.array_equal(got["connections"], xi) and np.array_equal(got["n"], n)
    assert np.array_equal(got["species_rows"], hist[:, 30:30 + 69])                                # bit for bit the 69 words
    for o in range(3):
        count, lists = engine.debug_neighbour_lists(box, r_cut, o, listing)
        assert np.array_equal(count, got["n"][o])
        pop = np.array([bin(int(m)).count("1") for m in got["bond_masks"][o]])
        assert np.array_equal(pop, got["connections"][o]) and not np.any(got["bond_masks"][o] >> count.astype(np.uint64))
        again = engine.debug_cluster_labels(count[None], lists[None], (got["connections"][o] >= 3)[None], got["bond_masks"][o][None], 1, 16)
        assert np.array_equal(again["labels"][0], got["labels"][o]) and np.array_equal(again["size_atoms"][0], got["size_atoms"][o])


# ---- 4. known structures --------------------------------------------------------------------------------------------------
def test_fcc_block_is_one_cluster(engine):
    pos = C.fcc_block()
    n_a = pos.shape[1]
    _resident(engine, pos)
    for link in (0, 1):
        got = engine.solid_clusters(Q.CUBIC, 4.6, link=link, n_sizes=n_a, per_atom=True)
        assert np.all(got["connections"] == 12) and np.all(got["labels"] == 0) and np.all(got["size_atoms"] == n_a)
        assert got["largest"].tolist() == [n_a, n_a] and got["largest_label"].tolist() == [0, 0] and got["size_counts"][n_a] == 2
        assert np.all(got["bond_masks"] == 2 ** 12 - 1) and got["species_rows"][0, 12] == 2 * n_a


def _crystallite(offset):
    """32 atoms of fcc, nearest neighbours 3.0 apart: 2 x 2 x 2 cells of four atoms at `offset`, with nothing around them"""
    a = 3.0 * 2.0 ** 0.5
    basis = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    cell = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 1, 3)
    return (cell + basis[None]).reshape(-1, 3) * a + np.asarray(offset, np.float64)


@functools.lru_cache(maxsize=None)
def _structures():
    two = np.concatenate([_crystallite((1.5, 1.5, 1.5)), _crystallite((12.5, 12.0, 11.5))]).astype(np.float32)[None]
    # a slab of three layers of a 8 x 8 lattice in the box's own fractional coordinates, the middle layer on the boundary
    H = np.asarray(Q.TRICLINIC, np.float32).astype(np.float64)
    i, j, k = np.meshgrid(np.arange(8), np.arange(8), np.array([-1, 0, 1]), indexing="ij")
    frac = np.stack([i / 8.0, j / 8.0, (k / 8.0) % 1.0], -1).reshape(-1, 3)
    slab = (frac @ H).astype(np.float32)[None]
    return two, slab


def test_two_crystallites_and_a_slab_through_the_boundary(engine):
    two, slab = _structures()
    groups = [np.arange(two.shape[1])]
    want = K.model(two, Q.CUBIC, groups, 3.5, 1, 6, 0.7, 5, 0, 64)
    assert want["n_clusters"].tolist() == [2] and want["size_counts"].sum() == 2 and (want["labels"] < 0).any()   # the twin: two, not all solid
    _resident(engine, two)
    got = engine.solid_clusters(Q.CUBIC, 3.5, 6, 0.7, 5, 0, 64, per_atom=True)
    assert K.differs(got, want, K.KEYS + ("connections", "n", "bond_masks")) == []
    assert not set(got["labels"][0][:32].tolist()) & set(got["labels"][0][32:].tolist()) - {-1}    # one cluster per copy
    groups = [np.arange(slab.shape[1])]
    want = K.model(slab, Q.TRICLINIC, groups, 3.6, 1, 6, 0.7, 4, 0, 256)
    assert want["n_clusters"].tolist() == [1] and want["largest"].tolist() == [192]                 # the twin: one cluster of all
    reset(engine)
    _resident(engine, slab)
    got = engine.solid_clusters(Q.TRICLINIC, 3.6, 6, 0.7, 4, 0, 256, per_atom=True)
    assert K.differs(got, want, K.KEYS + ("connections", "n", "bond_masks")) == [] and np.all(got["labels"] == 0)


def test_diamond_all_solid_then_none(engine):
    pos = Q.diamond(2)[0]
    _resident(engine, pos)
    four = engine.solid_clusters(Q.CUBIC, 2.8, min_connections=4, n_sizes=512, per_atom=True)
    assert np.all(four["connections"] == 4) and np.all(four["labels"] == 0) and four["largest"].tolist() == [512, 512]
    five = engine.solid_clusters(Q.CUBIC, 2.8, min_connections=5, n_sizes=512, per_atom=True)
    assert np.all(five["labels"] == -1) and not five["n_solid"].any() and np.array_equal(five["species_rows"], four["species_rows"])


# ---- 5. bit for bit -----------------------------------------------------------------------------------------------------------
def _equal(x, y, keys=None):
    return all((x[k] is None and y[k] is None) or np.array_equal(x[k], y[k]) for k in (keys or x))


def test_budgets_blocks_and_repeats(engine):
    from psa_amd import _hip
    pos, box, r_cut = C.family("cubic37")                                  # 40 frames
    n = pos.shape[1]
    groups = Q.two_species(n)
    listing = _listing("two", groups)
    _resident(engine, pos)
    whole = _solid_call(engine, box, r_cut, 0.35, 3, 1, listing)
    assert whole["n_clusters"].max() >= 2 and _equal(whole, _solid_call(engine, box, r_cut, 0.35, 3, 1, listing))
    bare = _solid_call(engine, box, r_cut, 0.35, 3, 1, listing, per_atom=False)
    assert all(bare[k] is None for k in ATOM_KEYS) and _equal(whole, bare, [k for k in whole if k not in ATOM_KEYS])
    for origins in (1, 2, 40):                                             # origins per block: 40, 20 and 1 block
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n * origins + 5)
        assert _equal(whole, _solid_call(engine, box, r_cut, 0.35, 3, 1, listing)), origins
    engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, PER_ORIGIN * n - 1)
    with pytest.raises(_hip.PsaHipError, match=f"need {PER_ORIGIN * n} bytes"):
        _solid_call(engine, box, r_cut, 0.35, 3, 1, listing)
    reset(engine)
    step = _solid_call(engine, box, r_cut, 0.35, 3, 1, listing, step=13)   # origins 0, 13, 26, 39
    assert all(np.array_equal(step[k], whole[k][::13]) for k in ("n_solid", "largest", "largest_label", "labels", "bond_masks"))


def test_permutation_of_the_atoms(engine):
    """xi and the masks are integers of Q, which is the same bits in any order of the atoms: the same partition and sizes, the
    labels mapped through the permutation, exactly"""
    pos, box, r_cut = _family("triclinic130")
    groups = Q.two_species(130)
    listing = _listing("two", groups)
    _resident(engine, pos)
    whole = _solid_call(engine, box, r_cut, 0.4, 3, 0, listing)
    rng = np.random.default_rng(8)
    perms = [rng.permutation(len(g)) for g in listing]
    moved = _solid_call(engine, box, r_cut, 0.4, 3, 0, [g[p] for g, p in zip(listing, perms)])
    at = np.concatenate([np.argsort(p) + s for p, s in zip(perms, (0, len(listing[0])))])   # column of atom i after the shuffle
    assert _equal(whole, moved, ("size_counts", "large_atoms", "n_solid", "n_clusters", "largest", "species_rows"))
    for k in ("size_atoms", "connections", "n"):
        assert np.array_equal(moved[k][:, at], whole[k]), k
    for o in range(3):
        a, b = whole["labels"][o], moved["labels"][o][at]
        assert K.same_partition(a, b)
        for label in np.unique(a[a >= 0]):
            assert np.all(b[a == label] == at[a == label].min())            # the smallest column of the members, after the shuffle


# ---- 6. no trace ----------------------------------------------------------------------------------------------------------------
def test_no_trace(engine):
    from psa_amd import local_order
    pos, box, r_cut = C.family("cubic37")
    _resident(engine, pos)
    table = local_order.w3j_blocks((4, 6))

    def others():
        return (*engine.angle_histogram(box, r_cut, 45), *engine.bond_order(box, r_cut, (4, 6), 50, per_atom=True),
                *engine.local_order(box, r_cut, (4, 6), 50, 50, table, None, 3, 0.2, 6, 0.35, True), engine.pair_histogram(box, [0, 3], 0.25, 40))

    def call(eng, loud=False):
        got = eng.solid_clusters(box, r_cut, 6, 0.35, 3, 1, 16, None, 3, True)
        return [np.asarray(v).copy() for v in got.values()]
    before = others()
    engine.timings()                                                       # (reset)
    r0 = call(engine)
    t = engine.timings()
    assert all(t[k] > 0 for k in ("gather", "transpose", "phase", "project", "fft", "epilogue", "d2h"))
    graph = K.random_graph(257, 12)
    g0 = engine.debug_cluster_labels(*graph)
    try:
        S.check_poisoned(engine, "solid_clusters per atom", call, r0)
        S.check_poisoned(engine, "debug_cluster_labels", lambda eng: [np.asarray(v).copy() for v in eng.debug_cluster_labels(*graph).values()],
                         [np.asarray(v).copy() for v in g0.values()])
    finally:
        engine.scratch_fill(-1)
    for a, b in zip(before, others()):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- 7. the calculator ----------------------------------------------------------------------------------------------------------
def _calculator(engine, pos, box, types=None, dt=0.002):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), dt)
    return SEDCalculator(tr, 1, 1, 1).attach(engine=engine)


def test_calculator(engine):
    from psa_amd import SolidClusters
    pos, box, r_cut = _family("triclinic130")
    groups = Q.two_species(130)
    types = np.ones(130, np.int32)
    types[groups[1]] = 2
    calc = _calculator(engine, pos, box, types)
    res = calc.calculate_solid_clusters(r_cut, 6, 0.4, 3, "solid_bonds", 16, basis_atom_types=[1, 2], per_atom=True)
    raw = _solid_call(engine, box, r_cut, 0.4, 3, 1, _listing("two", groups))
    assert isinstance(res, SolidClusters) and res.origins == 3 and res.link == "solid_bonds" and res.min_connections == 3
    assert all(np.array_equal(getattr(res, k), raw[k]) for k in ("size_counts", "n_solid", "n_clusters", "largest", "largest_label", "labels",
                                                               "size_atoms", "bond_masks"))
    assert np.array_equal(res.connections_atoms, raw["connections"]) and np.array_equal(res.neighbours, raw["n"])
    assert np.array_equal(res.connections, raw["species_rows"][:, :65]) and np.array_equal(res.incomplete, raw["species_rows"][:, 68])
    assert res.sizes.shape == (18,) and np.array_equal(res.samples, [3 * 90, 3 * 40]) and res.atoms.shape == (130,)
    assert np.array_equal(res.mean_size_counts, raw["size_counts"] / 3.0)
    xi = raw["connections"][:, :90]
    assert res.solid_fraction[0] == pytest.approx((xi[xi >= 0] >= 3).mean())
    for o in range(3):
        members = res.largest_atoms(o)
        assert members.size == res.largest[o] and np.array_equal(members, res.atoms[raw["labels"][o] == raw["largest_label"][o]])
    plain = calc.calculate_solid_clusters(r_cut)
    assert plain.labels is None and plain.size_counts.shape == (258,) and plain.link == "neighbours" and not plain.n_solid.any()
    with pytest.raises(ValueError, match="per_atom"):
        plain.largest_atoms(0)
    for bad in (dict(solid_l=5), dict(solid_l=14), dict(solid_threshold=0.0), dict(min_connections=65), dict(link="bonds"), dict(n_sizes=0),
                dict(n_sizes=4097)):
        with pytest.raises(ValueError):
            calc.calculate_solid_clusters(r_cut, **bad)
    ball = Q.ball(70, 2, 6.0)
    with pytest.raises(ValueError, match="more than 64 neighbours"):
        _calculator(engine, ball, Q.CUBIC).calculate_solid_clusters(6.0)


def test_sharded_calculator_refuses(engine):
    pos, box, r_cut = _family("cubic37")
    calc = _calculator(engine, pos, box)

    class Sharded:
        nranks = 2
    calc._shard = Sharded()
    with pytest.raises(NotImplementedError, match="sharded calculator"):
        calc.calculate_solid_clusters(r_cut)


def test_refusals(engine):
    from psa_amd import _hip
    pos, box, r_cut = _family("cubic37")
    _resident(engine, pos)

    def refused(word, **kw):
        with pytest.raises(_hip.PsaHipError, match=word):
            engine.solid_clusters(box, r_cut, **kw)
    for bad in (5, 0, 14, -2):
        refused(f"solid_l = {bad} is not an even order", solid_l=bad)
    for bad in (0.0, 1.5, -0.5, float("nan")):
        refused("threshold is in .* got", solid_threshold=bad)
    refused(r"min_connections is in \[0, 64\], got 65", min_connections=65)
    refused(r"min_connections is in \[0, 64\], got -1", min_connections=-1)
    refused("link is 0 .* got 2", link=2)
    refused(r"n_sizes is in \[1, 4096\], got 0", n_sizes=0)
    refused(r"n_sizes is in \[1, 4096\], got 4097", n_sizes=4097)
    refused("origin_step must be at least 1, got 0", origin_step=0)
    engine.comm_init(engine.new_unique_id(), 0, 1)
    try:
        refused("sharded context.*psa_solid_clusters|psa_solid_clusters.*sharded context")
    finally:
        engine.comm_destroy()
    empty = engine.solid_clusters(box, r_cut, groups=[np.zeros(0, np.int32)], n_sizes=4, per_atom=True)
    assert not empty["species_rows"].any() and not empty["size_counts"].any() and empty["largest_label"].tolist() == [-1] * 3
    assert empty["labels"].shape == (3, 0) and empty["n_solid"].tolist() == [0] * 3
    assert engine.solid_clusters(box, r_cut, 6, 0.3, 2)["n_solid"].any()
