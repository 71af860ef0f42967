"""The 48-node folded low-rank route on the GPU (psa_set_k1_lowrank_nodes, the default of a new context: the 48-node table
and the image D' = P_ref w - phi L W_hi, node_table_n48_kernel and diff_n48_table_kernel; k1_lowrank_n48.hip, or the
two-product node pass of k1_planes_lw.hip on the 48-node table and the D pass on the image; lowrank_combine_r_kernel<48>).

The view is Engine.debug_project_only(..., route=True) with the route forced on as in tests/test_gpu_lowrank_fold.py.
  (a) the 48-node pair launch against the 48-node two passes, bit for bit, the counters asserted.  One axis at a time
      around K = 40, n_g = 257, T = 96: K 2, 3, 79, 80, 81 (the cut between the roles is at D' row 160 = k-vector 80), 255,
      256; 257 and 513 run the two passes; 2, 4, 6, 8, 10, 16, 18 stages run (the ring of four, the fold of eight, the
      three-stage prefetch at the end), each with a full, a ragged and an all-padding last stage; T 1, 15, 16, 17, 63, 64,
      65, 130; an index list with duplicates, a weighted group, displacement mode, interval -1 and interval 1; the input
      families of tests/lowrank_env_cases.py;
  (b) every one of those results against float64 element by element, real and imaginary parts on their own, under the bound
      of tests/lowrank_n48_cases.py;
  (c) row determinism: K = 256 whole, as halves in either order and as 96 + 160 give bit-identical rows;
  (d) with the switch at 64 the route is the 64-node folded route, bit for bit: against a context that never left 64, and
      against tests/golden/lowrank_fold64_q.npy, q of the base case from the build before the switch existed.
No bound here is computed from device output."""
import os

import numpy as np
import pytest

import lowrank_env_cases as E
import lowrank_n48_cases as N
from engine_state import reset
from ref64 import gamma
from test_gpu_lowrank_envelope import _force

pytestmark = pytest.mark.gpu

U = E.U
TAILS = {"full": 0, "ragged": 5, "padded": 37}                # atoms short of 32 x stages
PAIR_ROWS = [2, 3, 79, 80, 81, 255, 256]
TWO_PASS_ROWS = [257, 513]
DEVICE_STAGES = [2, 4, 6, 8, 10, 16, 18]
FRAMES = [1, 15, 16, 17, 63, 64, 65, 130]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "lowrank_fold64_q.npy")


@pytest.fixture
def forced(engine):
    _force(engine)
    try:
        yield engine
    finally:
        engine.set_k1_lowrank_nodes(48)
        engine.set_lowrank_fold(True)
        reset(engine)
        for slot in (0, 1):
            engine.release(slot)
        engine.invalidate()


_CASES = {}                                 # the inputs, their float64 references and bounds, per shape


def _case(family="quiet_frames", K=None, n=None, T=None, geom="plain_100", idx=None):
    key = (family, K, n, T, geom, None if idx is None else tuple(idx))
    if key not in _CASES:
        c = N.case(family, K=K, n=n, T=T, geom=geom, idx=idx)
        c["R"] = E.reference(c)
        c["babs_n48"] = N.bound_abs_n48(c, c["R"])
        _CASES[key] = c
    return _CASES[key]


def _routed(engine, c, pair=True, nodes=48, k=None):
    """(q before the FFT (K, 3, T), launches on the route, launches the pair served), the fold on"""
    from psa_amd import _hip
    engine.set_option(_hip.OPT_K1_LOWRANK_PAIR, int(pair))
    engine.set_lowrank_fold(True)
    engine.set_k1_lowrank_nodes(nodes)
    engine.set_atom_weights(c["weights"])
    slot = 1 if c["disp"] else 0
    engine.ensure_resident(slot, c["data"])
    n0, p0 = engine.lowrank_launches(), engine.lowrank_pair_launches()
    got = engine.debug_project_only(slot, c["r"], c["k"] if k is None else k, c["idx"], _hip.F_DISPLACEMENTS if c["disp"] else 0,
                                    route=True)
    return got, engine.lowrank_launches() - n0, engine.lowrank_pair_launches() - p0


def _what(c, got):
    return f"{c['name']} K={got.shape[0]} n_g={c['n_g']} ({E.device_stages(c['n_g'])} stages run) T={got.shape[2]}"


def _bitwise(a, b, what):
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} words differ, first at (j, c, t, re/im) = {tuple(np.argwhere(diff)[0])}"


def _under_bound(c, got):
    R = c["R"]
    assert np.all(np.isfinite(got)), _what(c, got)
    e, at = E.excess(got, R["ref"], c["babs_n48"])
    msg = f"{_what(c, got)}: worst element {at} at {e:.3f} x the 48-node bound, gamma {gamma(got, R['ref'], R['B']) / U:.2f} u"
    print(msg)
    assert e <= 1, msg


def _both(engine, c, served=True):
    """(a) and (b) of one case: 48-node pair launch against 48-node two passes, bitwise; the result against float64"""
    on, n_on, p_on = _routed(engine, c, pair=True)
    off, n_off, p_off = _routed(engine, c, pair=False)
    what = _what(c, on)
    assert (n_on, p_on) == (1, 1 if served else 0), f"{what}, pair on: {n_on} launches on the route, {p_on} by the pair"
    assert (n_off, p_off) == (1, 0), f"{what}, pair off: {n_off} launches on the route, {p_off} by the pair"
    _bitwise(on, off, what)
    _under_bound(c, on)
    return on


@pytest.mark.parametrize("K", PAIR_ROWS)
def test_rows(forced, K):
    _both(forced, _case(K=K))


@pytest.mark.parametrize("K", TWO_PASS_ROWS)
def test_rows_past_one_block_run_the_two_passes(forced, K):
    _both(forced, _case(K=K), served=False)


@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("stages", DEVICE_STAGES)
def test_device_stages(forced, stages, tail):
    c = _case(n=32 * stages - TAILS[tail])
    assert E.device_stages(c["n_g"]) == stages
    _both(forced, c)


@pytest.mark.parametrize("T", FRAMES)
def test_frames(forced, T):
    _both(forced, _case(T=T))


def test_index_list_with_duplicates(forced):
    n_g = 32 * 5 - 5
    idx = np.random.default_rng(31).integers(0, n_g + 40, n_g)
    idx[5] = idx[6] = idx[n_g - 1]
    c = _case(n=n_g + 40, idx=idx.tolist())
    assert len(set(c["idx"].tolist())) < n_g
    _both(forced, c)


@pytest.mark.parametrize("family", E.FAMILIES)
def test_families(forced, family):
    """every input family (the quiet-frames families, the weighted group and displacement mode among them)"""
    got = _both(forced, _case(family))
    if family == "zeros":
        assert not got.any(), "an all-zero array must give exactly zero"


@pytest.mark.parametrize("geom", ["neg_-1-10", "seg_1"])
def test_other_side_and_other_interval(forced, geom):
    c = _case(geom=geom)
    assert c["plan"]["interval"] == (-1 if geom.startswith("neg") else 1)
    _both(forced, c)


# ---- (c) row determinism ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [True, False], ids=["pair", "two_passes"])
def test_rows_do_not_depend_on_the_split(forced, pair):
    c = _case(K=256)
    whole, n, p = _routed(forced, c, pair=pair)
    assert (n, p) == (1, int(pair))
    for parts in ([(0, 128), (128, 256)], [(128, 256), (0, 128)], [(0, 96), (96, 256)]):
        for lo, hi in parts:
            part, n, p = _routed(forced, c, pair=pair, k=c["k"][lo:hi])
            assert (n, p) == (1, int(pair))
            _bitwise(part, whole[lo:hi], f"rows [{lo}, {hi}) of {parts}, {'pair launch' if pair else 'two passes'}")


# ---- (d) the switch at 64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [40, 257])
def test_64_nodes_is_the_folded_route_as_it_was(forced, K):
    """the shared context, after 48-node launches, with the switch at 64, against a second context in which it was at 64
    before its first launch; the base case also against q recorded from the build before the switch existed"""
    from psa_amd import _hip
    c = _case(K=K)
    new, _, _ = _routed(forced, c, nodes=48)
    got, n, p = _routed(forced, c, nodes=64)
    other = _hip.Engine(0)
    try:
        _force(other)
        want, n2, p2 = _routed(other, c, nodes=64)
    finally:
        other.close()
    assert (n, p) == (n2, p2) == (1, int(K <= 256))
    _bitwise(got, want, f"64 nodes, K={K}")
    assert np.any(new.view(np.uint32) != got.view(np.uint32)), "the node count changes nothing"
    if K == 40:
        _bitwise(got, np.load(GOLDEN), "64 nodes against the recorded folded route")


def test_48_nodes_need_the_fold(forced):
    """with the fold off the switch is without effect: the unfolded 64-node route, whatever the node count says"""
    from psa_amd import _hip
    c = _case()
    forced.set_option(_hip.OPT_K1_LOWRANK_PAIR, 1)
    forced.set_atom_weights(c["weights"])
    forced.ensure_resident(0, c["data"])
    forced.set_lowrank_fold(False)
    out = {}
    for nodes in (48, 64):
        forced.set_k1_lowrank_nodes(nodes)
        n0 = forced.lowrank_launches()
        out[nodes] = forced.debug_project_only(0, c["r"], c["k"], c["idx"], 0, route=True)
        assert forced.lowrank_launches() - n0 == 1
    _bitwise(out[48], out[64], "fold off")
