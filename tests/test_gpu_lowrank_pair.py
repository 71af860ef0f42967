"""The low-rank route's pair launch (k1_lowrank_pair.hip: node rows and D rows of a list with one 512-row D block in ONE
kernel launch of two balanced workgroups per frame tile) against the two-pass route (k1_planes_lw.hip on the node table,
then k1_planes_diff.hip), bit for bit.

Node rows and D rows keep their chain order in the pair launch, so q before the combine -- and with it everything after
-- must not differ in a single bit.  The view is Engine.debug_project_only(..., route=True) with the route forced on as in
tests/test_gpu_lowrank_envelope.py, once with PSA_OPT_K1_LOWRANK_PAIR on and once with it off.  Every case asserts
through the two counters that the pair launch served the first run (or, above 256 k-vectors, declined it) and that the
second took the two passes.

One axis at a time around K = 40, n_g = 257, T = 96 on the [100] path through Gamma:
  K       2, 31, 32, 33 (the cut between the roles is at D row 64 = k-vector 32), 128, 255, 256; 257 and 513 need more
          than one D block: the pair declines and both runs take the two passes;
  stages  the count the kernels run (the planes pad the atom axis to 64): 2, 4, 6 (the prefetch meets the end), 8, 10
          (role B's four-stage ring wraps), 38, 40, 42 (role A's 40-stage period), each with a full last stage, a ragged
          one and one that is all padding (group sizes as in tests/lowrank_env_cases.py);
  T       1, 16, 17, 63, 64, 65, 130 and 8 x 64 + 1: a ninth frame tile, so the blocks past the last tile return;
  groups  an index list with duplicates, a weighted group, displacement mode, the negative side of Gamma.
One case runs the full project + finalize (complex result and intensity) both ways."""
import numpy as np
import pytest

import lowrank_env_cases as E
from engine_state import reset
from test_gpu_lowrank_envelope import _force

pytestmark = pytest.mark.gpu

TAILS = {"full": 0, "ragged": 5, "padded": 37}                # atoms short of 32 x stages (tests/test_gpu_lowrank_perelement.py)
PAIR_ROWS = [2, 31, 32, 33, 128, 255, 256]
DECLINED_ROWS = [257, 513]
DEVICE_STAGES = [2, 4, 6, 8, 10, 38, 40, 42]
FRAMES = [1, 16, 17, 63, 64, 65, 130, 8 * 64 + 1]


@pytest.fixture
def forced(engine):
    from psa_amd import _hip
    _force(engine)
    try:
        yield engine
    finally:
        engine.set_option(_hip.OPT_K1_LOWRANK_PAIR, 1)
        reset(engine)
        for slot in (0, 1):
            engine.release(slot)
        engine.invalidate()


_CASES = {}


def _case(family="quiet_frames", K=None, n=None, T=None, geom="plain_100", idx=None):
    key = (family, K, n, T, geom, None if idx is None else tuple(idx))
    if key not in _CASES:
        _CASES[key] = E.case(family, K=K, n=n, T=T, geom=geom, idx=idx)
    return _CASES[key]


def _routed(engine, c, pair):
    """(q before the FFT (K, 3, T), launches on the route, launches the pair served) with the option set to `pair`"""
    from psa_amd import _hip
    engine.set_option(_hip.OPT_K1_LOWRANK_PAIR, int(pair))
    engine.set_atom_weights(c["weights"])
    slot = 1 if c["disp"] else 0
    engine.ensure_resident(slot, c["data"])
    n0, p0 = engine.lowrank_launches(), engine.lowrank_pair_launches()
    got = engine.debug_project_only(slot, c["r"], c["k"], c["idx"], _hip.F_DISPLACEMENTS if c["disp"] else 0, route=True)
    return got, engine.lowrank_launches() - n0, engine.lowrank_pair_launches() - p0


def _both(engine, c, served=True):
    on, n_on, p_on = _routed(engine, c, True)
    off, n_off, p_off = _routed(engine, c, False)
    what = f"{c['name']} K={len(c['k'])} n_g={c['n_g']} ({E.device_stages(c['n_g'])} stages run) T={on.shape[2]}"
    assert (n_on, p_on) == (1, 1 if served else 0), f"{what}, option on: {n_on} launches on the route, {p_on} by the pair"
    assert (n_off, p_off) == (1, 0), f"{what}, option off: {n_off} launches on the route, {p_off} by the pair"
    assert np.all(np.isfinite(on)), what
    diff = on.view(np.uint32) != off.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} words differ, first at (j, c, t, re/im) = {tuple(np.argwhere(diff)[0])}"
    return on


@pytest.mark.parametrize("K", PAIR_ROWS)
def test_rows(forced, K):
    _both(forced, _case(K=K))


@pytest.mark.parametrize("K", DECLINED_ROWS)
def test_rows_past_one_block_decline(forced, K):
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


@pytest.mark.parametrize("family", ["weighted_mass", "displacements"])
def test_weighted_and_displacement(forced, family):
    _both(forced, _case(family))


def test_negative_side(forced):
    c = _case(geom="neg_-1-10")
    assert c["plan"]["interval"] == -1
    _both(forced, c)


def test_project_and_finalize(forced):
    """the whole calculation of the base case: complex result and intensity, pair launch against the two passes"""
    from psa_amd import _hip
    c = _case()
    T, K = c["data"].shape[0], len(c["k"])
    out = {}
    for pair in (1, 0):
        forced.set_option(_hip.OPT_K1_LOWRANK_PAIR, pair)
        forced.ensure_resident(0, c["data"])
        n0, p0 = forced.lowrank_launches(), forced.lowrank_pair_launches()
        forced.project(0, c["r"], c["k"], None, 0, K_total=K, k_offset=0)
        out[pair] = forced.finalize(T, K, False, with_intensity=True)
        assert (forced.lowrank_launches() - n0, forced.lowrank_pair_launches() - p0) == (1, pair)
    for got, want in zip(out[1], out[0]):
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
