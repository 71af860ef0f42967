"""The folded low-rank route on the GPU (psa_set_k1_lowrank_fold: the node table's lo piece folded into the D image,
diff_fold_table_kernel; two products per node row in k1_lowrank_fold.hip or in the two-product node pass of k1_planes_lw.hip
with the D pass on the folded image).

The view is Engine.debug_project_only(..., route=True) with the route forced on as in tests/test_gpu_lowrank_envelope.py.
  (a) the folded pair launch against the folded two passes, bit for bit, the counters asserted: node rows and D' rows keep
      their chain order, so q before the combine must not differ in a single bit.  One axis at a time around K = 40,
      n_g = 257, T = 96: K 2, 63, 64, 65 (the cut between the roles is at D' row 128 = k-vector 64), 128, 255, 256; 257
      and 513 decline the pair; 2, 4, 6, 8, 10, 38, 40, 42 stages run, each with a full, a ragged and an all-padding last
      stage; T 1, 16, 17, 63, 64, 65, 130, 513; an index list with duplicates, a weighted group, displacement mode, the
      negative side of Gamma;
  (b) every one of those results, and every input family, against float64 element by element under the folded bound of
      tests/lowrank_fold_cases.py and under the route's existing bound (lowrank_env_cases.bound_abs); the D pass by
      difference at 27, 91 and 1211 atoms under the existing bound_diff_abs;
  (c) row determinism: K = 256 whole, as halves in either order and as 96 + 160 give bit-identical rows;
  (d) with the fold off the route is what it is in a context that never had it on, bit for bit;
  (e) one full project + finalize with the fold on against the dense kernels after the FFT, to the tolerances of
      tests/test_gpu_lowrank_envelope.py.
No bound here is computed from device output."""
import numpy as np
import pytest

import lowrank_env_cases as E
import lowrank_fold_cases as F
from conftest import rel_max
from engine_state import reset
from ref64 import gamma, project64, row_rel, scale_B
from test_gpu_lowrank_envelope import TOL, TOL_ROW, _force

pytestmark = pytest.mark.gpu

U = E.U
TAILS = {"full": 0, "ragged": 5, "padded": 37}                # atoms short of 32 x stages
PAIR_ROWS = [2, 63, 64, 65, 128, 255, 256]
DECLINED_ROWS = [257, 513]
DEVICE_STAGES = [2, 4, 6, 8, 10, 38, 40, 42]
FRAMES = [1, 16, 17, 63, 64, 65, 130, 8 * 64 + 1]


def _release(engine):
    reset(engine)
    for slot in (0, 1):
        engine.release(slot)
    engine.invalidate()


@pytest.fixture
def forced(engine):
    _force(engine)
    try:
        yield engine
    finally:
        _release(engine)


_CASES = {}                                 # the inputs, their float64 references and bounds, per shape


def _case(family="quiet_frames", K=None, n=None, T=None, geom="plain_100", idx=None):
    key = (family, K, n, T, geom, None if idx is None else tuple(idx))
    if key not in _CASES:
        c = E.case(family, K=K, n=n, T=T, geom=geom, idx=idx)
        c["R"] = E.reference(c)
        c["babs"] = E.bound_abs(c, c["R"])
        c["babs_fold"] = F.bound_abs_fold(c, c["R"])
        _CASES[key] = c
    return _CASES[key]


def _routed(engine, c, pair=True, fold=True, k=None):
    """(q before the FFT (K, 3, T), launches on the route, launches the pair served) with the pair option and the fold switch as given"""
    from psa_amd import _hip
    engine.set_option(_hip.OPT_K1_LOWRANK_PAIR, int(pair))
    engine.set_lowrank_fold(bool(fold))
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


def _under_bounds(c, got, tag=""):
    """(b): the folded result under the folded bound and under the route's existing bound, element by element"""
    R = c["R"]
    assert np.all(np.isfinite(got)), _what(c, got)
    e_new, at = E.excess(got, R["ref"], c["babs_fold"])
    e_old, _ = E.excess(got, R["ref"], c["babs"])
    msg = (f"{tag}{_what(c, got)}: worst element {at} at {e_new:.3f} x the folded bound, {e_old:.3f} x the existing bound, gamma "
           f"{gamma(got, R['ref'], R['B']) / U:.2f} u")
    print(msg)
    assert e_new <= 1 and e_old <= 1, msg


def _both(engine, c, served=True):
    """(a) and (b) of one case: folded pair launch against folded two passes, bitwise; the result against float64"""
    on, n_on, p_on = _routed(engine, c, pair=True)
    off, n_off, p_off = _routed(engine, c, pair=False)
    what = _what(c, on)
    assert (n_on, p_on) == (1, 1 if served else 0), f"{what}, pair on: {n_on} launches on the route, {p_on} by the pair"
    assert (n_off, p_off) == (1, 0), f"{what}, pair off: {n_off} launches on the route, {p_off} by the pair"
    _bitwise(on, off, what)
    _under_bounds(c, on)
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


@pytest.mark.parametrize("family", E.FAMILIES)
def test_families(forced, family):
    """every input family (the weighted groups and displacement mode among them), pair launch and two passes"""
    got = _both(forced, _case(family))
    if family == "zeros":
        assert not got.any(), "an all-zero array must give exactly zero"


@pytest.mark.parametrize("geom", ["neg_-1-10", "seg_1"])
def test_other_side_and_other_interval(forced, geom):
    c = _case(geom=geom)
    assert c["plan"]["interval"] == (-1 if geom.startswith("neg") else 1)
    _both(forced, c)


# ---- (b) the D pass on its own, by difference -------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [True, False], ids=["pair", "two_passes"])
@pytest.mark.parametrize("n", [27, 91, 1211])
def test_d_pass_by_difference(forced, n, pair):
    """got(scattered) - got(on the line): the plan tables are bit-equal, so node rows, combine and E are the same in both
    runs; what is left is the two roundings of D + E, the D terms and one float32 rounding of each final sum"""
    line, off = E.line_and_scattered(n=n)
    for name in ("L", "phi", "kappa"):
        assert np.array_equal(line["plan"][name].view(np.uint8), off["plan"][name].view(np.uint8)), name
    B = scale_B(line["data"], line["r"])
    ref = project64(off["data"], off["r"], off["k"]) - project64(line["data"], line["r"], line["k"])
    babs = E.bound_diff_abs(line, off, B)
    runs = [_routed(forced, c, pair=pair) for c in (off, line)]
    assert all((n_lr, n_pair) == (1, int(pair)) for _, n_lr, n_pair in runs), [r[1:] for r in runs]
    got = runs[0][0].astype(np.complex128) - runs[1][0].astype(np.complex128)
    e, at = E.excess(got, ref, babs)
    msg = (f"D by difference n_g={n} ({E.device_stages(n)} stages run), {'pair launch' if pair else 'two passes'}: worst element {at} "
           f"at {e:.3f} x its bound, gamma {gamma(got, ref, B) / U:.2f} u of a bound of {float(babs.max() / B.max()) / U:.2f} u")
    print(msg)
    assert e <= 1, msg


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


# ---- (d) fold off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [40, 257])
def test_fold_off_is_the_route_as_it_was(forced, K):
    """the shared context, after folded launches, with the fold off, against a second context in which it was
    off before its first launch: pair launch (K = 40) and two passes (K = 257), bit for bit"""
    from psa_amd import _hip
    c = _case(K=K)
    _routed(forced, c, fold=True)
    got, n, p = _routed(forced, c, fold=False)
    other = _hip.Engine(0)
    try:
        _force(other)
        want, n2, p2 = _routed(other, c, fold=False)
    finally:
        other.close()
    assert (n, p) == (n2, p2) == (1, int(K <= 256))
    _bitwise(got, want, f"fold off, K={K}")
    E_old, _ = E.excess(got, c["R"]["ref"], c["babs"])
    assert E_old <= 1
    folded, _, _ = _routed(forced, c, fold=True)
    assert np.any(folded.view(np.uint32) != got.view(np.uint32)), "the fold changes nothing"


# ---- (e) the whole calculation against the dense kernels ---------------------------------------------------------------
def test_project_and_finalize_against_the_dense_route(forced):
    from psa_amd import _hip
    c = _case(K=256, T=256)
    T, K = c["data"].shape[0], len(c["k"])
    out = {}
    for lowrank in (1, 0):
        forced.set_option(_hip.OPT_K1_LOWRANK, lowrank)
        forced.set_lowrank_fold(True)
        forced.ensure_resident(0, c["data"])
        n0, p0 = forced.lowrank_launches(), forced.lowrank_pair_launches()
        forced.project(0, c["r"], c["k"], None, 0, K_total=K, k_offset=0)
        out[lowrank] = forced.finalize(T, K, False)
        assert (forced.lowrank_launches() - n0, forced.lowrank_pair_launches() - p0) == (lowrank, lowrank)
    err, rows = rel_max(out[1], out[0]), row_rel(out[1], out[0])
    msg = f"folded route against the dense kernels after the FFT: rel_max {err:.2e}, worst row {rows.max():.2e} (k {int(np.argmax(rows))})"
    print(msg)
    assert np.all(np.isfinite(out[1])) and err <= TOL and rows.max() <= TOL_ROW, msg
