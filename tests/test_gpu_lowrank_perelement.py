"""The low-rank k-path route (node rows through k1_planes_lw, the D pass k1_planes_diff.hip, lowrank_combine_r_kernel) against
a float64 reference, element by element, before the FFT.

The view is Engine.debug_project_only(..., route=True) (psa_debug_project_route): the launch is routed as psa_sed_project
routes a list, with the route forced on as in tests/test_gpu_lowrank_envelope.py, and every case asserts through
lowrank_launches that the route ran.  The metric is the largest |q - q64| of any output element, real and imaginary parts
on their own, over that element's own bound (tests/lowrank_env_cases.py: derived from the route's arithmetic in units of
B[c, t] = sum_a |w_a d[t, a, c]| and of the float64 node rows, never measured).  tests/test_lowrank_envelope_host.py shows
on the CPU, from a NumPy model, that a route which loses the second float16 piece of d on the quiet frames exceeds the
bound 20 - 27 x while it passes the post-FFT bars of the older low-rank tests, and that D-pass faults exceed the differential
bound 12 - 81 x at 27 to 257 atoms.

One axis at a time around K = 40, n_g = 257, T = 96 on the quiet-frames input -- rows (the D pass's 512-row blocks, the
combine's 64-row stages and groups of four), atom stages (the D pass's LDS-DMA runs two and three stages ahead, its ring
repeats every 40 stages; the planes pad the atom axis to 64, so the kernels run an even number of stages, 2 ceil(n_g / 64):
the axis is walked by that device count -- 2, 4, 6, 36, 38, 40, 42, 76, 78, 80, 82 -- and every case asserts it from the
size of the group's plane set), frames (16-frame groups, 64-frame D tiles, the combine's 256-frame blocks) --, every input family,
the other side of Gamma and a node interval away from it, and the D pass on its own by difference (the same path on the line
and scattered off it: equal plan tables, so equal node rows and combine).  Each case prints its shape, the worst element and
its error over its bound, gamma in u and the largest bound in u.  No bound or gamma here is computed from device output
other than the result under test."""
import time

import numpy as np
import pytest

import lowrank_env_cases as E
from lowrank_cases import D_LIMIT
from ref64 import gamma, project64, scale_B
from engine_state import reset
from test_gpu_lowrank_envelope import _force

pytestmark = pytest.mark.gpu

ROWS = [2, 3, 63, 64, 65, 255, 256, 257, 513]
STAGES = [1, 2, 3, 4, 5, 39, 40, 41, 79, 80, 81]              # ceil(n_g / 32): run as 2, 2, 4, 4, 6, 40, 40, 42, 80, 80, 82
DEVICE_STAGES = [2, 4, 6, 36, 38, 40, 42, 76, 78, 80, 82]      # what the kernels run: the prefetch depth at the end; 36 and
#                                                                38, 76 and 78: the last stages' prefetch wraps the 40-stage ring
TAILS = {"full": 0, "ragged": 5, "padded": 37}                # atoms short of 32 x stages; padded: the last stage is all padding
PL_STAGE_BYTES = 6144                                          # k1_f16.h: one 32-atom stage of one 16-frame group in the planes
FRAMES = [1, 15, 16, 17, 63, 64, 65, 130, 255, 256, 257]
U = E.U


@pytest.fixture
def forced(engine):
    _force(engine)
    try:
        yield engine
    finally:
        reset(engine)
        for slot in (0, 1):
            engine.release(slot)
        engine.invalidate()


_CASES = {}                                 # the inputs and their float64 references, per shape


def _case(family="quiet_frames", K=None, n=None, T=None, geom="plain_100", idx=None):
    key = (family, K, n, T, geom, None if idx is None else tuple(idx))
    if key not in _CASES:
        c = E.case(family, K=K, n=n, T=T, geom=geom, idx=idx)
        c["R"] = E.reference(c)
        c["babs"] = E.bound_abs(c, c["R"])
        _CASES[key] = c
    return _CASES[key]


def _run(engine, c):
    """the case's projection (K, 3, T) through the routed pre-FFT view; the route must have served it"""
    from psa_amd import _hip
    engine.set_atom_weights(c["weights"])
    slot = 1 if c["disp"] else 0
    engine.ensure_resident(slot, c["data"])
    n0 = engine.lowrank_launches()
    got = engine.debug_project_only(slot, c["r"], c["k"], c["idx"], _hip.F_DISPLACEMENTS if c["disp"] else 0, route=True)
    taken = engine.lowrank_launches() - n0
    assert taken == 1, f"{c['name']} K={len(c['k'])} n_g={c['n_g']}: {taken} launches on the low-rank route, not 1"
    # the stages the kernels ran, from the group's plane set: (frame groups x stages + 4 of padding) x 6 KiB (plane_bytes)
    n_sets, nbytes = engine.plane_cache()
    n_fg = -(-c["data"].shape[0] // 16)
    assert n_sets == 1 and nbytes == (n_fg * E.device_stages(c["n_g"]) + 4) * PL_STAGE_BYTES, (n_sets, nbytes, c["n_g"])
    return got


def _shape(c, got):
    return (f"{c['name']} K={got.shape[0]} n_g={c['n_g']}{'' if c['idx'] is None else ' (index list)'} S={E.stages(c['n_g'])} "
            f"({E.device_stages(c['n_g'])} stages run) T={got.shape[2]}")


def _check(c, got, t0=None, tag=""):
    R, babs = c["R"], c["babs"]
    assert np.all(np.isfinite(got)), _shape(c, got)
    e, at = E.excess(got, R["ref"], babs)
    g = gamma(got, R["ref"], R["B"])
    live = R["B"] > 0
    top = float(np.max((babs / np.where(live, R["B"], 1.0)[None])[:, live])) if live.any() else 0.0
    msg = (f"{tag}{_shape(c, got)}: worst element (j, c, t) = {at} at {e:.3f} x its bound, gamma {g / U:.2f} u, largest bound "
           f"{top / U:.1f} u" + (f", {time.perf_counter() - t0:.2f} s" if t0 else ""))
    print(msg)
    assert e <= 1, msg


def _dup_list(n_tot, n_g, seed):
    idx = np.random.default_rng(seed).integers(0, n_tot, n_g)
    idx[5] = idx[6] = idx[n_g - 1]
    return idx.tolist()


# ---- the plain view is what it was: with the same options and planes it stays on the dense kernels ---------------------
def test_plain_view_never_takes_the_route(forced):
    import dense_cases as D
    c = _case()
    forced.ensure_resident(0, c["data"])
    n0 = forced.lowrank_launches()
    plain = forced.debug_project_only(0, c["r"], c["k"])
    forced.debug_project_only(0, c["r"], c["k"], frames=(16, 48))
    assert forced.lowrank_launches() == n0 and forced.plane_cache()[0] > 0
    assert gamma(plain, c["R"]["ref"], c["R"]["B"]) <= D.bound("planes_lw", c["n_g"])
    with pytest.raises(ValueError):
        forced.debug_project_only(0, c["r"], c["k"], frames=(16, 48), route=True)


# ---- rows: the D pass's 512-row blocks (256 k-vectors), the combine's 64-row stages and its groups of four ------------
@pytest.mark.parametrize("K", ROWS)
def test_rows(forced, K):
    t0 = time.perf_counter()
    c = _case(K=K)
    _check(c, _run(forced, c), t0)


# ---- atom stages by the count the kernels run (even: _run asserts it): where the D pass's prefetch depth meets the end
# (2, 4, 6), where the last stages' prefetch wraps the ring (36, 38; 76, 78) and the ends of the unrolled period (40, 42;
# 80, 82), each with a full last stage, a ragged one and one that is all padding -----------------------------------------
@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("stages", DEVICE_STAGES)
def test_device_stages(forced, stages, tail):
    t0 = time.perf_counter()
    c = _case(n=32 * stages - TAILS[tail])
    assert E.device_stages(c["n_g"]) == stages
    _check(c, _run(forced, c), t0)


# ---- the same axis by n_g = 32 S and 32 S - 5: atom counts whose last data stage is odd or even, full or ragged.  The
# kernels run device_stages(n_g) of them (printed), so S = 1 and 2, 3 and 4, 39 and 40, 79 and 80 share their stage count ---
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("S", STAGES)
def test_atom_stages(forced, S, ragged):
    t0 = time.perf_counter()
    c = _case(n=32 * S - (5 if ragged else 0))
    assert E.stages(c["n_g"]) == S and E.device_stages(c["n_g"]) == S + S % 2
    _check(c, _run(forced, c), t0)


@pytest.mark.parametrize("S", [3, 38, 40, 41, 78])
def test_atom_stages_index_list_with_duplicates(forced, S):
    """(4, 38, 40, 42 and 78 stages run)"""
    t0 = time.perf_counter()
    n_g = 32 * S - 5
    c = _case(n=n_g + 40, idx=_dup_list(n_g + 40, n_g, 31))
    assert E.stages(c["n_g"]) == S and len(set(c["idx"].tolist())) < n_g
    _check(c, _run(forced, c), t0)


# ---- frames: 16-frame groups, the D pass's 64-frame tiles, the combine's 256-frame blocks ------------------------------
@pytest.mark.parametrize("T", FRAMES)
def test_frames(forced, T):
    t0 = time.perf_counter()
    c = _case(T=T)
    _check(c, _run(forced, c), t0)


def test_largest_shape(forced):
    """three 512-row D blocks x 82 stages run (two ring periods and two) x 96 frames"""
    t0 = time.perf_counter()
    c = _case(K=513, n=32 * 81 - 5)
    _check(c, _run(forced, c), t0)


# ---- every input family at the base shape -------------------------------------------------------------------------------
@pytest.mark.parametrize("family", E.FAMILIES)
def test_families(forced, family):
    """Displacement mode is on the route like the others: group_source asks get_planes for planes of positions - mean, and
    whenever that set exists (planes on, the list at least PSA_OPT_PLANES_MIN_K long, an index list seen before or
    PSA_OPT_PLANES_EAGER, finite data, room in HBM) the launch is a planes launch and prepare_lowrank takes it; without the
    set the data is the float32 displacement array and the route is never taken.  _run asserts the launch."""
    t0 = time.perf_counter()
    c = _case(family)
    got = _run(forced, c)
    if family == "zeros":
        assert not got.any(), "an all-zero array must give exactly zero"
    _check(c, got, t0)


# ---- the negative side of Gamma along [-1 -1 0] and a node interval away from Gamma: other nodes, phi, interval != 0 -------
@pytest.mark.parametrize("geom", ["neg_-1-10", "seg_1"])
def test_other_side_and_other_interval(forced, geom):
    t0 = time.perf_counter()
    c = _case(geom=geom)
    assert c["plan"]["interval"] == (-1 if geom.startswith("neg") else 1)
    _check(c, _run(forced, c), t0, tag=f"{geom} (interval {c['plan']['interval']}): ")


# ---- the D pass on its own, by difference --------------------------------------------------------------------------------
_DIFF = {}


def _diff_case(K, S):
    if (K, S) not in _DIFF:
        line, off = E.line_and_scattered(K=K, n=32 * S - 5)
        pl, po = line["plan"], off["plan"]
        for name in ("L", "phi", "kappa"):
            assert np.array_equal(pl[name].view(np.uint8), po[name].view(np.uint8)), f"{name} differs between the two lists"
        assert D_LIMIT[0] <= po["d_bound"] <= D_LIMIT[1], po["d_bound"]
        B = scale_B(line["data"], line["r"])
        ref = project64(off["data"], off["r"], off["k"]) - project64(line["data"], line["r"], line["k"])
        _DIFF[(K, S)] = (line, off, B, ref, E.bound_diff_abs(line, off, B))
    return _DIFF[(K, S)]


@pytest.mark.parametrize("K", [40, 257])
@pytest.mark.parametrize("S", [1, 3, 38, 40, 41, 78])
def test_d_pass_by_difference(forced, S, K):
    """got(scattered) - got(on the line): node rows and combine are the same arithmetic in both runs (the plan tables are
    bit-equal), so what is left is the two D terms and one float32 rounding of each final sum.  n_g = 32 S - 5: the D pass
    runs 2, 4, 38, 40, 42 and 78 stages"""
    t0 = time.perf_counter()
    line, off, B, ref, babs = _diff_case(K, S)
    got = _run(forced, off).astype(np.complex128) - _run(forced, line).astype(np.complex128)
    e, at = E.excess(got, ref, babs)
    size = float(np.max(np.maximum(np.abs(ref.real), np.abs(ref.imag)) / B[None]))
    msg = (f"D by difference K={K} n_g={line['n_g']} S={S} ({E.device_stages(line['n_g'])} stages run) T={got.shape[2]} d_bound {off['plan']['d_bound']:.2e}: worst element "
           f"{at} at {e:.3f} x its bound, gamma {gamma(got, ref, B) / U:.2f} u of a bound of {float(babs.max() / B.max()) / U:.2f} u, "
           f"the D difference itself up to {size / U:.0f} u, {time.perf_counter() - t0:.2f} s")
    print(msg)
    assert e <= 1, msg
