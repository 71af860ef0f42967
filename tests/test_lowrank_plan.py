"""The host plan of the low-rank route for k-paths (api_lowrank.hip, psa_lowrank_plan): which lists it serves, that
its combine matrix times the node exponentials gives the line's phases, that its bound on D holds, and that it does
not depend on how a path is split.  No GPU: the plan is host code, the D-pass kernel is checked by its resources."""
import re

import numpy as np
import pytest

from kernel_build import device_compile
from lowrank_cases import D_LIMIT, DIRECTIONS, LIMITS, geometry, mass_weights


def _path(cfg):
    from psa_amd import synth
    from psa_amd.core.sed_calculator import SEDCalculator
    from psa_amd.core.trajectory import Trajectory
    spec, req = synth.baseline_spec(cfg)
    r0, types, box = synth.lattice(spec.cells)
    stub = np.zeros((1, spec.n_atoms, 3), np.float32)
    calc = SEDCalculator(Trajectory(stub, stub, types, np.zeros(1, np.float32), box, np.diag(box).copy(),
                                    np.zeros(3, np.float32), spec.dt_ps), *spec.cells)
    if req["kind"] != "path":
        return r0, None, calc
    _, vecs = calc.get_k_path(req["direction"], req["bz_coverage"], req["n_k"])
    return r0, np.asarray(vecs, np.float32), calc


def _check_plan(p, vecs, r0, n_atoms=4096):
    r = r0[np.linspace(0, len(r0) - 1, n_atoms).astype(int)].astype(np.float64)
    x = r @ p["u"]
    W = np.exp(1j * (r @ p["k0"]))[None, :] * np.exp(1j * np.outer(p["kappa"], x - p["x_c"]))      # (64, A)
    kap = (vecs.astype(np.float64) - p["k0"]) @ p["u"]
    kline = p["k0"][None, :] + kap[:, None] * p["u"][None, :]
    exact = np.exp(1j * (kline @ r.T))
    got = p["C"].astype(np.complex128) @ W
    # C is stored as complex64: 2^-24 per entry, summed over 64 nodes with a Lebesgue constant of a few
    assert np.max(np.abs(got - exact)) < 1e-6
    # in fp64 (C rebuilt from the nodes) the interpolation itself is exact to 1e-10
    bw = (-1.0) ** np.arange(64) * np.sin(np.pi * (2 * np.arange(64) + 1) / 128)
    L = bw[None, :] / (kap[:, None] - p["kappa"][None, :])
    L /= L.sum(axis=1, keepdims=True)
    got64 = (np.exp(1j * kap * p["x_c"])[:, None] * L) @ W
    assert np.max(np.abs(got64 - exact)) < 1e-10
    # the reference's float32 phases stay within the bound of the line's
    rf = r.astype(np.float32)
    k32 = vecs.astype(np.float32)
    arg = np.float32(k32[:, None, 2] * rf[None, :, 2] + (k32[:, None, 1] * rf[None, :, 1] + k32[:, None, 0] * rf[None, :, 0]))
    assert np.max(np.abs(np.exp(1j * arg.astype(np.float64)) - exact)) <= p["d_bound"]
    assert p["d_bound"] <= 2.0 ** -13 and p["d_bound"] * p["dscale"] <= 2.0 ** 14


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C5"])
def test_paths_get_a_plan(cfg):
    from psa_amd import _hip
    r0, vecs, _ = _path(cfg)
    p = _hip.lowrank_plan(vecs, r0)
    assert p is not None and p["interval"] == 0
    _check_plan(p, vecs, r0)


def test_golden_large_phase_path():
    """A path whose phases reach far (the large-phase golden cases' regime): positions pushed out by 100."""
    from psa_amd import _hip
    r0, vecs, _ = _path("C2")
    r = (r0[:8192] + np.float32(100.0)).astype(np.float32)
    p = _hip.lowrank_plan(vecs, r)
    if p is not None:
        _check_plan(p, vecs, r)


def test_grids_offline_and_nan_fall_back():
    from psa_amd import _hip
    r0, vecs, calc = _path("C3")
    rng = np.random.default_rng(3)
    assert _hip.lowrank_plan(rng.normal(size=(64, 3)).astype(np.float32), r0) is None              # off the line
    bent = vecs.copy()
    bent[len(bent) // 2:, 2] += np.float32(0.01)
    assert _hip.lowrank_plan(bent, r0) is None
    bad = vecs.copy()
    bad[5, 0] = np.nan
    assert _hip.lowrank_plan(bad, r0) is None
    bad_r = r0.copy()
    bad_r[7, 1] = np.inf
    assert _hip.lowrank_plan(vecs, bad_r) is None
    g = np.stack(np.meshgrid(np.linspace(-1, 1, 8), np.linspace(-1, 1, 8), [0.0], indexing="ij"), -1).reshape(-1, 3)
    assert _hip.lowrank_plan(g.astype(np.float32), r0) is None                                     # a grid (C4's kind)
    assert _hip.lowrank_plan(vecs[:1], r0) is None


def test_lines_it_declines():
    """Lines the float32 k-vectors do not determine exactly -- off Gamma, or along a direction that is not a lattice
    direction -- and lists that cross Gamma stay on the dense kernels (their plan would depend on the sub-list)."""
    from psa_amd import _hip
    r0, vecs, _ = _path("C3")
    shifted = vecs + np.float32([0.0123, 0.0456, 0.0789])
    assert _hip.lowrank_plan(shifted, r0) is None
    assert _hip.lowrank_plan(shifted[128:], r0) is None
    t = np.linspace(0.0, 0.8, 200)[:, None]
    odd = (t * np.array([1.0, 0.3127, 0.0713]) / np.linalg.norm([1.0, 0.3127, 0.0713])).astype(np.float32)
    assert _hip.lowrank_plan(odd, r0) is None
    crossing = np.concatenate([-vecs[:0:-1], vecs])
    assert _hip.lowrank_plan(crossing, r0) is None


@pytest.mark.parametrize("sign", [1, -1])
def test_sub_lists_get_the_same_plan(sign):
    """Halves, thirds, an inner slice -- of the path and of its mirror image (Gamma towards -[110]): the same u, k0,
    interval, nodes and, row by row, the same C, bit for bit."""
    from psa_amd import _hip
    r0, vecs, _ = _path("C3")
    vecs = (sign * vecs).astype(np.float32)
    whole = _hip.lowrank_plan(vecs, r0)
    assert whole is not None and whole["interval"] == (0 if sign > 0 else -1)
    _check_plan(whole, vecs, r0)
    for lo, hi in [(0, 128), (128, 256), (0, 96), (96, 200), (200, 256), (37, 219)]:
        p = _hip.lowrank_plan(vecs[lo:hi], r0)
        assert p is not None
        for key in ("u", "k0", "kappa"):
            assert np.array_equal(p[key], whole[key]), key
        for key in ("x_c", "h_x", "width", "interval"):
            assert p[key] == whole[key], key
        assert np.array_equal(p["C"].view(np.uint32), whole["C"][lo:hi].view(np.uint32))


def test_index_list_group():
    from psa_amd import _hip
    r0, vecs, _ = _path("C3")
    idx = np.arange(0, len(r0), 2, dtype=np.int32)
    p = _hip.lowrank_plan(vecs, r0, idx)
    assert p is not None
    _check_plan(p, vecs, r0[idx])


def test_diff_kernel_uses_no_scratch():
    """The D pass waits for its LDS-DMA with a counted vmcnt: no scratch, no spill (tests/test_kernel_resources.py)."""
    res = device_compile("k1_planes_diff.hip")
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stderr)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", res.stderr)]
    assert scratch and all(s == 0 for s in scratch), res.stderr[-1500:]
    assert all(s == 0 for s in spills), spills
    asm = res.asm
    assert "scratch_" not in asm
    # two instantiations x 40 unrolled stages x 16 row tiles x 3 components
    assert asm.count("v_mfma_f32_16x16x32_f16") == 2 * 40 * 48


# ---- the geometries of the GPU envelope (tests/test_gpu_lowrank_envelope.py): the premises it rests on ------------
@pytest.mark.parametrize("name", DIRECTIONS + LIMITS + ["plain_100"])
def test_envelope_geometries(name):
    """Each geometry gets its node interval, and the plan's interpolation and bound on D hold."""
    from psa_amd import _hip
    k, r, interval = geometry(name)
    p = _hip.lowrank_plan(k, r)
    assert p is not None and p["interval"] == interval, name
    _check_plan(p, k, r)
    if name in LIMITS:
        assert D_LIMIT[0] <= p["d_bound"] <= D_LIMIT[1], p["d_bound"]     # D at its limit: really there


def test_envelope_weighted_limit_keeps_its_plan():
    """Per-atom weights do not enter the plan: the weighted case runs on the shifted geometry's plan and bound."""
    from psa_amd import _hip
    k, r, _ = geometry("limit_shift")
    w = mass_weights(len(r), 4)
    assert 1.0 <= w.min() and w.max() <= 240.0 and w.max() / w.min() > 200
    p = _hip.lowrank_plan(k, r)
    assert D_LIMIT[0] <= p["d_bound"] <= D_LIMIT[1]


@pytest.mark.parametrize("group", ["one_atom", "slab", "whole"])
def test_envelope_groups_have_finite_normalised_rows(group):
    """The incoherent case's groups: one atom (h_x clamped to 1e-12, an interval 6e13 wide), a 2 A slab across u and
    the whole box get different plans, each with finite rows of C whose Lagrange weights sum to one."""
    from psa_amd import _hip
    k, r, _ = geometry("plain_100")
    x_u = r[:, 0]
    idx = {"one_atom": np.array([int(np.argmin(x_u))], np.int32),
           "slab": np.flatnonzero((x_u > 5.0) & (x_u < 7.0)).astype(np.int32),
           "whole": None}[group]
    p = _hip.lowrank_plan(k, r, idx)
    assert p is not None and p["interval"] == 0
    whole = _hip.lowrank_plan(k, r)
    if group != "whole":
        assert p["x_c"] != whole["x_c"] and p["width"] != whole["width"]
    if group == "one_atom":
        assert p["h_x"] == 1e-12 and p["width"] == pytest.approx(6e13)
    C = p["C"].astype(np.complex128)
    assert np.all(np.isfinite(C))
    # C[j, l] = exp(i kappa_j x_c) L_l(kappa_j): the row sums are unit phases
    kap = k.astype(np.float64) @ p["u"]
    np.testing.assert_allclose(C.sum(axis=1), np.exp(1j * kap * p["x_c"]), rtol=0, atol=1e-5)
    _check_plan(p, k, r if idx is None else r[idx])
