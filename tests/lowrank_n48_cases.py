"""Model and per-element bound of the 48-NODE folded low-rank k-path route (psa_set_k1_lowrank_nodes: api_lowrank.hip,
node_table_n48_kernel and diff_n48_table_kernel in k1_planes_diff.hip, k1_lowrank_n48.hip or the two-product node pass of
k1_planes_lw.hip and the D pass), on the inputs and references of tests/lowrank_env_cases.py.  Shared by
tests/test_lowrank_n48_host.py and tests/test_gpu_lowrank_n48.py.  NumPy and the host-only plan.

The identity.  q = phi L (W_hi v_hi + W_hi v_lo) + D' v_hi with D' = P_ref w - phi L W_hi: whatever the 48 node rows' hi piece
does not carry -- D = (P_ref - P_line) w, E = phi L W_lo, the interpolation residual R = P_line - phi L W (<= 4.6e-7 over a
whole node interval at h_k h_x = 30) and the float32 rounding of phi and L on the v_hi term -- meets v_hi through the image.

Model.  model_n48 restates it with float64 accumulation: node rows from [(y1, x1), (y1, x2)] (y1: the float16 hi piece of the
48-node table times 2^14), combined with the 48-node plan's float32 L and phi; the image (P_ref w - phi (L @ y1) / 2^14)
dscale_fold taken in float64 and rounded ONCE to float16; times x1 only.  lose= plants faults: no_lo (the image built from
the table's value y1 + y2 instead of its hi piece: W_lo's share is then in neither place), tile=i (D' of the 16-row tile i,
eight k-vectors, zeroed), l64 (the image built from the 64-node plan's L, phi and table against 48-node node rows),
no_residual (the image without R: D + E alone, as the 64-node route builds it).

Bound.  Derived, never measured from a kernel: the bound of tests/lowrank_fold_cases.py on the 48-node plan's L and phi with
d_bound + e_bound + r_bound in the D' term,
    lowrank_env_cases.bound_abs + (fold_terms(n_g, d_bound, e_bound + r_bound) - d_terms(n_g, d_bound)) B,
r_bound the plan's fp64 maximum of |R| over its rows and the group's atoms, held to 1e-6, the cap a launch scales the image
by."""
import numpy as np

import dense_cases as D
import lowrank_env_cases as E
import lowrank_fold_cases as F

U = E.U
NODES = 48
R_MAX = 1e-6                                    # api_lowrank.hip: LR48_R_MAX
LEBESGUE_48 = 3.5                               # sum_l |L_l| of 48 Chebyshev points of the first kind: (2 / pi) ln 48 + 1 = 3.46


def plan48(c):
    from psa_amd import _hip
    p = _hip.lowrank_plan_nodes(c["k"], c["r"], c["idx"], NODES)
    assert p is not None, "the 48-node plan declines a list the 64-node plan takes"
    return p


def case(family="quiet_frames", **kw):
    """lowrank_env_cases.case with the 48-node plan as c["plan"] (the 64-node one stays in c["plan64"])"""
    c = E.case(family, **kw)
    c["plan64"] = c["plan"]
    c["plan"] = plan48(c)
    return c


def plan_caps_n48(plan):
    """the 48-node plan's quantities that enter the bound, held to what is known without the plan"""
    E.plan_caps(plan)
    assert plan["L"].shape[1] == NODES and plan["kappa"].shape == (NODES,)
    lam = np.abs(plan["L"].astype(np.float64)).sum(axis=1)
    assert float(lam.max()) <= LEBESGUE_48, float(lam.max())
    rot = np.abs(plan["phi"].real.astype(np.float64)) + np.abs(plan["phi"].imag.astype(np.float64))
    want = float((rot * lam).max()) * 2.0 ** -12
    assert abs(plan["e_bound"] - want) <= 1e-12 * want, (plan["e_bound"], want)
    assert 0 < plan["e_bound"] <= F.E_MAX
    assert 0 <= plan["r_bound"] <= R_MAX, plan["r_bound"]
    s = float(plan["dscale_fold"])
    assert s > 0 and np.log2(s) == round(np.log2(s)), f"dscale_fold {s} is no power of two"
    assert 2.0 ** 13 < (plan["d_bound"] + plan["e_bound"] + R_MAX) * s <= 2.0 ** 14, (plan["d_bound"], plan["e_bound"], s)


def bound_abs_n48(c, R):
    """(K, 3, T) float64: the 48-node route's bound of every element, absolute; c = case(...), R = lowrank_env_cases.reference(c)"""
    p = c["plan"]
    plan_caps_n48(p)
    extra = F.fold_terms(c["n_g"], p["d_bound"], p["e_bound"] + p["r_bound"]) - E.d_terms(c["n_g"], p["d_bound"])
    assert extra > 0
    return E.bound_abs(c, R) + extra * R["B"][None, :, :]


def _f16_once(x):
    """float64 -> float16 in one rounding, as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def model_n48(c, lose=None):
    """(K, 3, T) complex128: the 48-node route restated (module docstring)"""
    plan, lose = c["plan"], lose or {}
    d, P, g = D.group_inputs(c)
    wn, wscale = D.f16_weights(c, g)
    wn64 = 1.0 if wn is None else wn.astype(np.float64)[None, None, :]
    x1, x2, vscale = D.f16_data(d)
    # node rows: two products with the hi piece
    W = E.node_table64(c, plan)
    y1, y2 = D.f16_pieces(np.stack([W.real, W.imag]) * wn64 * 2.0 ** 14)
    Qn = D._accumulate([(y1, x1), (y1, x2)], wscale / (vscale * 2.0 ** 14))
    s = np.einsum("jl,lct->jct", plan["L"].astype(np.float64), Qn, optimize=True)
    q = plan["phi"].astype(np.complex128)[:, None, None] * s
    # the image: P_ref w - phi L W_hi, one float16 rounding
    Pw = P.astype(np.float64) * wn64
    if lose.get("l64"):
        p64 = c["plan64"]
        W64 = E.node_table64(c, p64)
        z1 = D.f16_pieces(np.stack([W64.real, W64.imag]) * wn64 * 2.0 ** 14)[0]
        carried = F.e_table(c, p64, z1)
    elif lose.get("no_lo"):
        carried = F.e_table(c, plan, y1.astype(np.float64) + y2.astype(np.float64))
    elif lose.get("no_residual"):
        Pl = E.line_phases64(c, plan)
        carried = (Pl.real + 1j * Pl.imag) * (1.0 if wn is None else wn.astype(np.float64)[None, :]) - F.e_table(c, plan, y2)
    else:
        carried = F.e_table(c, plan, y1)
    scale = float(plan["dscale_fold"])
    D16 = _f16_once((Pw - np.stack([carried.real, carried.imag])) * scale)
    if "tile" in lose:
        j0 = 8 * lose["tile"]
        assert j0 < D16.shape[1]
        D16[:, j0:j0 + 8, :] = 0
    return q + D._accumulate([(D16, x1)], wscale / (vscale * scale))
