"""Model and per-element bound of the FOLDED low-rank k-path route (psa_set_k1_lowrank_fold: api_lowrank.hip,
diff_fold_table_kernel in k1_planes_diff.hip, k1_lowrank_fold.hip or the two-product node pass of k1_planes_lw.hip and the D
pass), on the inputs, plan and references of tests/lowrank_env_cases.py.  Shared by tests/test_lowrank_fold_host.py and
tests/test_gpu_lowrank_fold.py.  NumPy and the host-only plan.

The identity.  The route computes q = phi L (W_hi v_hi + W_hi v_lo + W_lo v_hi) + D v_hi.  The combine is linear, so
phi L (W_lo v_hi) = E v_hi with E[j, a] = phi_j sum_l L[j, l] W_lo[l, a]: the folded route multiplies two products per node
row and keeps D' = D + E, rounded once, in the D image.

Model.  model_fold restates it with float64 accumulation like lowrank_env_cases.model_lowrank: the node rows from
[(y1, x1), (y1, x2)] (y1, y2: the float16 pieces of the node table times 2^14, x1, x2: those of the data), combined with the
plan's float32 L and phi; the image ((P_ref - P_line) w + phi (L @ (y2_re + i y2_im)) / 2^14) dscale_fold rounded to float32
and then to ONE float16; times x1 only.  lose= plants faults: e_lost (E missing from the image), e_from_hi (E built from the
hi pieces y1), e_tile=i (E of the 16-row tile i, eight k-vectors, missing).

Bound.  Derived, never measured from a kernel.  lowrank_env_cases.bound_abs with the D term's d_bound replaced by
d_bound + e_bound, e_bound = max_j rot_j Lam_j 2^-12 the plan's bound on a part of E (|W_lo| <= 2^-12 per part: the
residual of a float16 piece of a value of at most 1), plus the float32 evaluation of E on the device -- 64 FMAs and
phase_add's two operations, no more than CHAIN u of rot_j Lam_j 2^-12 <= e_bound:
    ((2^-10 (1 + 2^-14) + S u) (d_bound + e_bound) + 2 u + CHAIN u e_bound) B     in place of the D term.
The node rows' term does not grow: they lose a product, and what the split drops, W_lo v_lo = E v_lo, is what it dropped
before.  e_bound is held to what is known without the plan, sqrt 2 x the Lebesgue constant x 2^-12 = 1.26e-3."""
import numpy as np

import dense_cases as D
import lowrank_env_cases as E

U = E.U
E_MAX = 2.0 ** 0.5 * E.LEBESGUE * 2.0 ** -12


def plan_caps_fold(plan):
    """the plan's e_bound and dscale_fold against its own L and phi, and the caps no plan can exceed"""
    E.plan_caps(plan)
    lam = np.abs(plan["L"].astype(np.float64)).sum(axis=1)
    rot = np.abs(plan["phi"].real.astype(np.float64)) + np.abs(plan["phi"].imag.astype(np.float64))
    want = float((rot * lam).max()) * 2.0 ** -12
    assert abs(plan["e_bound"] - want) <= 1e-12 * want, (plan["e_bound"], want)
    assert 0 < plan["e_bound"] <= E_MAX, plan["e_bound"]
    s = float(plan["dscale_fold"])
    assert s > 0 and np.log2(s) == round(np.log2(s)), f"dscale_fold {s} is no power of two"
    assert 2.0 ** 13 < (plan["d_bound"] + plan["e_bound"]) * s <= 2.0 ** 14, (plan["d_bound"], plan["e_bound"], s)


def fold_terms(n_g, d_bound, e_bound):
    """the folded D pass's share in units of B"""
    return E.d_terms(n_g, d_bound + e_bound) + E.CHAIN * U * e_bound


def bound_abs_fold(c, R):
    """(K, 3, T) float64: the folded route's bound of every element, absolute; R = lowrank_env_cases.reference(c)"""
    p = c["plan"]
    plan_caps_fold(p)
    extra = fold_terms(c["n_g"], p["d_bound"], p["e_bound"]) - E.d_terms(c["n_g"], p["d_bound"])
    assert extra > 0
    return E.bound_abs(c, R) + extra * R["B"][None, :, :]


def e_table(c, plan, pieces):
    """(K, n) complex128: phi_j sum_l L[j, l] (pieces_re + i pieces_im)[l, a] / 2^14, the plan's float32 L and phi"""
    z = pieces[0].astype(np.float64) + 1j * pieces[1].astype(np.float64)
    return plan["phi"].astype(np.complex128)[:, None] * (plan["L"].astype(np.float64) @ z) * 2.0 ** -14


def model_fold(c, plan=None, lose=None):
    """(K, 3, T) complex128: the folded route restated (module docstring).  lose: dict(e_lost=True, e_from_hi=True, e_tile=i)"""
    plan, lose = plan or c["plan"], lose or {}
    d, P, g = D.group_inputs(c)
    wn, wscale = D.f16_weights(c, g)
    wn64 = 1.0 if wn is None else wn.astype(np.float64)[None, None, :]
    x1, x2, vscale = D.f16_data(d)
    # node rows: two products
    W = E.node_table64(c, plan)
    y1, y2 = D.f16_pieces(np.stack([W.real, W.imag]) * wn64 * 2.0 ** 14)
    Qn = D._accumulate([(y1, x1), (y1, x2)], wscale / (vscale * 2.0 ** 14))
    s = np.einsum("jl,lct->jct", plan["L"].astype(np.float64), Qn, optimize=True)
    q = plan["phi"].astype(np.complex128)[:, None, None] * s
    # the folded image: one float16 piece of (D + E) dscale_fold
    Et = e_table(c, plan, y1 if lose.get("e_from_hi") else y2)
    if lose.get("e_lost"):
        Et[:] = 0
    if "e_tile" in lose:
        j0 = 8 * lose["e_tile"]
        assert j0 < Et.shape[0]
        Et[j0:j0 + 8] = 0
    Pl = E.line_phases64(c, plan)
    scale = float(plan["dscale_fold"])
    Dm = ((P.astype(np.float64) - np.stack([Pl.real, Pl.imag])) * wn64 + np.stack([Et.real, Et.imag])) * scale
    D16 = D._f16(Dm.astype(np.float32))
    return q + D._accumulate([(D16, x1)], wscale / (vscale * scale))
