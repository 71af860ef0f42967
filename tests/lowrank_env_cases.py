"""Inputs, model and per-element bound of the low-rank k-path route (api_lowrank.hip, k1_planes_lw.hip on the node table,
k1_planes_diff.hip, lowrank_combine.hip) before the FFT, shared by the host proof (tests/test_lowrank_envelope_host.py)
and the GPU suite (tests/test_gpu_lowrank_perelement.py).  Seeded, NumPy and the host-only plan (psa_lowrank_plan).

Inputs.  The families of tests/dense_cases.py (quiet frames, slow atoms, a coherent row, maxima on a power of two,
weights, displacement mode, zeros) on a k-path from Gamma along [100] and positions in a 40 A box centred on the origin
(tests/lowrank_cases.py), which the plan takes in one node interval.  Base shape K = 40, n_g = 257, T = 96.
The displacements family is the exception: dense_cases.case replaces the positions by the float32 frame mean of its own
trajectory, a 10 A box 40 - 50 A from the origin, and the plan is made on those: h_x = 5 instead of 20 (a node interval four
times as wide), x_c = 45 (phi far from 1, rot up to sqrt 2), d_bound 1.9e-5 instead of 8e-6.

Atom stages.  The route reads the group's cached planes, whose atom axis is padded to 64 (k1_pair_atom_pad), so the node
pass and the D pass always run an EVEN number of 32-atom stages: device_stages(n_g) = 2 ceil(n_g / 64); the stages past
n_g hold zeros.  The bound keeps S = ceil(n_g / 32), the stages that carry data.

Model.  model_lowrank restates the route with float64 accumulation, so only its splits and tables are modelled:
  node table  W[l, a] = w_a exp(i (k0.r_a + kappa_l (u.r_a - x_c))) in float64 from the plan's kappa, u, x_c, times 2^14, in two
              float16 pieces; node rows Qn[l] = the three kept products with the two pieces of d (dense_cases.f16_data)
  combine     s[j] = sum_l L[j, l] Qn[l], then phi[j] s[j], with the plan's own float32 L and phi
  D           (P_ref - P_line) dscale: P_ref the float32 sincos of the float32 phase argument, P_line = exp(i kappa_j u.r_a)
              in float64, the plan's dscale; rounded to ONE float16 piece; times the hi piece of d only
lose= plants faults: x2 (frames whose second piece of d is lost in the node rows), d_frames (frames whose D term is lost),
d_tile (one 16-row tile of the D image lost: rows 2 j + (re, im), so eight k-vectors), d_comp (D meets the hi piece of the
next component).

Bound.  Derived, never measured from the kernels.  Per output element (j, c, t), real and imaginary parts on their own,
|q_gpu - q_64| <= bound_abs, with u = 2^-24, S = ceil(n_g / 32), B = B[c, t] = sum_a |w_a d[t, a, c]| (tests/ref64.py),
Lam_j = sum_l |L[j, l]|, rot_j = |Re phi_j| + |Im phi_j| <= sqrt 2, Qn64 the float64 node rows of the inputs (never the
device's), N_j = sum_l |L[j, l]| |Qn64[l, c, t]| <= Lam_j B:
  node rows   each part of each Qn[l] is a k1_planes_lw output: within dense_cases.bound("planes_lw", n_g) B =
              (6 + 8 + ceil(S / 8)) u B (3u split, 2u table, 1u store, 8u chain, 1u per fold).  Through the real weights the
              parts of s[j] are off by Lam_j times that, and through the rotation by phi a part of phi s is off by
              |Re phi| e_re + |Im phi| e_im:                                 rot_j Lam_j (14 + ceil(S / 8)) u B
  combine     the 64-term float32 FMA chain sum_l L Qn[l] (l in order, one rounding each): 64 u sum_l |L| |Qn[l]|; the
              float32 roundings of L and of phi (api_lowrank.hip: each rounded once from fp64): 1 u each; phase_add's
              product and fma (lowrank_combine.hip): 2 u of |phi_r s_r| + |phi_i s_i| <= |s|; with the device's
              |Qn| <= |Qn64| + node error:                                   68 u (N_j + Lam_j (14 + ceil(S / 8)) u B)
  D pass      d_bound, the plan's bound on |D| (api_lowrank.hip).  D dscale goes to float32 and then to float16:
              2^-11 (1 + 2^-13) d_bound (dscale puts d_bound in (2^13, 2^14]: normal float16 range); it meets the hi piece
              of d only (k1_f16.h: |d - x1| <= 2^-11 |d|): another 2^-11 d_bound; one unfolded MFMA chain over all stages
              (DESIGN.md rule 3: S 2^-24 per chain of S stages): S u d_bound; and D is built from the device's sincosf where
              the reference has the exact sincos of the float32 argument, the 2u of the dense bounds' table:
                                                                             ((2^-10 (1 + 2^-14) + S u) d_bound + 2 u) B
  final sum   o + phi s is rounded once, |q| <= B:                           1 u B
  interpolation  64 Chebyshev nodes on h_k h_x <= 30 (api_lowrank.hip): 30^64 / (2^63 64!) = 3e-14 per atom, and the fp64
              rounding of L, of the order of 64 Lam 2^-53:                   2^-40 B (the host proof checks the node sum)
At the base shape Lam <= 3.61, S = 9: node rows 58 u, combine 68 u N / B = 44 u where N / B is largest (0.64), D and the final
sum 3.2 u: about 100 u at the worst element, less where the node rows are small.  The bound assumes what the dense one
does: data inside the envelope of the "2 x f16" split (dense_cases.py).

The D pass by difference.  Two lists with the same kappa_j -- every vector on the line, and the same with a perpendicular
scatter (lowrank_cases.scattered) -- have bit-equal L, phi and kappa, and the same node rows, so got_scattered - got_line
is the difference of the two D terms plus one rounding of each final sum.  bound_diff: the D terms of both lists and 2 u,
((2^-10 (1 + 2^-14) + S u) (d_bound_s + d_bound_l) + 4 u + 2 u) B: 6 u and a little, against a D term of tens of u.

Lam_j, rot_j and d_bound come from the plan, which also feeds the device, so bound_abs first holds the plan to what is known
without it (plan_caps): Lam_j <= (2 / pi) ln 64 + 1 = 3.65, the Lebesgue constant of 64 Chebyshev points of the first kind,
|phi_j| <= 1 + 2^-23, d_bound <= 2^-13 (the plan's own acceptance).  With N_j <= Lam_j B that caps every bound at
bound_units(n_g, 3.65, sqrt 2, 3.65, 2^-13) = (sqrt 2 3.65 (14 + ceil(S / 8)) + 68 3.65 + 5) u, 336 u at S = 9, whatever the
plan says."""
import math

import numpy as np

import dense_cases as D
from lowrank_cases import box, k_vectors, scattered
from ref64 import project64, scale_B

U = D.U
BASE = dict(K=40, n=257, T=96)
EDGE = 40.0                                   # the box: centred on the origin
NODES = 64
CHAIN = 64 + 4                                # the combine: 64 FMAs, the roundings of L and phi, phase_add's two
INTERP = 2.0 ** -40
LEBESGUE = 2.0 / math.pi * math.log(NODES) + 1.0      # sum_l |L_l| of 64 Chebyshev points of the first kind, anywhere inside
D_MAX = 2.0 ** -13                                    # the plan accepts no larger d_bound
FAMILIES, QUIET_FAMILIES = D.FAMILIES, D.QUIET_FAMILIES


# ---- inputs ---------------------------------------------------------------------------------------------------------
def k_path(K, name="plain_100"):
    """(K, 3) float32: the k-vectors of a geometry of tests/lowrank_cases.py"""
    return k_vectors(name, K)[0]


def case(family, K=None, n=None, T=None, quiet_exp=-10, geom="plain_100", idx=None, k=None):
    """dense_cases.case of the family on a k-path and centred positions, with its plan (c["plan"], asserted to take the
    list).  idx: an index-list group; k: these k-vectors instead of the geometry's"""
    from psa_amd import _hip
    K, n = K or BASE["K"], n or BASE["n"]
    T = T or (160 if family == "quiet_blocks" else BASE["T"])
    r = box(n, EDGE, 100 + FAMILIES.index(family), -EDGE / 2)
    c = D.case(family, K=K, n=n, T=T, quiet_exp=quiet_exp, r=r, k=k_path(K, geom) if k is None else k)
    if idx is not None:
        c = D.with_idx(c, idx)
    c["plan"] = _hip.lowrank_plan(c["k"], c["r"], c["idx"])
    assert c["plan"] is not None, f"{family} K={K} n_g={c['n_g']} {geom}: the plan declines the list"
    return c


def line_and_scattered(family="quiet_frames", K=None, n=None, T=None, sigma=1e-6, seed=2):
    """(case on the [100] path, the same case with a perpendicular scatter of sigma per component): the same data,
    positions and kappa"""
    line = case(family, K=K, n=n, T=T)
    off = dict(line)
    off["k"] = scattered(line["k"], sigma, seed)
    from psa_amd import _hip
    off["plan"] = _hip.lowrank_plan(off["k"], off["r"], off["idx"])
    assert off["plan"] is not None, "the plan declines the scattered list"
    return line, off


# ---- float64 pieces of the route ------------------------------------------------------------------------------------
def _group(c):
    return np.arange(c["data"].shape[1]) if c["idx"] is None else np.asarray(c["idx"], np.int64)


def node_table64(c, plan):
    """(64, n) complex128: W[l, a] = exp(i (k0.r_a + kappa_l (u.r_a - x_c))), without weights"""
    r = c["r"][_group(c)].astype(np.float64)
    return np.exp(1j * ((r @ plan["k0"])[None, :] + plan["kappa"][:, None] * (r @ plan["u"] - plan["x_c"])[None, :]))


def line_phases64(c, plan):
    """(K, n) complex128: exp(i k~_j.r_a), k~_j the k-vector projected on the plan's line"""
    r = c["r"][_group(c)].astype(np.float64)
    kap = (c["k"].astype(np.float64) - plan["k0"]) @ plan["u"]
    return np.exp(1j * ((r @ plan["k0"])[None, :] + kap[:, None] * (r @ plan["u"])[None, :]))


def reference(c):
    """dict(ref (K, 3, T) complex128, B (3, T), Qn (64, 3, T) complex128 float64 node rows): reference quantities only"""
    args = (c["data"], c["r"])
    W = node_table64(c, c["plan"])
    d, _, g = D.group_inputs(c)
    if c["weights"] is not None:
        W = W * c["weights"][g].astype(np.float64)[None, :]
    Qn = np.einsum("la,tac->lct", W, d.astype(np.float64), optimize=True)
    return dict(ref=project64(*args, c["k"], c["idx"], c["weights"], c["disp"]),
                B=scale_B(*args, c["idx"], c["weights"], c["disp"]), Qn=Qn)


# ---- the bound --------------------------------------------------------------------------------------------------------
def stages(n_g):
    """32-atom stages that carry data: the S of the bound"""
    return -(-int(n_g) // 32)


def device_stages(n_g):
    """32-atom stages the route's kernels run: the planes pad the atom axis to 64, so they come in pairs"""
    return 2 * -(-int(n_g) // 64)


def plan_caps(plan):
    """the plan's quantities that enter a bound, held to what is known without the plan"""
    lam = float(np.abs(plan["L"].astype(np.float64)).sum(axis=1).max())
    assert lam <= LEBESGUE, f"sum_l |L[j, l]| = {lam} exceeds the Lebesgue constant {LEBESGUE:.3f}"
    assert float(np.abs(plan["phi"].astype(np.complex128)).max()) <= 1 + 2.0 ** -23, "|phi| > 1"
    assert 0 < plan["d_bound"] <= D_MAX, plan["d_bound"]


def d_terms(n_g, d_bound):
    """the D pass's share in units of B: D to float16, the hi piece alone, the unfolded chain, the device's sincosf"""
    return (2.0 ** -10 * (1 + 2.0 ** -14) + stages(n_g) * U) * d_bound + 2 * U


def bound_units(n_g, lam, rot, n_over_B, d_bound):
    """the bound of one element in units of its B: lam = sum_l |L[j, l]|, rot = |Re phi_j| + |Im phi_j|, n_over_B =
    sum_l |L[j, l]| |Qn64[l, c, t]| / B[c, t]"""
    node = D.bound("planes_lw", n_g)
    return rot * lam * node + CHAIN * U * (n_over_B + lam * node) + d_terms(n_g, d_bound) + U + INTERP


def bound_abs(c, R):
    """(K, 3, T) float64: the bound of every element, absolute (zero exactly where B is zero); R = reference(c)"""
    p = c["plan"]
    plan_caps(p)
    aL = np.abs(p["L"].astype(np.float64))
    lam = aL.sum(axis=1)[:, None, None]
    rot = (np.abs(p["phi"].real.astype(np.float64)) + np.abs(p["phi"].imag.astype(np.float64)))[:, None, None]
    N = np.einsum("jl,lct->jct", aL, np.abs(R["Qn"]), optimize=True)
    B = R["B"][None, :, :]
    # bound_units, its n_over_B B = N kept absolute so that B = 0 divides nothing
    return bound_units(c["n_g"], lam, rot, 0.0, p["d_bound"]) * B + CHAIN * U * N


def bound_diff_abs(line, off, B):
    """(1, 3, T): the bound of got_scattered - got_line against project64(scattered) - project64(line)"""
    n_g = line["n_g"]
    plan_caps(line["plan"])
    plan_caps(off["plan"])
    return ((d_terms(n_g, line["plan"]["d_bound"]) + d_terms(n_g, off["plan"]["d_bound"]) + 2 * U) * B)[None, :, :]


def excess(got, ref, babs):
    """(largest |got - ref| / bound over all elements, real and imaginary parts on their own; its index (j, c, t)).
    Elements whose bound is zero (B = 0) must be exactly zero in got (asserted) and are left out."""
    got, ref = np.asarray(got), np.asarray(ref)
    babs = np.broadcast_to(babs, ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.maximum(np.abs(got.real.astype(np.float64) - ref.real), np.abs(got.imag.astype(np.float64) - ref.imag))
    live = babs > 0
    assert not np.any(got[~live]), "elements whose scale B is zero must be exactly zero"
    if not live.any():
        return 0.0, (0, 0, 0)
    ratio = np.where(live, err / np.where(live, babs, 1.0), 0.0)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


# ---- the model ------------------------------------------------------------------------------------------------------
def model_lowrank(c, plan=None, lose=None):
    """(K, 3, T) complex128: the route restated (module docstring).  lose: dict(x2=frames, d_frames=frames, d_tile=i,
    d_comp=True)"""
    plan, lose = plan or c["plan"], lose or {}
    d, P, g = D.group_inputs(c)
    wn, wscale = D.f16_weights(c, g)
    wn64 = 1.0 if wn is None else wn.astype(np.float64)[None, None, :]
    x1, x2, vscale = D.f16_data(d, lose.get("x2"))
    # node rows
    W = node_table64(c, plan)
    y1, y2 = D.f16_pieces(np.stack([W.real, W.imag]) * wn64 * 2.0 ** 14)
    Qn = D._accumulate([(y1, x1), (y2, x1), (y1, x2)], wscale / (vscale * 2.0 ** 14))
    # combine
    s = np.einsum("jl,lct->jct", plan["L"].astype(np.float64), Qn, optimize=True)
    q = plan["phi"].astype(np.complex128)[:, None, None] * s
    # D: one float16 piece, the hi piece of d
    Pl = line_phases64(c, plan)
    Dm = (P.astype(np.float64) - np.stack([Pl.real, Pl.imag])) * float(plan["dscale"]) * wn64
    D16 = D._f16(Dm.astype(np.float32))
    if "d_tile" in lose:
        j0 = 8 * lose["d_tile"]
        assert j0 < D16.shape[1]
        D16[:, j0:j0 + 8, :] = 0
    xd = x1
    if "d_frames" in lose:
        xd = x1.copy()
        xd[lose["d_frames"]] = 0
    if lose.get("d_comp"):
        xd = np.roll(xd, 1, axis=2)
    return q + D._accumulate([(D16, xd)], wscale / (vscale * float(plan["dscale"])))


def interpolation_error(c):
    """max over (j, a) of |phi_j sum_l L[j, l] W[l, a] - exp(i k~_j.r_a)| with the plan's float32 L and phi taken away:
    the fp64 tables rebuilt from kappa (barycentric form), so what is left is the interpolation and fp64 rounding"""
    p = c["plan"]
    kap = (c["k"].astype(np.float64) - p["k0"]) @ p["u"]
    th = math.pi * (2 * np.arange(NODES) + 1) / (2.0 * NODES)
    bw = np.where(np.arange(NODES) % 2 == 1, -1.0, 1.0) * np.sin(th)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = bw[None, :] / (kap[:, None] - p["kappa"][None, :])
        L = L / L.sum(axis=1, keepdims=True)
    hit = kap[:, None] == p["kappa"][None, :]
    L[hit.any(axis=1)] = hit[hit.any(axis=1)].astype(np.float64)
    got = np.exp(1j * kap * p["x_c"])[:, None] * (L @ node_table64(c, p))
    return float(np.max(np.abs(got - line_phases64(c, p))))
