"""Inputs, bounds and split models of the dense projection kernels' float64 envelope, shared by the host proof
(tests/test_dense_envelope_host.py) and the GPU suite (tests/test_gpu_dense_envelope.py).  Seeded, NumPy only.

Inputs.  Every family stays inside the documented envelope of the "2 x f16" split (no value that matters lies more than
2^17 below its group's maximum) but has output elements far below the global maximum: quiet frames, slow atoms, one
coherent row among incoherent ones, maxima on a power of two, weights, displacement mode, zeros.

Bounds.  bound(form, n_g) is the per-element error in units of B[c, t] = sum_a |w_a d[t, a, c]| (tests/ref64.py) that
the project's own documents promise, u = 2^-24, S = ceil(n_g / 32) atom stages, F the float32 fold period:
  2 x f16 (k1_pair, k1_planes 32/64/128 rows, k1_planes_lw), F = 8; k1_planes_wide, F = 10 (W_FOLD):
      (6 + F + ceil(S / F)) u: 3u split (k1_f16.h: two residuals and the dropped x2*y2), 2u float32 sincos of the table,
      1u final rounding, F u for one MFMA chain (DESIGN.md rule 3: S * 2^-24 per chain of S stages), 1u per fold
  3 x bf16 (k1_split): (6 + 2 S) u: its hi and lo accumulators are each one chain over all S stages
  k1_mfma, k1_wave: (n_g + 4) u: the worst case of a float32 dot product in any order
None of them is measured from the kernels.

Models.  model_f16 / model_bf16 restate the two splits in NumPy with float64 accumulation, so only the split is modelled;
lose= zeroes the second piece of d on the given frames, the fault the envelope must see."""
import math

import numpy as np

from ref64 import phase_argument

U = 2.0 ** -24
BASE = dict(K=40, n=1000, T=96)
F16_FORMS = ("pair", "planes32", "planes64", "planes128", "planes_lw")
FORMS = F16_FORMS + ("planes_wide", "bf16x3", "mfma32", "wave")


def bound(form, n_g):
    S = -(-int(n_g) // 32)
    if form in F16_FORMS or form == "planes_wide":
        F = 10 if form == "planes_wide" else 8
        return (6 + F + -(-S // F)) * U
    if form == "bf16x3":
        return (6 + 2 * S) * U
    if form in ("mfma32", "wave", "float32"):
        return (n_g + 4) * U
    raise KeyError(form)


# ---- geometry -------------------------------------------------------------------------------------------------------
def positions(n, seed, edge=40.0, shift=0.0):
    """n random float32 positions in a cube of the given edge whose corner is at (shift, shift, shift)"""
    return (np.random.default_rng(seed).random((n, 3)) * edge + shift).astype(np.float32)


def k_list(K, seed=5, kmax=1.5):
    """K random float32 k-vectors, |component| <= kmax: not on one line, no (k, -k) pairs, no twins"""
    return ((np.random.default_rng(seed).random((K, 3)) * 2 - 1) * kmax).astype(np.float32)


def quiet_mask(T, blocks=False):
    """the quiet frames: every third one, or (blocks) one whole 16-frame group and one whole 64-frame tile"""
    t = np.arange(T)
    if blocks:
        return ((t >= 16) & (t < 32)) | ((t >= 64) & (t < 128))
    return t % 3 == 2


def _normal(T, n, seed):
    return np.random.default_rng(seed).standard_normal((T, n, 3)).astype(np.float32)


def _quieten(x, quiet, quiet_exp):
    x = x.copy()
    x[quiet] *= np.float32(2.0 ** quiet_exp)                 # exact
    return x


def species_weights(n, kind, seed=7):
    """per-atom weights of three species: sqrt(m) (O, Si, Hf) or signed charges"""
    vals = np.sqrt(np.float32([15.999, 28.086, 178.49])) if kind == "mass" else np.float32([-2.0, 1.5, 0.5])
    return vals[np.random.default_rng(seed).integers(0, 3, n)].astype(np.float32)


FAMILIES = ["quiet_frames", "quiet_blocks", "slow_atoms", "slow_atoms_group", "coherent", "pow2_max_0", "pow2_max_-30",
            "pow2_max_30", "pow2_max_below_1", "weighted_mass", "weighted_charge", "displacements", "zeros"]
QUIET_FAMILIES = ["quiet_frames", "quiet_blocks", "coherent", "pow2_max_0", "pow2_max_-30", "pow2_max_30",
                  "pow2_max_below_1", "weighted_mass", "weighted_charge"]


def case(family, K=None, n=None, T=None, quiet_exp=-10, r=None, k=None):
    """dict(data (T, N, 3) float32, r (N, 3) float32 mean positions, k (K, 3) float32, idx, weights, disp, quiet (T,) bool
    or None, n_g).  K, n, T default to the family's own shape (BASE; coherent: 4096 atoms; quiet_blocks: 160 frames);
    the quiet frames are 2^quiet_exp of the others.  r, k: the family on these positions and k-vectors instead of its
    own random ones (tests/lowrank_env_cases.py: a k-path; displacement mode keeps its own positions)."""
    K = K or BASE["K"]
    n = n or (4096 if family == "coherent" else BASE["n"])
    T = T or (160 if family == "quiet_blocks" else BASE["T"])
    seed = 100 + FAMILIES.index(family)
    r, k = positions(n, seed) if r is None else r, k_list(K) if k is None else k
    assert r.shape == (n, 3) and k.shape == (K, 3) and r.dtype == k.dtype == np.float32
    out = dict(name=family, r=r, k=k, idx=None, weights=None, disp=False, quiet=None)
    if family in ("quiet_frames", "quiet_blocks", "weighted_mass", "weighted_charge"):
        out["quiet"] = quiet_mask(T, family == "quiet_blocks")
        out["data"] = _quieten(_normal(T, n, seed), out["quiet"], quiet_exp)
        if family.startswith("weighted"):
            out["weights"] = species_weights(n, family.split("_")[1])
    elif family in ("slow_atoms", "slow_atoms_group"):
        x = _normal(T, n, seed)
        lo, hi = n // 3, n // 3 + max(1, n // 3)
        x[:, lo:hi, :] *= np.float32(2.0 ** -8)
        out["data"] = x
        if family == "slow_atoms_group":
            out["idx"] = np.arange(lo, hi, dtype=np.int32)
    elif family == "coherent":
        # row k0 adds up coherently to about B / 2; every other row stays at sqrt(N)
        k0 = k[K // 2].astype(np.float64)
        wave = np.cos(r.astype(np.float64) @ k0)
        x = wave[None, :, None] + 0.05 * np.random.default_rng(seed).standard_normal((T, n, 3))
        out["quiet"] = quiet_mask(T)
        out["data"] = _quieten(x.astype(np.float32), out["quiet"], quiet_exp)
    elif family.startswith("pow2_max"):
        # max|d| exactly 2^e (or the largest float32 below 1), on a loud frame
        tag = family[len("pow2_max_"):]
        top = np.nextafter(np.float32(1), np.float32(0)) if tag == "below_1" else np.float32(2.0 ** int(tag))
        out["quiet"] = quiet_mask(T)
        x = _normal(T, n, seed).astype(np.float64)
        x[out["quiet"]] *= 2.0 ** quiet_exp
        x = (x / np.abs(x).max() * float(top)).astype(np.float32)
        assert np.abs(x).max() == top
        out["data"] = x
    elif family == "displacements":
        # positions 40 units from the origin with 0.05 of thermal motion; the mean is the float32 mean over the frames,
        # as the calculator takes it.  (No quiet frames: a float32 position near 40 leaves a displacement of 0.05 some
        # 14 significant bits, and one 2^10 smaller has none left for a second float16 piece.)
        r0 = positions(n, seed, edge=10.0, shift=40.0)
        out["data"] = (r0[None].astype(np.float64) + 0.05 * np.random.default_rng(seed + 50).standard_normal((T, n, 3))).astype(np.float32)
        out["r"] = np.mean(out["data"], axis=0, dtype=np.float32)
        out["disp"] = True
    elif family == "zeros":
        out["data"] = np.zeros((T, n, 3), np.float32)
    else:
        raise KeyError(family)
    out["n_g"] = n if out["idx"] is None else len(out["idx"])
    return out


def with_idx(c, idx):
    """the case on an index-list group"""
    c = dict(c)
    c["idx"] = np.asarray(idx, np.int32)
    c["n_g"] = len(c["idx"])
    return c


# ---- NumPy models of the two splits ---------------------------------------------------------------------------------
def group_inputs(c):
    """(d (T, n, 3) float32 group data, P (2, K, n) float32 cos / sin table, the group's atoms)"""
    g = np.arange(c["data"].shape[1]) if c["idx"] is None else np.asarray(c["idx"], np.int64)
    d = c["data"][:, g, :]
    if c["disp"]:
        d = d - c["r"][g][None, :, :]
    arg = phase_argument(c["k"], c["r"][g]).astype(np.float64)            # the float32 argument
    P = np.stack([np.cos(arg), np.sin(arg)]).astype(np.float32)           # a correctly rounded float32 sincos
    return np.ascontiguousarray(d, np.float32), P, g


def _f16(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float16).astype(np.float32)


def _bf16(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def _accumulate(terms, scale):
    """(K, 3, T) complex128: sum over the atoms of the kept products, in float64; terms: [(P piece (2, K, n), d piece
    (T, n, 3))]"""
    out = 0.0
    for p, x in terms:
        q = np.einsum("rka,tac->rkct", p.astype(np.float64), x.astype(np.float64), optimize=True)
        out = out + q
    out = out * scale
    return out[0] + 1j * out[1]


def f16_weights(c, g):
    """(w / 2^ew (n,) float32 or None, 2^ew): the group's weights as the "2 x f16" tables carry them, 2^ew >= max|w|"""
    if c["weights"] is None:
        return None, 1.0
    w = c["weights"][g]
    wscale = 2.0 ** math.ceil(math.log2(float(np.abs(w).max())))
    return w * np.float32(1.0 / wscale), wscale


def f16_pieces(x):
    """x1 = f16(x), x2 = f16(x - x1) as float32 arrays; of a float32 x the residual is exact, of a float64 x (the
    low-rank route's node table) it is rounded to float32 once"""
    x1 = _f16(np.asarray(x, np.float32))
    return x1, _f16(np.asarray(x - x1, np.float32))


def f16_data(d, lose=None):
    """(x1, x2, 2^(14-e)): the two float16 pieces of the group data d times 2^(14-e), 2^e >= max|d|; lose: frames whose
    x2 is lost"""
    amax = float(np.abs(d).max())
    vscale = 2.0 ** (14 - math.ceil(math.log2(amax))) if amax > 0 else 1.0
    x1, x2 = f16_pieces(d * np.float32(vscale))
    if lose is not None:
        x2[lose] = 0
    return x1, x2, vscale


def model_f16(c, lose=None):
    """The "2 x f16" split (k1_f16.h): d times 2^(14-e), 2^e >= max|d| of the group; P' = (w / 2^ew) (cos, sin) times
    2^14; each into x1 = f16(x), x2 = f16(x - x1); kept x1 y1 + x1 y2 + x2 y1.  lose: frames whose x2 of d is lost."""
    d, P, g = group_inputs(c)
    wn, wscale = f16_weights(c, g)
    if wn is not None:
        P = P * wn[None, None, :]
    x1, x2, vscale = f16_data(d, lose)
    y1, y2 = f16_pieces(P * np.float32(2.0 ** 14))
    return _accumulate([(y1, x1), (y2, x1), (y1, x2)], wscale / (vscale * 2.0 ** 14))


def model_bf16(c, lose=None):
    """The "3 x bf16" split (k1_split.hip): no scale; x = x1 + x2 + x3 in bf16, residuals exact; kept x1 y1 + x1 y2 +
    x2 y1 + x2 y2 + x1 y3 + x3 y1.  lose: frames whose x2 of d is lost (x3 is still the residual of x - x1 - x2)."""
    d, P, g = group_inputs(c)
    if c["weights"] is not None:
        P = P * c["weights"][g][None, None, :]
    x1 = _bf16(d)
    x2 = _bf16(d - x1)
    x3 = _bf16(d - x1 - x2)
    if lose is not None:
        x2 = x2.copy()
        x2[lose] = 0
    y1 = _bf16(P)
    y2 = _bf16(P - y1)
    y3 = _bf16(P - y1 - y2)
    return _accumulate([(y1, x1), (y2, x1), (y1, x2), (y2, x2), (y3, x1), (y1, x3)], 1.0)


def oracle32(c):
    """(K, 3, T) complex64: the float32 NumPy oracle's projection of the case (oracle/psa_oracle.py)"""
    from oracle import psa_oracle as O
    g = np.arange(c["data"].shape[1]) if c["idx"] is None else np.asarray(c["idx"], np.int64)
    d = c["data"][:, g, :]
    if c["disp"]:
        d = d - c["r"][g][None, :, :]
    P = O.phase_table(c["k"], c["r"][g])
    if c["weights"] is not None:
        P = (P * c["weights"][g][None, :]).astype(np.complex64)
    return np.ascontiguousarray(O.project_group(d, P).transpose(1, 2, 0))
