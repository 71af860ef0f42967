"""Input families of the dynamic-spectra tests, the kernel's per-element bound from reference quantities only, and a
NumPy float32 model of the kernel's arithmetic (psa_amd/csrc/dynamic.hip) -- with the phase formed as the kernel forms it,
or as the float32 FMA chain in radians that it must not be.

The bound, per element of q (K, NC, T) against tests/dynamic64.project64:
    |q - q64| <= (eps_term + (DYN_CHAIN + folds(N_g) + 4) u) sum_a |w_a| |d_a,c(t)|          u = 2^-24
    eps_term = 2 pi 1.51 u + sqrt(2) DYN_SINCOS_ERR,   folds(N_g) = ceil(ceil(N_g / 2) / DYN_CHAIN)
Nothing in it comes from the code under test: u is the float32 unit roundoff, DYN_CHAIN and the strand structure are the
kernel's stated summation order, DYN_SINCOS_ERR is twice the error of the hardware sine and cosine measured against
float64, and sum |w| |d| is computed in float64 from the inputs."""
import math

import numpy as np

from psa_amd import _hip

U = 2.0 ** -24
EPS_TERM_CAP = 2.0 ** -18            # the phase uncertainty a float32 position carries at |k.r| = 64 rad


def folds(n_g):
    return math.ceil(math.ceil(n_g / 2) / _hip.DYN_CHAIN)


def eps_term():
    return 2 * math.pi * 1.51 * U + math.sqrt(2.0) * _hip.DYN_SINCOS_ERR


def bound(absum, n_g):
    """per-element bound for sum_a |w_a| |d_a,c(t)| = absum (any shape)"""
    return (eps_term() + (_hip.DYN_CHAIN + folds(n_g) + 4) * U) * np.asarray(absum, np.float64)


def slices(K):
    """atom slices the lanes of a workgroup are split into for a call of K k-vectors (dynamic_slices)"""
    ks = 1
    while ks < _hip.DYN_THREADS and ks < K:
        ks *= 2
    return _hip.DYN_THREADS // ks


# ---- input families -------------------------------------------------------------------------------------------
BOX = 21.72                          # 4 cells of silicon, Angstrom


def trajectory(n_atoms, n_frames, seed, offset=0.0):
    """(positions, velocities) (T, N, 3) float32: sites scattered over a 21.72 A box, each atom wandering about its
    site by 0.1 A per frame, velocities of order 5 A/ps; offset: added to every coordinate (OFFSET = 1200 A puts |k.r| at
    1e4 rad for the aligned k-vectors of k_list)"""
    rng = np.random.default_rng(seed)
    site = rng.uniform(0.0, BOX, (1, n_atoms, 3))
    pos = (site + 0.1 * rng.standard_normal((n_frames, n_atoms, 3)) + offset).astype(np.float32)
    vel = (5.0 * rng.standard_normal((n_frames, n_atoms, 3))).astype(np.float32)
    return pos, vel


KMAX = 4 * 2 * np.pi / 5.43 / np.sqrt(3.0)      # per component: |k| up to four Brillouin zones of silicon, 4.6 / A
OFFSET = 1200.0                                # Angstrom, added to every coordinate by the offset families


def k_list(K, seed, aligned=False):
    """(K, 3) float32 k-vectors with |component| <= KMAX; with K >= 2 the second is k = 0, with K >= 4 the fourth the
    exact negation of the third.  aligned: every component in [0.85, 1] KMAX, so that k.r of positions offset by OFFSET
    in every coordinate is 3 x 1200 x (2.3 .. 2.7) = 0.8e4 .. 1.0e4 rad (sum_c |k_c r_c| / 2 pi <= 1600 turns, inside the
    2^12 the kernel's bound is stated for)"""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.85, 1.0, (K, 3)) * KMAX if aligned else rng.uniform(-1.0, 1.0, (K, 3)) * KMAX
    k = k.astype(np.float32)
    if K >= 2:
        k[1] = 0.0
    if K >= 4:
        k[3] = -k[2]
    return k


def max_abs_phase(positions, k_vectors, idx=None):
    """largest |k.r| in radians over the frames, the atoms of the set and the k-vectors, in float64"""
    r = np.asarray(positions, np.float64)
    if idx is not None:
        r = r[:, np.asarray(idx, np.int64)]
    return float(np.max(np.abs(r.reshape(-1, 3) @ np.asarray(k_vectors, np.float64).reshape(-1, 3).T)))


def weights(kind, n_atoms, seed):
    """None (unit), sqrt of masses of two species, or signed scattering lengths"""
    rng = np.random.default_rng(seed)
    if kind == "unit":
        return None
    if kind == "sqrt_mass":
        return np.sqrt(np.where(rng.integers(0, 2, n_atoms) == 0, 28.0855, 72.63)).astype(np.float32)
    if kind == "signed":
        return np.where(rng.integers(0, 2, n_atoms) == 0, -3.739, 6.646).astype(np.float32)   # H, D coherent lengths, fm
    raise ValueError(kind)


# ---- a float32 model of the kernel's arithmetic ------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _fma(a, b, c):
    """float32 fma of float32 arrays: the product is exact in float64, the sum rounded once to float64 and then to
    float32 (a double rounding that does not matter to a model)"""
    return _f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def kappa_parts(k_vectors):
    """k / 2 pi in float64 from the float32 k, as float32 hi and lo"""
    kap = np.asarray(k_vectors, np.float32).astype(np.float64) / (2 * np.pi)
    hi = kap.astype(np.float32)
    return hi, (kap - hi.astype(np.float64)).astype(np.float32)


def turns_model(r, kh, kl):
    """the kernel's reduced phase in turns for atom positions r (..., 3) float32 and one k-vector's parts: float32"""
    p = [_f32(kh[c].astype(np.float64) * r[..., c].astype(np.float64)) for c in range(3)]
    e = [_f32(kh[c].astype(np.float64) * r[..., c].astype(np.float64) - p[c].astype(np.float64)) for c in range(3)]
    f = [p[c] - np.rint(p[c]) for c in range(3)]
    s = f[0] + f[1]
    s = s - np.rint(s)
    s = s + f[2]
    s = s - np.rint(s)
    lo = (e[0] + e[1]) + e[2]
    for c in range(3):
        lo = _fma(np.broadcast_to(kl[c], r[..., c].shape), r[..., c], lo)
    return (s + lo).astype(np.float32)


def radians_chain_model(r, k):
    """what the kernel must not do: k.r as a float32 FMA chain in radians"""
    th = _f32(k[0].astype(np.float64) * r[..., 0].astype(np.float64))
    th = _fma(np.broadcast_to(k[1], r[..., 1].shape), r[..., 1], th)
    return _fma(np.broadcast_to(k[2], r[..., 2].shape), r[..., 2], th)


def project_model(positions, velocities, k_vectors, idx=None, w=None, currents=True, radians_chain=False, call_K=None):
    """(K, NC, T) complex64 as the kernel's arithmetic gives it, the sine and cosine taken as exact float64 functions of
    the float32 argument rounded to float32: strands p mod 2 S, chains of DYN_CHAIN float32 FMAs folded into a second
    float32 sum, the strands added in float64 in ascending order and rounded once.  call_K: the number of k-vectors of
    the call these belong to (it sets the strands; None: these are the call)."""
    pos = np.asarray(positions, np.float32)
    T, N = pos.shape[:2]
    g = np.arange(N) if idx is None else np.asarray(idx, np.int64)
    k = np.asarray(k_vectors, np.float32).reshape(-1, 3)
    K, n_g, nc = k.shape[0], g.size, 4 if currents else 1
    ww = np.ones(N, np.float32) if w is None else np.asarray(w, np.float32)
    kh, kl = kappa_parts(k)
    G = 2 * slices(call_K or K)
    out = np.zeros((K, nc, T), np.complex64)
    for j in range(K):
        total = np.zeros((2 * nc, T), np.float64)
        for strand in range(min(G, n_g)):
            acc = np.zeros((2 * nc, T), np.float32)
            fold = np.zeros((2 * nc, T), np.float32)
            # (the kernel's chain counter runs over the steps of all tiles, padded ones included: a strand's n-th atom
            # is step n whatever the tile, since DYN_ATOMS is a multiple of 2 S)
            for n, p in enumerate(range(strand, n_g, G)):
                a = g[p]
                r = pos[:, a, :]
                if radians_chain:
                    th = radians_chain_model(r, k[j]).astype(np.float64)
                else:
                    th = 2 * np.pi * turns_model(r, kh[j], kl[j]).astype(np.float64)
                cs, sn = _f32(np.cos(th)), _f32(np.sin(th))
                d = [np.full(T, ww[a], np.float32)]
                if currents:
                    d += [_f32(ww[a].astype(np.float64) * np.asarray(velocities, np.float32)[:, a, c].astype(np.float64))
                          for c in range(3)]
                for c in range(nc):
                    acc[2 * c] = _fma(d[c], cs, acc[2 * c])
                    acc[2 * c + 1] = _fma(d[c], sn, acc[2 * c + 1])
                if (n + 1) % _hip.DYN_CHAIN == 0:
                    fold = fold + acc
                    acc[:] = 0
            total += (fold + acc).astype(np.float64)
        for c in range(nc):
            out[j, c] = (total[2 * c] + 1j * total[2 * c + 1]).astype(np.complex64)
    return out
