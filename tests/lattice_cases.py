"""Input families of the lattice-spectra tests, the projection kernel's per-element bound from reference quantities only,
and a NumPy float32 model of the kernel's arithmetic (psa_amd/csrc/lattice.hip) -- with the fractional coordinates
carried as two float32, as the kernel carries them, or rounded to one, as it must not.

The bound, per element of q (K, NC, T) against tests/lattice64.project64:
    |q - q64| <= (eps_lat + (LAT_CHAIN + folds(N_g) + 4) u) sum_a |w_a| |d_a,c(t)|          u = 2^-24
    eps_lat = 3 (2 pi u + sqrt(2) DYN_SINCOS_ERR) + 6 u,   folds(N_g) = ceil(N_g / LAT_CHAIN)
Nothing in it comes from the code under test: u is the float32 unit roundoff; LAT_CHAIN and the single strand are the
kernel's stated summation order; eps_lat is derived in the kernel's header from its stated arithmetic -- three table
entries, each with an argument within 1.0 u turns and the hardware sine and cosine (DYN_SINCOS_ERR: twice their error
measured against float64), and two float32 complex products --; sum |w| |d| is computed in float64 from the inputs."""
import math

import numpy as np

from dynamic_cases import EPS_TERM_CAP, U, weights  # noqa: F401  (the cap and the weight families are the project's)
from psa_amd import _hip

CUBIC = np.diag([21.72] * 3).astype(np.float32)                       # 4 cells of silicon, Angstrom
TRICLINIC = np.array([[21.72, 0.0, 0.0], [2.1, 20.5, 0.0], [-1.3, 3.2, 23.9]], np.float32)
M = _hip.LAT_MAX_INDEX


def inverse(box):
    """the 9 float64 numbers both the library and the reference use"""
    return np.linalg.inv(np.asarray(box, np.float32).astype(np.float64))


def folds(n_g):
    return math.ceil(n_g / _hip.LAT_CHAIN)


def eps_lat():
    return 3 * (2 * math.pi * U + math.sqrt(2.0) * _hip.DYN_SINCOS_ERR) + 6 * U


def bound(absum, n_g):
    """per-element bound for sum_a |w_a| |d_a,c(t)| = absum (any shape)"""
    return (eps_lat() + (_hip.LAT_CHAIN + folds(n_g) + 4) * U) * np.asarray(absum, np.float64)


# ---- input families -------------------------------------------------------------------------------------------
def trajectory(n_atoms, n_frames, seed, box=CUBIC, shift=0):
    """(positions, velocities) (T, N, 3) float32: sites scattered over the box, each atom wandering about its site by
    0.1 A per frame, velocities of order 5 A/ps; shift: every atom is moved by up to +-shift whole box vectors along every
    axis (an unwrapped trajectory: shift = 40 puts |k.r| at 1e4 rad for indices of +-LAT_MAX_INDEX)"""
    rng = np.random.default_rng(seed)
    H = np.asarray(box, np.float32).astype(np.float64)
    frac = rng.uniform(0.0, 1.0, (1, n_atoms, 3))
    if shift:
        frac = frac + rng.integers(-shift, shift + 1, (1, n_atoms, 3))
        frac[0, 0] = [shift + 0.37, -shift - 0.41, shift + 0.73]           # one atom at the far corner, whatever the draw
    pos = (frac @ H + 0.1 * rng.standard_normal((n_frames, n_atoms, 3))).astype(np.float32)
    vel = (5.0 * rng.standard_normal((n_frames, n_atoms, 3))).astype(np.float32)
    return pos, vel


def corner_indices():
    """the eight sign patterns of (M, M, M), M = LAT_MAX_INDEX"""
    return np.array([[sx * M, sy * M, sz * M] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.int32)


def mixed_indices(K, seed):
    """(K, 3) int32 indices up to +-12 per axis; with K >= 2 the second is n = 0, with K >= 4 the fourth the negation of
    the third"""
    n = np.random.default_rng(seed).integers(-12, 13, (K, 3)).astype(np.int32)
    if K >= 2:
        n[1] = 0
    if K >= 4:
        n[3] = -n[2]
    return n


def max_abs_phase(positions, indices, inv, idx=None):
    """largest |k.r| = 2 pi |n.s| in radians over the frames, the atoms of the set and the vectors, in float64"""
    r = np.asarray(positions, np.float64)
    if idx is not None:
        r = r[:, np.asarray(idx, np.int64)]
    s = r.reshape(-1, 3) @ np.asarray(inv, np.float64)
    return float(2 * np.pi * np.max(np.abs(s @ np.asarray(indices, np.float64).reshape(-1, 3).T)))


def travelling_wave(n_atoms, n_frames, box, k0_index, bin0, amp=1.5, seed=0, e_hat=(0.6, 0.0, 0.8)):
    """(positions, velocities) (T, N, 3) float32 of sites scattered over the box and displaced by
    u = A e cos(w0 t - k0.R), k0 = n0.G commensurate, w0 on bin `bin0` of `n_frames` frames: a wave travelling along +k0,
    whose line sits at +w0 for k0 and at -w0 for -k0 -- so the frequency mirror of a folded pair matters"""
    rng = np.random.default_rng(seed)
    H = np.asarray(box, np.float32).astype(np.float64)
    R = rng.uniform(0.0, 1.0, (n_atoms, 3)) @ H
    k0 = 2 * np.pi * (np.asarray(k0_index, np.float64) @ inverse(box).T)
    w0 = 2 * np.pi * bin0 / n_frames
    e = np.asarray(e_hat, np.float64)
    ph = w0 * np.arange(n_frames)[:, None] - (R @ k0)[None, :]
    pos = R[None] + amp * np.cos(ph)[..., None] * e + 0.02 * rng.standard_normal((n_frames, n_atoms, 3))
    vel = -amp * w0 * np.sin(ph)[..., None] * e
    return pos.astype(np.float32), vel.astype(np.float32)


# ---- a float32 model of the kernel's arithmetic ------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _fma(a, b, c):
    """float32 fma of float32 arrays: the product is exact in float64, the sum rounded to float64 and then to float32"""
    return _f32(np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
                + np.asarray(c, np.float32).astype(np.float64))


def box_parts(inv):
    """Hinv as float32 hi and lo, (3, 3) each"""
    inv = np.asarray(inv, np.float64)
    hi = inv.astype(np.float32)
    return hi, (inv - hi.astype(np.float64)).astype(np.float32)


def frac_model(r, hi, lo, j):
    """(s_hi, s_lo) float32 of axis j for positions r (..., 3) float32, as lat_frac forms them"""
    x = [np.asarray(r[..., c], np.float32) for c in range(3)]
    h = [np.float32(hi[c, j]) for c in range(3)]
    p = [h[c] * x[c] for c in range(3)]
    e = [_fma(np.broadcast_to(h[c], x[c].shape), x[c], -p[c]) for c in range(3)]
    f = [p[c] - np.rint(p[c]) for c in range(3)]
    t = f[0] + f[1]
    bb = t - f[0]
    err1 = (f[0] - (t - bb)) + (f[1] - bb)
    t = t - np.rint(t)
    t2 = t + f[2]
    bb = t2 - t
    err2 = (t - (t2 - bb)) + (f[2] - bb)
    s_hi = t2 - np.rint(t2)
    s_lo = (e[0] + e[1]) + e[2]
    for c in range(3):
        s_lo = _fma(np.broadcast_to(np.float32(lo[c, j]), x[c].shape), x[c], s_lo)
    return s_hi.astype(np.float32), (s_lo + (err1 + err2)).astype(np.float32)


def entry_model(m, s_hi, s_lo, single=False):
    """(cos, sin) float32 of 2 pi m s as lat_entry forms them, the sine and cosine taken as exact float64 functions of
    the float32 argument rounded to float32; single: s rounded to one float32 first"""
    m = np.float32(m)
    if single:
        s_hi, s_lo = (s_hi + s_lo).astype(np.float32), np.zeros_like(s_lo)
    p = m * s_hi
    e = _fma(np.broadcast_to(m, s_hi.shape), s_hi, -p)
    g = p - np.rint(p)
    turns = (g + _fma(np.broadcast_to(m, s_lo.shape), s_lo, e)).astype(np.float64)
    return _f32(np.cos(2 * np.pi * turns)), _f32(np.sin(2 * np.pi * turns))


def cmul_model(a, b):
    """lat_cmul: (a.x b.x - fl(a.y b.y), a.x b.y + fl(a.y b.x)) with one fma each"""
    return _fma(a[0], b[0], -(a[1] * b[1])), _fma(a[0], b[1], a[1] * b[0])


def project_model(positions, velocities, indices, inv, idx=None, w=None, currents=True, single=False, with_term_error=False):
    """(K, NC, T) complex64 as the kernel's arithmetic gives it: per atom the entries of the indices in use, two complex
    products per vector, chains of LAT_CHAIN float32 FMAs folded into a second float32 sum, and the last fold.
    with_term_error: also the largest |E_1 E_2 E_3 - exp(2 pi i n.s)| over all units, against float64."""
    pos = np.asarray(positions, np.float32)
    T, N = pos.shape[:2]
    g = np.arange(N) if idx is None else np.asarray(idx, np.int64)
    n = np.asarray(indices, np.int64).reshape(-1, 3)
    K, nc = n.shape[0], 4 if currents else 1
    ww = np.ones(N, np.float32) if w is None else np.asarray(w, np.float32)
    hi, lo = box_parts(inv)
    acc = np.zeros((K, 2 * nc, T), np.float32)
    fold = np.zeros((K, 2 * nc, T), np.float32)
    worst = 0.0
    for count, a in enumerate(g):
        r = pos[:, a, :]
        s = [frac_model(r, hi, lo, j) for j in range(3)]
        d = [np.full(T, ww[a], np.float32)]
        if currents:
            d += [ww[a] * np.asarray(velocities, np.float32)[:, a, c] for c in range(3)]
        tables = [{int(m): entry_model(m, s[j][0], s[j][1], single) for m in np.unique(n[:, j])} for j in range(3)]
        s64 = r.astype(np.float64) @ np.asarray(inv, np.float64)
        for k in range(K):
            E = cmul_model(cmul_model(tables[0][int(n[k, 0])], tables[1][int(n[k, 1])]), tables[2][int(n[k, 2])])
            if with_term_error:
                ref = np.exp(2j * np.pi * ((s64 - np.rint(s64)) @ n[k].astype(np.float64)))
                worst = max(worst, float(np.max(np.abs((E[0].astype(np.float64) + 1j * E[1].astype(np.float64)) - ref))))
            for c in range(nc):
                acc[k, 2 * c] = _fma(d[c], E[0], acc[k, 2 * c])
                acc[k, 2 * c + 1] = _fma(d[c], E[1], acc[k, 2 * c + 1])
        if (count + 1) % _hip.LAT_CHAIN == 0:
            fold = fold + acc
            acc[:] = 0
    tot = fold + acc
    out = (tot[:, 0::2] + 1j * tot[:, 1::2]).astype(np.complex64)
    return (out, worst) if with_term_error else out
