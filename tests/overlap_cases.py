"""Input families of the self-overlap tests, the allowance of a count from reference quantities only, and a NumPy twin of
the stated arithmetic (psa_amd/csrc/overlap.hip) with the planted faults the host test holds outside the allowance.
Nothing in the allowance comes from the code under test.

Allowance.  The sample is the van Hove sample of tests/msd_cases.py with one bin of width a, so its error model applies
unchanged: x = |D| / a carries at most tol = (|e|_2 + 4.5 u32 |D|) / a (1 + 2^-20), e from msd_cases._sample_errors; a
reference sample is borderline when x64 lies within tol of the edge k = 1.  Q[j,g,k] may differ from the reference by the
number of borderline samples among the atoms of g at that lag and origin; S1 by their sum over the origins; S2 by
sum_k (2 Q al + al^2).

Lattice family.  Positions on a lattice of spacing 0.25, steps of -0.25, 0 or 0.25 per frame and axis, UNWRAPPED, far
inside float32's exact range: u, a_c, b_c and D_c are exact multiples of 0.25 below 2^7, r2 an exact multiple of 1/16,
sqrt(1/4) = 1/2 exactly and correctly rounded roots are monotone.  At a = 0.5 (inv_a = 2 exactly) x < 1 iff r2 < 1/4
with no rounding anywhere: the allowance is zero by construction, and |D| = 0.5 exactly is not counted.  At a = 0.6 the
nearest lattice distances are sqrt(5)/4 = 0.559 (x = 0.93) and sqrt(6)/4 = 0.612 (x = 1.02): no borderline sample."""
import numpy as np

import msd64 as R
import msd_cases as M
from psa_amd import _hip

CUBIC, TRICLINIC = M.CUBIC, M.TRICLINIC


# ---- input families -----------------------------------------------------------------------------------------------------
def lattice_walk(n_atoms, n_frames, seed, cooperative=False):
    """UNWRAPPED float32 positions on the lattice of spacing 0.25 inside the cubic box at frame 0, every later frame moved
    by -0.25, 0 or 0.25 per axis; `cooperative`: all atoms share one walk.  Every value is exact in float32."""
    rng = np.random.default_rng(seed)
    start = 0.25 * rng.integers(0, 80, (1, n_atoms, 3))
    steps = 0.25 * rng.integers(-1, 2, (n_frames, 1 if cooperative else n_atoms, 3))
    steps[0] = 0.0
    pos = start + np.cumsum(steps, axis=0)
    out = np.ascontiguousarray(np.broadcast_to(pos, (n_frames, n_atoms, 3)).astype(np.float32))
    assert np.array_equal(out.astype(np.float64), np.broadcast_to(pos, out.shape)) and np.abs(out).max() < 2.0 ** 10
    return out


# ---- the allowance ------------------------------------------------------------------------------------------------------
def allowance(u, S, groups, lags, step, cutoff):
    """(allowed (n_lags, G, n_o_max) int64; borderline samples; all samples): per (lag, group, origin) the number of
    reference samples borderline at the edge k = 1 under msd_cases._sample_errors with dr = cutoff"""
    E, eu = M.excursion(u), M.unwrap_bound(S).max(axis=0)
    lags = [int(t) for t in lags]
    allowed = np.zeros((len(lags), len(groups), R.n_origins(u.shape[0], min(lags), step)), np.int64)
    borderline = total = 0
    for j, lag in enumerate(lags):
        for g, atoms in enumerate(groups):
            a = np.asarray(atoms, np.int64)
            if a.size == 0:
                continue
            D = R.displacements(u, a, lag, step)
            e, _, _ = M._sample_errors(D, E[a][None], eu[a][None])
            r = np.sqrt((D * D).sum(axis=2))
            tol = (np.sqrt((e * e).sum(axis=2)) + 4.5 * M.U32 * r) / cutoff * (1.0 + 2.0 ** -20)
            near = np.abs(r / cutoff - 1.0) <= tol
            allowed[j, g, :near.shape[0]] = near.sum(axis=1)
            borderline += int(near.sum())
            total += near.size
    return allowed, borderline, total


def sums_allowance(Q, allowed):
    """what S1 and S2 may differ from the reference's by, from the reference's Q and the counts' allowance"""
    return allowed.sum(axis=2), (2 * Q * allowed + allowed * allowed).sum(axis=2)


def inside(got, ref, allowed):
    return bool(np.all(np.abs(np.asarray(got, np.int64) - ref) <= allowed))


# ---- a NumPy twin of the stated arithmetic, with the planted faults -----------------------------------------------------
FAULTS = ("le", "o0_neighbour", "u32", "s2_of_mean", "groups_merged", "lag_shift", "origins_of_lag_0")


def _r2(u, atoms, lag, step, fault):
    """r2 (n_o, n_a) float32 of one lag as the count kernel forms it (msd_cases._units); "o0_neighbour": a and b taken from
    the first origin of the next origin tile"""
    if fault != "o0_neighbour":
        return M._units(u, atoms, lag, step, "u32" if fault == "u32" else None)[1]
    NO = min(_hip.MSD_ORIGINS, (M.W - _hip.MSD_LAGS) // step + 1)
    o = R.origins(u.shape[0], lag, step)
    o0 = np.minimum((np.arange(o.size) // NO + 1) * NO * step, ((u.shape[0] - 1) // step) * step)
    a = np.asarray(atoms, np.int64)
    base = u[o0][:, a]
    D = (u[o + lag][:, a] - base).astype(np.float32) - (u[o][:, a] - base).astype(np.float32)
    return M._fma32(D[..., 2], D[..., 2], M._fma32(D[..., 1], D[..., 1], D[..., 0] * D[..., 0]))


def overlap_model(u, groups, lags, step, cutoff, fault=None):
    """(Q (n_lags, G, n_o_max) int64, S1, S2 (n_lags, G) int64) as the kernels' arithmetic gives them.  Faults: "le" (<= for
    <), "o0_neighbour", "u32" (u kept as float32 from frame 0), "s2_of_mean" (S2 = S1^2 / n_o), "groups_merged" (every
    group counts all listed atoms), "lag_shift" (row j holds the lag of row j + 1), "origins_of_lag_0" (n_o(0) origins at
    every lag, the later frame held at T - 1)"""
    assert fault is None or fault in FAULTS, fault
    inv_a = np.float32(1.0 / cutoff)
    lags = [int(t) for t in lags]
    T = u.shape[0]
    if fault == "lag_shift":
        lags = lags[1:] + lags[:1]
    n_o_max = R.n_origins(T, 0 if fault == "origins_of_lag_0" else min(lags), step)
    Q = np.zeros((len(lags), len(groups), n_o_max), np.int64)
    merged = np.concatenate([np.asarray(g, np.int64) for g in groups]) if groups else np.zeros(0, np.int64)
    for j, lag in enumerate(lags):
        for g, atoms in enumerate(groups):
            atoms = merged if fault == "groups_merged" else np.asarray(atoms, np.int64)
            if atoms.size == 0:
                continue
            if fault == "origins_of_lag_0":
                held = np.concatenate([u, np.broadcast_to(u[-1:], (lag,) + u.shape[1:])]) if lag else u
                r2 = M._units(held, atoms, lag, step)[1][:n_o_max]
            else:
                r2 = _r2(u, atoms, lag, step, fault)
            x = np.sqrt(r2) * inv_a
            assert x.dtype == np.float32
            ov = x <= np.float32(1.0) if fault == "le" else x < np.float32(1.0)
            Q[j, g, :ov.shape[0]] = ov.sum(axis=1)
    S1, S2 = Q.sum(axis=2), (Q * Q).sum(axis=2)
    if fault == "s2_of_mean":
        n_o = np.array([R.n_origins(T, t, step) for t in lags], np.int64)[:, None]
        S2 = S1 * S1 // n_o
    return Q, S1, S2
