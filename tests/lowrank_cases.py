"""Geometries of the low-rank k-path route's envelope, shared by the plan's CPU tests (tests/test_lowrank_plan.py) and
the GPU tests (tests/test_gpu_lowrank_envelope.py).  Everything is built from seeds: random positions in a box, a
k-path through Gamma along a lattice direction, optionally pushed off the line."""
import numpy as np

D_LIMIT = (2.0 ** -14, 2.0 ** -13)      # "D at its limit": the plan's d_bound in this range (2^-13: acceptance)


def box(n, edge, seed, shift=0.0):
    """n random positions in a cube of the given edge whose corner is at (shift, shift, shift), float32"""
    return (np.random.default_rng(seed).random((n, 3)) * edge + shift).astype(np.float32)


def path(direction, k_lo, k_hi, K):
    """K float32 k-vectors from k_lo to k_hi along a direction (|k| in 1/Angstrom; the list runs away from Gamma)"""
    u = np.asarray(direction, np.float64)
    u = u / np.linalg.norm(u)
    return (np.linspace(k_lo, k_hi, K)[:, None] * u[None, :]).astype(np.float32)


def scattered(k, sigma, seed):
    """k with a random perpendicular scatter of sigma per component (the [100] paths below: y and z)"""
    k = k.astype(np.float64)
    k[:, 1:] += np.random.default_rng(seed).standard_normal((len(k), 2)) * sigma
    return k.astype(np.float32)


def mass_weights(n, seed):
    """mass-like per-atom weights (H, C, Si, U: about 1 to 240)"""
    return np.random.default_rng(seed).choice(np.float32([1.008, 12.011, 28.086, 238.03]), n).astype(np.float32)


N_ATOMS = 2048

# name: (k-vectors, expected interval); limit_* are "D at its limit": d_bound in D_LIMIT
def k_vectors(name, K=300):
    if name == "dir_1-10":
        return path([1, -1, 0], 0.0, 1.5, K), 0
    if name == "dir_111":
        return path([1, 1, 1], 0.0, 1.5, K), 0
    if name == "dir_210":
        return path([2, 1, 0], 0.0, 1.5, K), 0
    if name == "neg_-1-10":                  # the canonical sign flips u: the list lies on the side kappa <= 0
        return path([-1, -1, 0], 0.0, 1.5, K), -1
    if name == "neg_00-1":
        return path([0, 0, -1], 0.0, 1.5, K), -1
    if name == "seg_1":                      # a segment inside [w, 2w), w = 60 / 40 * 2 = 3.0 for the centred box
        return path([1, 0, 0], 3.2, 5.5, K), 1
    if name == "seg_-2":                     # its mirror image
        return path([-1, 0, 0], 3.2, 5.5, K), -2
    if name == "plain_100":
        return path([1, 0, 0], 0.0, 1.5, K), 0
    if name == "limit_shift":                # with its box 110 A from the origin: phases up to ~450 rad, 3 roundings
        return path([1, 1, 1], 0.0, 2.0, K), 0
    if name == "limit_offline":              # 1e-6 of perpendicular scatter: D carries a real off-line phase
        return scattered(path([1, 0, 0], 0.0, 1.5, K), 1e-6, 2), 0
    raise KeyError(name)


# name: (k-vectors, positions, expected interval); the box is 40 A centred on the origin, but limit_shift's: 20 A, 110 A
# from the origin
def geometry(name, K=300):
    k, interval = k_vectors(name, K)
    r = box(N_ATOMS, 20.0, 1, 110.0) if name == "limit_shift" else box(N_ATOMS, 40.0, 1, -20.0)
    return k, r, interval


DIRECTIONS = ["dir_1-10", "dir_111", "dir_210", "neg_-1-10", "neg_00-1", "seg_1", "seg_-2"]
LIMITS = ["limit_shift", "limit_offline"]
