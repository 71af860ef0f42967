"""Input families of the self-spectra tests, the series kernel's per-element bound from reference quantities only, a NumPy
float32 model of the kernel's arithmetic (psa_amd/csrc/self.hip), and the host's tile rule restated.

The bound, per element of z (n_g, K, T) against tests/self64.series64:
    |z - z64| <= (eps_lat + C_MUL u) |w_a|                                  u = 2^-24
eps_lat is tests/lattice_cases.eps_lat (derived in the header of lattice.hip from the stated arithmetic of a term: three
table entries and two float32 complex products); C_MUL = 1 is the kernel header's count of the float32 multiplications
applied after those two products before the window: w_a E, one per component.  Nothing in it comes from the code under
test."""
import numpy as np

import lattice_cases as C
from lattice_cases import CUBIC, TRICLINIC, U, cmul_model, entry_model, frac_model, inverse, weights  # noqa: F401
from psa_amd import _hip

C_MUL = 1
A = _hip.SELF_ATOMS


def bound(w):
    """per-element bound for an atom of weight w (any shape)"""
    return (C.eps_lat() + C_MUL * U) * np.abs(np.asarray(w, np.float64))


# ---- input families -------------------------------------------------------------------------------------------
def _positions(s, box):
    return (np.asarray(s, np.float64) @ np.asarray(box, np.float32).astype(np.float64)).astype(np.float32)


def frozen(n_atoms, n_frames, seed, box=CUBIC):
    """(a) every frame equals frame 0: (T, N, 3) float32"""
    s0 = np.random.default_rng(seed).uniform(0.0, 1.0, (1, n_atoms, 3))
    return np.ascontiguousarray(np.broadcast_to(_positions(s0, box), (n_frames, n_atoms, 3)))


def ballistic(n_atoms, n_frames, seed, n0, box=CUBIC):
    """(b) s_a(t) = s_a(0) + sigma_a t folded into the box, as float32 positions; sigma_a = b_a n0 / (|n0|^2 T), so that
    n0.sigma_a T = b_a, an integer that differs per atom: atom a is a line in bin b_a mod T of column n0.  Returns
    (positions, b (N,) int)."""
    rng = np.random.default_rng(seed)
    n0 = np.asarray(n0, np.float64)
    b = rng.permutation(np.arange(-(n_frames // 2) + 1, n_frames // 2))[:n_atoms]
    assert b.size == n_atoms and np.unique(b % n_frames).size == n_atoms
    sigma = b[:, None] * n0[None, :] / (np.dot(n0, n0) * n_frames)
    s = rng.uniform(0.0, 1.0, (1, n_atoms, 3)) + sigma[None] * np.arange(n_frames)[:, None, None]
    return _positions(s - np.floor(s), box), b


def random_walk(n_atoms, n_frames, seed, box=CUBIC):
    """(c) steps of 0.05 box lengths per frame and axis.  Returns (wrapped, unwrapped, wrapped64, unwrapped64): float32
    positions folded into the box; the same frames moved back by whole box vectors -- formed in float64 from the float32
    wrapped positions and rounded to float32 --; and the float64 pair, which differs by whole box vectors exactly."""
    rng = np.random.default_rng(seed)
    H = np.asarray(box, np.float32).astype(np.float64)
    s = rng.uniform(0.0, 1.0, (1, n_atoms, 3)) + np.cumsum(0.05 * rng.standard_normal((n_frames, n_atoms, 3)), axis=0)
    turns = np.floor(s)
    wrapped = ((s - turns) @ H).astype(np.float32)
    wrapped64 = wrapped.astype(np.float64)
    unwrapped64 = wrapped64 + turns @ H
    assert np.abs(turns).max() >= 1                                        # some atom does cross the boundary
    return wrapped, unwrapped64.astype(np.float32), wrapped64, unwrapped64


def far(n_atoms, n_frames, seed, box=CUBIC):
    """(d) far from the origin: |k.r| ~ 1e4 rad at indices of +-LAT_MAX_INDEX"""
    return C.trajectory(n_atoms, n_frames, seed, box=box, shift=40)[0]


def grid_indices(K):
    """the first K <= 80 of the 4 x 4 x 5 vectors n_1, n_2 in 0..3, n_3 in 0..4 in the order of their indices: 13 distinct
    (axis, index) pairs, so SELF_KS alone cuts their tiles"""
    n = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    return n[:K].astype(np.int32)


# ---- the host's tile rule (api_self.hip), restated ------------------------------------------------------------------
def tiles(indices, bin_of=None):
    """sizes of the vector tiles of a call: the vectors sorted by (bin,) n_1, n_2, n_3, then cut greedily into tiles of
    at most SELF_KS vectors with at most SELF_ENTRIES distinct (axis, index) pairs"""
    n = np.asarray(indices).reshape(-1, 3)
    keys = (n[:, 2], n[:, 1], n[:, 0]) + (() if bin_of is None else (np.asarray(bin_of),))
    n = n[np.lexsort(keys)]
    sizes, used, count = [], [set(), set(), set()], 0
    for v in n:
        more = sum(int(v[j]) not in used[j] for j in range(3))
        if count == _hip.SELF_KS or sum(map(len, used)) + more > _hip.SELF_ENTRIES:
            sizes.append(count)
            used, count = [set(), set(), set()], 0
        for j in range(3):
            used[j].add(int(v[j]))
        count += 1
    return sizes + [count]


# ---- a float32 model of the series kernel's arithmetic ------------------------------------------------------------------
def series_model(positions, indices, inv, idx=None, w=None, single=False):
    """(n_g, K, T) complex64 as the kernel's arithmetic gives it: lat_frac, one entry per distinct (axis, m), two complex
    products, then w_a E per component.  single: the fractional coordinate rounded to one float32, as it must not be."""
    pos = np.asarray(positions, np.float32)
    N = pos.shape[1]
    g = np.arange(N) if idx is None else np.asarray(idx, np.int64)
    n = np.asarray(indices, np.int64).reshape(-1, 3)
    ww = np.ones(N, np.float32) if w is None else np.asarray(w, np.float32)
    hi, lo = C.box_parts(inv)
    out = np.zeros((g.size, n.shape[0], pos.shape[0]), np.complex64)
    for i, a in enumerate(g):
        s = [frac_model(pos[:, a, :], hi, lo, j) for j in range(3)]
        tables = [{int(m): entry_model(m, s[j][0], s[j][1], single) for m in np.unique(n[:, j])} for j in range(3)]
        for k in range(n.shape[0]):
            E = cmul_model(cmul_model(tables[0][int(n[k, 0])], tables[1][int(n[k, 1])]), tables[2][int(n[k, 2])])
            out[i, k] = (ww[a] * E[0]) + 1j * (ww[a] * E[1])
    return out
