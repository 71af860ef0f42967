"""Input families of the pair-distribution tests, the allowance of the histogram derived from the arithmetic stated at the
head of psa_amd/csrc/pair.hip and from nothing in the code, and a NumPy twin of that arithmetic with the planted faults
the host test holds outside the allowance.

The allowance, u = 2^-24.  c = float32(sigma - floor(sigma) - 0.5) is rounded below 0.5: 2^-26 each; e = c(b) - c(a) is one
float32 subtraction of a value below 1: 2^-25; e - rint(e) is exact.  So |delta e_j| <= 2^-24, plus what the float64
sigma carries, E64 = 8 2^-53 max_j sum_c |r_c| |Hinv_cj| (three roundings of the chain and the subtractions, of the
route and of the reference both; far below 2^-24 unless |r| is 10^7 boxes).
    |delta d_c| <= sum_j (|delta e_j| + 3 u |e_j|) |H_jc|            (e's error through h, and three roundings of the chain;
                                                                       h = float32(H) is exact for the float32 boxes used)
    tol = (|delta d|_2 + 4.5 u |d| + extra) / dr (1 + 2^-20)         (the sum's three roundings halve under the root: 1.5 u;
                                                                       the root, inv_dr and the product one each)
`extra` is for comparisons across two inputs that differ by the float32 rounding of their positions.  A reference sample
is borderline when x = |d| / dr lies within tol of an integer k in [1, n_r]; a bin may differ from the reference by the
borderline samples at its two edges, the totals by nothing.  This is `histogram_allowance` of msd_cases.py for pairs."""
import numpy as np

import pair64 as R
from lattice_cases import CUBIC, TRICLINIC  # noqa: F401
from psa_amd import _hip

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TILE = _hip.PAIR_TILE
BORDERLINE_CAP = {False: 1e-3, True: 2e-3}                                 # n_r <= 256; n_r = 1024


def cap(n_r):
    assert n_r <= 256 or n_r == 1024
    return BORDERLINE_CAP[n_r == 1024]


# ---- input families -----------------------------------------------------------------------------------------------
def walk(n_atoms, n_frames, seed, box=CUBIC, step=0.05):
    """a random walk of `step` box lengths per frame and axis from uniform starts.  dict of float32 positions (T, N, 3):
    "wrapped" folded into the box; "unwrapped" the same frames moved back by whole box vectors (formed in float64 from
    the float32 wrapped positions, rounded to float32); "moved" each atom moved by up to +-3 whole box vectors of its own;
    "shifted" each atom moved by up to +-1000 box vectors of its own"""
    rng = np.random.default_rng(seed)
    H = np.asarray(box, np.float32).astype(np.float64)
    s = rng.uniform(0.0, 1.0, (1, n_atoms, 3)) + np.cumsum(step * rng.standard_normal((n_frames, n_atoms, 3)), axis=0)
    turns = np.floor(s)
    wrapped = ((s - turns) @ H).astype(np.float32)
    w64 = wrapped.astype(np.float64)
    out = {"wrapped": wrapped, "unwrapped": (w64 + turns @ H).astype(np.float32)}
    for name, reach in (("moved", 3), ("shifted", 1000)):
        n = rng.integers(-reach, reach + 1, (1, n_atoms, 3)).astype(np.float64)
        out[name] = (w64 + n @ H).astype(np.float32)
    return out


def frozen(n_atoms, n_frames, seed, box=CUBIC):
    s0 = np.random.default_rng(seed).uniform(0.0, 1.0, (1, n_atoms, 3))
    H = np.asarray(box, np.float32).astype(np.float64)
    return np.ascontiguousarray(np.broadcast_to((s0 @ H).astype(np.float32), (n_frames, n_atoms, 3)))


LATTICE_BOXES = {
    "cubic": CUBIC,
    # the same cubic lattice in a sheared cell: the second box vector leans by one lattice constant along x
    "sheared": np.array([[21.72, 0.0, 0.0], [21.72 / 4, 21.72, 0.0], [0.0, 0.0, 21.72]], np.float32),
}


def simple_cubic(n_frames, box_name):
    """64 atoms on a 4 x 4 x 4 simple-cubic lattice of constant a = 21.72 / 4, frozen: (positions, a).  Both boxes of
    LATTICE_BOXES are periods of that lattice; in the sheared one half of the atoms lie outside the cell as stored"""
    a = float(np.float32(21.72)) / 4.0
    site = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3) * a
    return np.ascontiguousarray(np.broadcast_to(site.astype(np.float32), (n_frames, 64, 3))), a


# ---- the allowance ----------------------------------------------------------------------------------------------------
def sigma_error(positions, box):
    """E64: what the float64 fractional coordinates of the route and of the reference carry together"""
    r = np.abs(np.asarray(positions, np.float64)).reshape(-1, 3).max(axis=0)
    return 8.0 * U64 * float((r @ np.abs(R.box64(box)[1])).max())


def tolerance(e, d, r, box, dr, e64=0.0, extra=0.0):
    """per sample: what x = r / dr may carry"""
    aH = np.abs(R.box64(box)[0])
    dd = (U32 + e64 + 3.0 * U32 * np.abs(e)) @ aH
    return (np.sqrt((dd * dd).sum(axis=1)) + 4.5 * U32 * r + extra) / dr * (1.0 + 2.0 ** -20)


def allowance_of(e, d, r, box, dr, n_r, e64=0.0, extra=0.0):
    """(allowed (n_r + 1,) int64, borderline samples) of one set of reference samples"""
    x = r / dr
    k = np.rint(x).astype(np.int64)
    near = (np.abs(x - k) <= tolerance(e, d, r, box, dr, e64, extra)) & (k >= 1) & (k <= n_r)
    edge = np.bincount(k[near], minlength=n_r + 2)[:n_r + 2]
    allowed = np.zeros(n_r + 1, np.int64)
    allowed[:n_r] = edge[:n_r] + edge[1:n_r + 1]
    allowed[n_r] = edge[n_r]
    return allowed, int(near.sum())


def reference(positions, box, groups, lags, step, dr, n_r, extra=0.0):
    """(counts (n_vh, S, S, n_r + 1) int64 of tests/pair64.py, allowed (the same shape), borderline samples, all samples)
    from one pass of the brute force"""
    S = len(groups)
    ref = np.zeros((len(lags), S, S, n_r + 1), np.int64)
    allowed = np.zeros_like(ref)
    e64 = sigma_error(positions, box)
    borderline = total = 0
    for j, lag in enumerate(lags):
        for a in range(S):
            for b in range(S):
                if len(groups[a]) == 0 or len(groups[b]) == 0:
                    continue
                e, d, r = R.pair_samples(positions, box, groups[a], groups[b], int(lag), step)
                ref[j, a, b] = R.bins(r, dr, n_r)
                allowed[j, a, b], near = allowance_of(e, d, r, box, dr, n_r, e64, extra)
                borderline += near
                total += r.size
    return ref, allowed, borderline, total


def expected_totals(n_frames, groups, lags, step):
    """(n_vh, S, S): n_o N_a (N_b - delta_ab)"""
    n = np.array([len(g) for g in groups], np.int64)
    n_o = np.array([R.n_origins(n_frames, int(t), step) for t in lags], np.int64)
    return n_o[:, None, None] * n[None, :, None] * (n[None, None, :] - np.eye(n.size, dtype=np.int64)[None])


# ---- a NumPy twin of the stated arithmetic, with the planted faults ---------------------------------------------------
FAULTS = ("no_image", "frac32", "orthogonal_only", "same_frame", "self_included", "diagonal_doubled", "bin_shift")


def _fma32(a, b, c):
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def fractions_model(positions, box, fault=None):
    """c (T, N, 3) float32 as pair.hip states it.  Fault "frac32": sigma formed in float32"""
    r32 = np.asarray(positions, np.float32)
    inv = R.box64(box)[1]
    if fault == "frac32":
        i32 = inv.astype(np.float32)
        s = _fma32(r32[..., 2:3], i32[2], _fma32(r32[..., 1:2], i32[1], r32[..., 0:1] * i32[0]))
        return (s - np.floor(s) - np.float32(0.5)).astype(np.float32)
    r = r32.astype(np.float64)
    s = r[..., 2:3] * inv[2] + (r[..., 1:2] * inv[1] + r[..., 0:1] * inv[0])
    return (s - np.floor(s) - 0.5).astype(np.float32)


def histogram_model(positions, box, groups, lags, step, dr, n_r, fault=None):
    """(n_vh, S, S, n_r + 1) int64 as the pair kernel's arithmetic gives them.  Faults: FAULTS"""
    c = fractions_model(positions, box, fault)
    h = R.box64(box)[0].astype(np.float32)
    if fault == "orthogonal_only":
        h = np.diag(np.diag(h))
    inv_dr, edge = np.float32(1.0 / dr), np.float32(n_r)
    S, T = len(groups), c.shape[0]
    out = np.zeros((len(lags), S, S, n_r + 1), np.int64)
    for j, lag in enumerate(lags):
        lag = int(lag)
        o = R.origins(T, lag, step)
        for a in range(S):
            for b in range(S):
                ia, ib = np.asarray(groups[a], np.int64), np.asarray(groups[b], np.int64)
                if ia.size == 0 or ib.size == 0:
                    continue
                cb = c[o if fault == "same_frame" else o + lag][:, None, ib, :]
                e = (cb - c[o][:, ia, None, :]).astype(np.float32)                      # (n_o, N_a, N_b, 3)
                if fault != "no_image":
                    e = e - np.rint(e)
                d = [_fma32(e[..., 2], h[2, k], _fma32(e[..., 1], h[1, k], e[..., 0] * h[0, k])) for k in range(3)]
                r2 = _fma32(d[2], d[2], _fma32(d[1], d[1], d[0] * d[0]))
                x = np.sqrt(r2) * inv_dr
                bin_ = np.floor(x).astype(np.int64) + (1 if fault == "bin_shift" else 0)
                bin_ = np.where(x < edge, bin_, n_r).clip(max=n_r)
                keep = np.broadcast_to((ia[:, None] != ib[None, :])[None], bin_.shape)
                if fault == "self_included":
                    keep = np.ones_like(keep)
                out[j, a, b] = np.bincount(bin_[keep], minlength=n_r + 1)
                if fault == "diagonal_doubled" and lag == 0 and a == b:
                    # the diagonal tile of the triangle counted like an off-diagonal one: every (a, b) of the tile, the
                    # pairs a >= b and a = b among them, evaluated and doubled, where a < b alone should be
                    pa = np.arange(ia.size) // TILE
                    tile = np.broadcast_to((pa[:, None] == pa[None, :])[None], bin_.shape)
                    out[j, a, b] += np.bincount(bin_[tile], minlength=n_r + 1)
    return out
