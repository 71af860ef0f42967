"""
Local order from the vectors q_lm: the neighbour-averaged q-bar_l of Lechner and Dellago (J. Chem. Phys. 129, 114707, 2008), the
third-order invariants w_l and w-bar_l of Steinhardt, Nelson and Ronchetti, and the solid-like bonds of ten Wolde, Ruiz-Montero
and Frenkel (J. Chem. Phys. 104, 9932, 1996) -- what is used after the (q_4, q_6) scatter of `psa_amd/order.py`.

With the neighbours of `psa_amd/order.py` (all species together, at most 64; n of them around the centre a, unit legs d_b)
and Yt_lm = sqrt(4 pi / (2 l + 1)) Y_lm, Condon-Shortley phase included:

    Q_lm(a) = sum_b round(Yt_lm(d_b) 2^40)  (64-bit integers, m = 0 .. l; Q_{l,-m} = (-1)^m conj Q_lm),  q_lm = Q_lm 2^-40 / n
    q-bar_lm(a) = (q_lm(a) + sum_{b in N(a)} q_lm(b)) / (n + 1),        q-bar_l^2 = sum_m |q-bar_lm|^2
    W_l(v) = sum_{m1+m2+m3=0} (l l l; m1 m2 m3) Re(v_m1 v_m2 v_m3),   w_l(v) = W_l(v) / (sum_m |v_m|^2)^(3/2)
    w = w_l(Q(a)),   w-bar = w_l(q-bar(a))
    a-b is a solid-like bond when D = Re sum_m Q_lm(a) conj Q_lm(b) > 0 and D^2 > thr^2 sum_m |Q_lm(a)|^2 sum_m |Q_lm(b)|^2
    xi(a) = the number of solid-like bonds of a, 0 .. 64

for even l only: for odd l the 3j symbol is antisymmetric under an exchange of two columns and W_l vanishes identically.
Known shells: (w_4, w_6) = (-0.159317, -0.013161) fcc, (+0.134097, -0.012442) hcp, (-0.159317, +0.013161) the eight of bcc,
(+0.159317, +0.013161) simple cubic; w_6 = -0.169754 for the icosahedron, whose q_4 vanishes.  w_l of a shell whose q_l is
nearly 0 is noise in any code: a quotient of two numbers that both are rounding residue (the icosahedron's w_4 is one).

    qbar_counts[alpha, j, i]   (a in alpha, origin) with q-bar_{ls[j]} in bin i of n_q uniform bins over [0, 1]
    w_counts, wbar_counts      the same for w and w-bar in n_w uniform bins over [-w_range, w_range]
    connections[alpha, i]      (a in alpha, origin) with exactly i solid-like bonds

Q is the same bits for any blocking, budget and atom order; the float64 sums run in the order of the neighbour list, so two
calls and any budget give the same bits, and a permutation of the atoms moves a value by the roundings of a reordered sum.  A
centre is left out of everything, all or nothing, when it has more than 64 neighbours (`truncated`; the calculator raises),
none (`isolated`), a coincident one (`undefined`), or a neighbour that is truncated or undefined (`incomplete`):

    sum_i qbar_counts[alpha, j, i] + truncated + isolated + undefined + incomplete = n_o N_alpha      for every j
    sum_i connections[alpha, i]    + the same four                                 = n_o N_alpha
    sum_i w_counts[alpha, j, i] + w_outside[alpha, j] + w_undefined[alpha, j] + the four = n_o N_alpha  (wbar alike)

  * Left out: odd l, the q_lm of other neighbour definitions, Voronoi or solid-angle weights, cell lists, sharding.  (The
    clusters of the solid-like atoms: `psa_amd/clusters.py`.)

This module is host code only: the 3j table, made in exact rational arithmetic, and the result type.
`SEDCalculator.calculate_local_order` runs the kernels (psa_amd/csrc/angle.hip's neighbour pass, psa_amd/csrc/qlm.hip).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache
from typing import List, Optional

import numpy as np

from ._hip import ANGLE_MAX_NEIGHBOURS, LOCAL_MAX_BINS, LOCAL_MAX_LS, LOCAL_SHIFT, ORDER_MAX_L  # noqa: F401
from .pairs import _divide


def _root(q: Fraction) -> float:
    """sqrt of a non-negative rational, rounded once: the integer root of the numerator scaled by 4^k over the denominator"""
    if q == 0:
        return 0.0
    shift = 128
    return math.isqrt((q.numerator << (2 * shift)) // q.denominator) / float(1 << shift)


@lru_cache(maxsize=None)
def wigner_3j_table(l: int) -> np.ndarray:
    """(2 l + 1, 2 l + 1) float64: the 3j symbols (l l l; m1 m2 -m1-m2) at [m1 + l, m2 + l], 0 where |m1 + m2| > l.  Racah's
    formula in Python integers and Fractions, the square root taken last (of an exact rational, rounded once)."""
    l = int(l)
    if l < 0:
        raise ValueError(f"l must not be negative, got {l}")
    f = math.factorial
    out = np.zeros((2 * l + 1, 2 * l + 1))
    delta = Fraction(f(l) ** 3, f(3 * l + 1))
    for m1 in range(-l, l + 1):
        for m2 in range(-l, l + 1):
            m3 = -m1 - m2
            if abs(m3) > l:
                continue
            total = Fraction(0)
            for k in range(max(0, -m1, m2), min(l, l - m1, l + m2) + 1):
                total += Fraction((-1) ** k, f(k) * f(l - k) * f(l - m1 - k) * f(l + m2 - k) * f(m1 + k) * f(k - m2))
            under = delta * f(l + m1) * f(l - m1) * f(l + m2) * f(l - m2) * f(l + m3) * f(l - m3)
            sign = (-1) ** ((m3) % 2) * (1 if total >= 0 else -1)                  # (-1)^(j1 - j2 - m3) = (-1)^m3
            out[m1 + l, m2 + l] = sign * _root(under * total * total)
    out.setflags(write=False)
    return out


def w3j_blocks(ls) -> np.ndarray:
    """the blocks of `wigner_3j_table` of the orders, flattened and concatenated: what `Engine.local_order` takes as `w3j`"""
    return np.concatenate([wigner_3j_table(int(l)).ravel() for l in ls]) if len(ls) else np.zeros(0)


@dataclass
class LocalOrder:
    """Result of `SEDCalculator.calculate_local_order`: `qbar_counts` (S, n_l, n_q), `w_counts`, `wbar_counts` (S, n_l, n_w),
    `connections` (S, 65) uint64; `ls` (n_l,) the orders; `q_edges`, `q` the bins of q-bar over [0, 1], `w_edges`, `w` those of
    w and w-bar over [-w_range, w_range]; `truncated`, `isolated`, `undefined`, `incomplete` (S,) and `w_outside`,
    `w_undefined`, `wbar_outside`, `wbar_undefined` (S, n_l) uint64 the (centre, origin) left out; `samples` (S,) = n_o N_alpha;
    `origins` = n_o; `groups` the atom-index arrays used; `solid_l`, `solid_threshold` of the bond test.  With `per_atom`:
    `qbar_atoms` (n_o, n_a, n_l) float64 (the root of qbar2), `w_atoms`, `wbar_atoms` the same shape, NaN where the centre is
    left out or the value undefined; `connections_atoms` (n_o, n_a) int32, -1 where left out; `neighbours` (n_o, n_a) the true
    neighbour counts; `atoms` (n_a,) the atom of every column; `mean` (S, n_l) the mean q-bar_l over the centres counted.
    Without: None."""
    qbar_counts: np.ndarray
    w_counts: np.ndarray
    wbar_counts: np.ndarray
    connections: np.ndarray
    ls: np.ndarray
    q_edges: np.ndarray
    q: np.ndarray
    w_edges: np.ndarray
    w: np.ndarray
    truncated: np.ndarray
    isolated: np.ndarray
    undefined: np.ndarray
    incomplete: np.ndarray
    w_outside: np.ndarray
    w_undefined: np.ndarray
    wbar_outside: np.ndarray
    wbar_undefined: np.ndarray
    samples: np.ndarray
    origins: int
    groups: List[np.ndarray]
    solid_l: int = 6
    solid_threshold: float = 0.7
    qbar_atoms: Optional[np.ndarray] = None
    w_atoms: Optional[np.ndarray] = None
    wbar_atoms: Optional[np.ndarray] = None
    connections_atoms: Optional[np.ndarray] = None
    neighbours: Optional[np.ndarray] = None
    atoms: Optional[np.ndarray] = None
    mean: Optional[np.ndarray] = None

    def order(self, l: int) -> int:
        """the column of order l in the counts, the per-atom arrays and `mean`"""
        at = np.flatnonzero(np.asarray(self.ls) == int(l))
        if at.size != 1:
            raise ValueError(f"order {l} is not among ls = {list(map(int, self.ls))}")
        return int(at[0])

    @property
    def density(self) -> np.ndarray:
        """qbar_counts normalised to integrate to 1 over q-bar, (S, n_l, n_q) float64; 0 where a species has no centre counted"""
        width = np.diff(np.asarray(self.q_edges, np.float64))[None, None, :]
        return _divide(self.qbar_counts, self.qbar_counts.sum(axis=-1, dtype=np.uint64)[:, :, None].astype(np.float64) * width)

    def solid_fraction(self, min_connections: int = 7) -> np.ndarray:
        """(S,) float64: the share of the centres counted that have at least `min_connections` solid-like bonds (the usual
        criterion of a solid-like particle); NaN for a species with no centre counted"""
        k = int(min_connections)
        if not 0 <= k <= ANGLE_MAX_NEIGHBOURS:
            raise ValueError(f"min_connections is in [0, {ANGLE_MAX_NEIGHBOURS}], got {min_connections!r}")
        total = self.connections.sum(axis=1, dtype=np.uint64).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(total > 0, self.connections[:, k:].sum(axis=1, dtype=np.uint64).astype(np.float64) / total, np.nan)


def row_words(n_l: int, n_q: int, n_w: int) -> int:
    return n_l * n_q + 2 * n_l * n_w + ANGLE_MAX_NEIGHBOURS + 1 + 4 + 4 * n_l


def split_row(hist, n_l: int, n_q: int, n_w: int) -> dict:
    """the parts of the (S, R) rows `Engine.local_order` returns, by name"""
    hist = np.asarray(hist)
    S = hist.shape[0]
    if hist.shape != (S, row_words(n_l, n_q, n_w)):
        raise ValueError(f"rows of {hist.shape} do not fit n_l = {n_l}, n_q = {n_q}, n_w = {n_w}")
    at, out = 0, {}
    for name, shape in (("qbar_counts", (n_l, n_q)), ("w_counts", (n_l, n_w)), ("wbar_counts", (n_l, n_w)),
                        ("connections", (ANGLE_MAX_NEIGHBOURS + 1,)), ("truncated", ()), ("isolated", ()), ("undefined", ()),
                        ("incomplete", ()), ("w_outside", (n_l,)), ("w_undefined", (n_l,)), ("wbar_outside", (n_l,)),
                        ("wbar_undefined", (n_l,))):
        size = int(np.prod(shape, dtype=np.int64))
        out[name] = hist[:, at:at + size].reshape((S,) + shape).copy()
        at += size
    return out


def result(hist, qbar2, w, wbar, xi, n, ls, n_q: int, n_w: int, w_range: float, solid_l: int, solid_threshold: float, origins: int,
           groups) -> LocalOrder:
    """the result type from what `Engine.local_order` returns"""
    ls = np.asarray(ls, np.int64).ravel().copy()
    parts = split_row(hist, ls.size, int(n_q), int(n_w))
    q_edges = np.linspace(0.0, 1.0, int(n_q) + 1)
    w_edges = np.linspace(-float(w_range), float(w_range), int(n_w) + 1)
    sizes = np.array([len(g) for g in groups], np.int64)
    res = LocalOrder(ls=ls, q_edges=q_edges, q=0.5 * (q_edges[1:] + q_edges[:-1]), w_edges=w_edges, w=0.5 * (w_edges[1:] + w_edges[:-1]),
                     samples=int(origins) * sizes, origins=int(origins), groups=list(groups), solid_l=int(solid_l),
                     solid_threshold=float(solid_threshold), **parts)
    if qbar2 is None:
        return res
    with np.errstate(invalid="ignore"):
        res.qbar_atoms = np.sqrt(np.asarray(qbar2, np.float64))
    res.w_atoms, res.wbar_atoms = np.asarray(w), np.asarray(wbar)
    res.connections_atoms, res.neighbours = np.asarray(xi), np.asarray(n)
    res.atoms = np.concatenate([np.asarray(g, np.int64) for g in groups]) if len(groups) else np.zeros(0, np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])
    res.mean = np.full((len(groups), ls.size), np.nan)
    for a in range(len(groups)):
        part = res.qbar_atoms[:, start[a]:start[a + 1]].reshape(-1, ls.size)
        kept = part[~np.isnan(part[:, 0])] if part.size else part
        if kept.size:
            res.mean[a] = kept.mean(axis=0)
    return res
