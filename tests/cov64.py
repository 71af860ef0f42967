"""A float64 restatement of the spectral covariance (psa_amd/covariance.py, psa_sed_covariance), the bound its kernel is
held to, and the inputs and float32 models of the bound's tests (tests/test_gpu_covariance.py, tests/test_cov_host.py).

    S_i[k,w]     = the spectra of tests/modes64.py (spectra64), row i = 3 b + c
    G[m,k,i,j]   = scale sum_w g[m,w] S_i[k,w] conj(S_j[k,w])                                       cov64
    A[m,k,i,j]   = scale sum_w |g[m,w]| |S_i[k,w]| |S_j[k,w]|

Everything is float64 / complex128 after the float32 phase argument of tests/ref64.py.

The bound of the covariance kernels (per real component of an element, u = 2^-24, spectra and weights taken as exact
float32 inputs), from the summation structure written at the top of psa_amd/csrc/covariance.hip.  A real component is
sum_w of two products per frequency (x_i (g x_j) + y_i (g y_j), or y_i (g x_j) + x_i (-g y_j)), each of modulus at most
|g| |S_i| |S_j|, so the sum of the moduli of all terms of a component is at most A.
  * The weighted operand g x is rounded once before it enters the matrix core: relative error u of every term, u A in
    all (the sign is exact).
  * A float32 accumulator is a chain of at most 2 COV_CHAIN FMAs (two per frequency; the fp32 MFMA is a k-ordered fmaf
    chain).  FMA number r rounds a partial sum of modulus at most the chain's own sum of moduli A_c: 2 COV_CHAIN u A_c.
  * The accumulator is folded at most COV_FOLDS times into a second float32 sum: each addition rounds a partial sum of
    modulus at most the slab's sum of moduli A_s: COV_FOLDS u A_s.  The sums of A_c over a slab's chains is A_s, of A_s
    over a k-point's slabs A.  (With one weight row a wavefront sums every other chain of a chunk: half the folds.)
  * A wavefront owns its (weight, tile pair, part) alone -- nothing is combined between wavefronts in float32, which the
    issue's formula allowed four additions for -- and the slabs are added, scaled and stored in float64 (2^-53: nothing
    on this scale).
To first order (1 + 2 COV_CHAIN + COV_FOLDS) u A; the second-order terms are below (2 COV_CHAIN + COV_FOLDS + 1)^2 u^2 / 2
< 0.003 u, and three more u are left as slack:

    |G_gpu - G_64| per real component  <=  (2 COV_CHAIN + COV_FOLDS + 4) u A  =  292 u A                  bound()

Derived, not measured.  A float32 NumPy chain in the kernel's structure without FMA (chain32: every product and every sum
rounded on its own, which rounds more often than the kernel) stays far inside it on the generator's inputs, while one
dropped frequency or one row truncated to bfloat16 exceeds it (tests/test_cov_host.py)."""
import re
from pathlib import Path

import numpy as np

from modes64 import _bf16, spectra64
from psa_amd import _hip

U = 2.0 ** -24
COV_CHAIN, COV_FOLDS, COV_TILE, COV_CHUNK = _hip.COV_CHAIN, _hip.COV_FOLDS, _hip.COV_TILE, _hip.COV_CHUNK
KERNEL_SOURCE = Path(__file__).resolve().parent.parent / "psa_amd" / "csrc" / "covariance.hip"


def kernel_constants():
    """{name: value} of the constexpr int COV_* constants in covariance.hip, read from its text (products of earlier
    constants are evaluated)"""
    out = {}
    for name, expr in re.findall(r"constexpr int (COV_\w+) = ([^;]+);", KERNEL_SOURCE.read_text()):
        out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))
    return out


def bound():
    """per-component bound of |G_gpu - G_64| in units of A (see the module text)"""
    return (2 * COV_CHAIN + COV_FOLDS + 4) * U


def rows(S):
    """(K, 3B, T) complex128: row i = 3 b + c of spectra (B, K, 3, T)"""
    S = np.asarray(S)
    B, K, _, T = S.shape
    return S.astype(np.complex128).transpose(1, 0, 2, 3).reshape(K, 3 * B, T)


def cov64(S, g, scale=1.0):
    """(G complex128, A float64), both (n_w, K, 3B, 3B), from spectra (B, K, 3, T) and weights (n_w, T) or (T,)"""
    X = rows(S)
    g = np.atleast_2d(np.asarray(g)).astype(np.float64)
    G = np.einsum("mw,kiw,kjw->mkij", g, X, np.conj(X), optimize=True) * scale
    A = np.einsum("mw,kiw,kjw->mkij", np.abs(g), np.abs(X), np.abs(X), optimize=True) * abs(scale)
    return G, A


def covariance64(data, mean, k, groups, g, weights=None, displacements=False):
    """(G, A) of the atom groups (index arrays) of a trajectory: cov64 of spectra64 (which carries the 1/T)"""
    return cov64(spectra64(data, mean, k, groups, weights, displacements), g)


def per_component(got, ref, A):
    """max over the elements and their real and imaginary parts of |got - ref| / A; elements whose A is zero must be
    exactly zero in got"""
    got, ref, A = np.asarray(got, np.complex128), np.asarray(ref, np.complex128), np.asarray(A, np.float64)
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    live = A > 0
    assert not np.any(got[~live]), "elements whose scale A is zero must be exactly zero"
    err = np.maximum(np.abs(got.real - ref.real), np.abs(got.imag - ref.imag))
    return float(np.max(err[live] / A[live])) if live.any() else 0.0


def kernel_case(B, T, K, n_w, seed=0):
    """Inputs of the bound test in the style of modes64.kernel_case: spectra (B, K, 3, T) complex64 whose rows span six
    decades in magnitude -- a factor 10^-1.5 from the first k-point to the last, 10^-4.5 at random within a k-point --
    with one frequency bin 10^3 louder; weights (n_w, T) float32: row 0 random in [0.25, 4), row 1 falling as 1/w^2
    over the positive and negative frequencies, both 0 at w = 0"""
    rng = np.random.default_rng(7000 * B + T + seed)
    mag = 10.0 ** (-4.5 * rng.random((B, K, 3, 1)) - 1.5 * (np.arange(K) / max(K - 1, 1))[None, :, None, None])
    S = mag * (rng.standard_normal((B, K, 3, T)) + 1j * rng.standard_normal((B, K, 3, T)))
    S[..., T // 3] *= 1e3
    w = np.fft.fftfreq(T) * T
    g = np.stack([rng.uniform(0.25, 4.0, T), 1.0 / np.where(w == 0, 1.0, w) ** 2])[:n_w]
    g[:, 0] = 0.0
    return np.ascontiguousarray(S.astype(np.complex64)), np.ascontiguousarray(g.astype(np.float32))


def loudest_row(S, k):
    """the row i = 3 b + c of k-point k with the largest magnitude"""
    return int(np.argmax(np.max(np.abs(rows(S)[k]), axis=-1)))


def chain32(S, g, drop=None, truncate=None):
    """(n_w, K, 3B, 3B) complex128 from float32 sums in the kernel's structure, without FMA (every product and every sum
    rounded on its own): per frequency the two products of a component are added to a float32 accumulator, which is
    folded into a second float32 sum every COV_CHAIN frequencies; the second sums of the chunks of COV_CHUNK
    frequencies are added in float64.  drop=(k, w): frequency w is left out at k-point k; truncate=(k, i): row i of
    k-point k enters truncated to bfloat16."""
    X = rows(S).astype(np.complex64)
    xr, xi = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)         # (K, n, T) float32
    g = np.atleast_2d(np.asarray(g, np.float32))
    if truncate is not None:
        k, i = truncate
        xr[k, i], xi[k, i] = _bf16(xr[k, i]), _bf16(xi[k, i])
    n_w, (K, n, T) = g.shape[0], xr.shape
    total = np.zeros((n_w, K, n, n), np.complex128)
    zero = lambda: np.zeros((n_w, K, n, n), np.float32)                           # noqa: E731
    acc_r, acc_i, fold_r, fold_i = zero(), zero(), zero(), zero()
    for w in range(T):
        a, b = xr[:, :, w].copy(), xi[:, :, w].copy()                           # (K, n)
        if drop is not None and drop[1] == w:
            a[drop[0]] = b[drop[0]] = 0.0
        for m in range(n_w):
            ga, gb = g[m, w] * a, g[m, w] * b                                     # the weighted operands, rounded once
            acc_r[m] = (acc_r[m] + a[:, :, None] * ga[:, None, :]) + b[:, :, None] * gb[:, None, :]
            acc_i[m] = (acc_i[m] + b[:, :, None] * ga[:, None, :]) + a[:, :, None] * (-gb)[:, None, :]
        if (w + 1) % COV_CHAIN == 0 or w + 1 == T:
            fold_r, fold_i = fold_r + acc_r, fold_i + acc_i
            acc_r, acc_i = zero(), zero()
        if (w + 1) % COV_CHUNK == 0 or w + 1 == T:
            total += fold_r.astype(np.float64) + 1j * fold_i.astype(np.float64)
            fold_r, fold_i = zero(), zero()
    return total
