"""A float64 restatement of the mode-projected SED (psa_amd/modes.py), the bound its contraction kernel is held to,
and the inputs and float32 models of the bound's tests (tests/test_gpu_modes.py, tests/test_modes_host.py).

    S_b[k,c,w]  = (1/T) sum_t exp(-2 pi i w t / T) sum_{a in b} w_a d[t,a,c] exp(i k.r_a)        spectra64
    Q[k,nu,w]   = sum_b sum_c conj(eig[k,nu,b,c]) S_b[k,c,w]
    Phi[w,k,nu] = |Q|^2,     A[w,k,nu] = sum_b sum_c |eig[k,nu,b,c]| |S_b[k,c,w]|                 contract64

The phase argument is the float32 FMA chain of tests/ref64.py (phase_argument), everything after it is float64 /
complex128.

The bound of the contraction kernel (per element, u = 2^-24, spectra and vectors taken as exact complex64 inputs).
In float32 a complex product errs by at most sqrt(2) 2u |e| |s| in modulus and a complex addition by u |z| (both parts
rounded once; Higham, Accuracy and Stability of Numerical Algorithms, section 3.6), so a complex dot product of
n = 3B terms summed in any order errs by (n + 2) u A to first order.  An FMA chain rounds the two real chains at other
points than "product, then sum"; twice that covers every such order:  |dQ| <= 2 (n + 2) u A.  The modulus
|Q|^2 = Qr^2 + Qi^2 then errs by 2 |Q| |dQ| + 2 u Phi with |Q| <= A and Phi <= A^2:

    |Phi_gpu - Phi_64|  <=  (4 (n + 2) + 2) u A^2  =  (12 B + 10) u A^2            bound(B); 106 u at B = 8

Derived, not measured.  A float32 NumPy chain without FMA (chain32) stays at 7-15 u on the shapes of CASES, so the
bound leaves room for any summation order and none for a lost term: one term truncated to bfloat16 (relative error
2^-8 of that term) or dropped exceeds it by orders of magnitude where that term carries the sum, while the global
rel_max of the same output stays under the project's 1e-5 bar (tests/test_modes_host.py)."""
import numpy as np

from ref64 import project64

U = 2.0 ** -24

# (B, M, T, K) of the kernel's bound test: T = 200, 100, 70 are no multiples of the kernel's 64-frequency tile, K = 5, 6
# leave a partial tile of 4 k-vectors, M = 39 takes several passes, B = 40 walks 120 rows per output
CASES = [(1, 3, 192, 3), (2, 6, 200, 5), (8, 24, 200, 5), (8, 5, 256, 3), (13, 39, 100, 6), (40, 7, 70, 3)]


def bound(B):
    """per-element bound of |Phi_gpu - Phi_64| in units of A^2 (see the module text)"""
    return (12 * B + 10) * U


def spectra64(data, mean, k, groups, weights=None, displacements=False):
    """(B, K, 3, T) complex128: the spectrum of each atom group (None: every atom; an empty group gives zeros)"""
    data = np.asarray(data)
    T = data.shape[0]
    out = np.zeros((len(groups), len(k), 3, T), np.complex128)
    for b, g in enumerate(groups):
        if g is not None and len(g) == 0:
            continue
        out[b] = np.fft.fft(project64(data, mean, k, g, weights, displacements), axis=-1) / T
    return out


def contract64(S, eig):
    """(Phi, A), both (T, K, M) float64, from spectra (B, K, 3, T) and mode vectors (K, M, B, 3)"""
    S = np.asarray(S).astype(np.complex128)
    e = np.asarray(eig).astype(np.complex128)
    Q = np.einsum("kmbc,bkcw->wkm", np.conj(e), S)
    A = np.einsum("kmbc,bkcw->wkm", np.abs(e), np.abs(S))
    return Q.real ** 2 + Q.imag ** 2, A


def mode_sed64(data, mean, k, groups, eig, weights=None, displacements=False):
    """(T, K, M) float64 mode-projected SED of the atom groups (index arrays) with mode vectors eig (K, M, B, 3)"""
    return contract64(spectra64(data, mean, k, groups, weights, displacements), eig)[0]


def per_element(got, ref, A):
    """max |got - ref| / A^2 over the elements whose A is not zero (those must be exactly zero in got)"""
    got, ref, A = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(A, np.float64)
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    live = A > 0
    assert not np.any(got[~live]), "elements whose scale A is zero must be exactly zero"
    return float(np.max(np.abs(got - ref)[live] / A[live] ** 2)) if live.any() else 0.0


def random_unitary(rng, K, B, M=None):
    """(K, M, B, 3) complex64: the first M rows of a random unitary 3B x 3B matrix per k-point (M = None: all 3B)"""
    n = 3 * B
    z = rng.standard_normal((K, n, n)) + 1j * rng.standard_normal((K, n, n))
    q = np.stack([np.linalg.qr(zk)[0] for zk in z])
    return np.ascontiguousarray(q[:, :(n if M is None else M), :].reshape(K, -1, B, 3).astype(np.complex64))


def kernel_case(B, M, T, K, seed=0):
    """Inputs of the bound test: spectra (B, K, 3, T) complex64 whose rows span six decades in magnitude -- a factor
    10^-1.5 from the first k-point to the last, 10^-4.5 at random within a k-point -- with one frequency bin 10^3
    louder, and random unitary mode vectors (K, M, B, 3)"""
    rng = np.random.default_rng(1000 * B + M + seed)
    mag = 10.0 ** (-4.5 * rng.random((B, K, 3, 1)) - 1.5 * (np.arange(K) / max(K - 1, 1))[None, :, None, None])
    S = mag * (rng.standard_normal((B, K, 3, T)) + 1j * rng.standard_normal((B, K, 3, T)))
    S[..., T // 3] *= 1e3
    return np.ascontiguousarray(S.astype(np.complex64)), random_unitary(rng, K, B, M)


def _bf16(x):
    """float32 values truncated to bfloat16 (the low 16 bits cleared)"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def loudest_term(S, k):
    """(b, c) of the row of k-point k with the largest magnitude"""
    mag = np.max(np.abs(S[:, k]), axis=-1)                 # (B, 3)
    return np.unravel_index(int(np.argmax(mag)), mag.shape)


def chain32(S, eig, truncate=None, drop=None):
    """(T, K, M) float32: the contraction as a float32 chain in the order of the terms, every product and every sum
    rounded on its own (NumPy has no FMA).  truncate=(k, b, c): that term's spectrum enters truncated to bfloat16;
    drop=(k, b, c): that term is left out."""
    S = np.ascontiguousarray(S, np.complex64)
    e = np.ascontiguousarray(eig, np.complex64)
    B, K, _, T = S.shape
    M = e.shape[1]
    qr, qi = np.zeros((T, K, M), np.float32), np.zeros((T, K, M), np.float32)
    for b in range(B):
        for c in range(3):
            x, y = S[b, :, c, :].real.T.copy(), S[b, :, c, :].imag.T.copy()          # (T, K) float32
            if truncate is not None and truncate[1:] == (b, c):
                x[:, truncate[0]], y[:, truncate[0]] = _bf16(x[:, truncate[0]]), _bf16(y[:, truncate[0]])
            if drop is not None and drop[1:] == (b, c):
                x[:, drop[0]] = y[:, drop[0]] = 0.0
            p, q = e[:, :, b, c].real[None], -e[:, :, b, c].imag[None]                # conj(eig): (1, K, M)
            qr = (qr + p * x[:, :, None]) - q * y[:, :, None]
            qi = (qi + p * y[:, :, None]) + q * x[:, :, None]
    return qr * qr + qi * qi
