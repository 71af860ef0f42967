"""A float64 restatement of the SED of one atom group, for checking the projection kernels against more than the
float32 oracle (tests/test_gpu_lowrank_envelope.py).

The phase argument is the reference's own: the float32 product np.dot(k, r.T), which equals the device's FMA chain
fma(kz, rz, fma(ky, ry, kx rx)) (tests/test_oracle_golden.py::test_phase_argument_is_fma_chain).  It is not rebuilt
from separately rounded products: at a few hundred radians one ulp of it is 3e-5 rad.  Everything after it -- exp,
the weights, the projection, the FFT and the 1/T -- is float64 / complex128.

line=plan (a dict of psa_amd._hip.lowrank_plan) gives the "line only" SED instead: exp(i k~.r) in float64, k~ the
k-vector projected on the plan's line.  That is what the low-rank k-path route returns if its D term is lost; a test
that tells the two apart can see D."""
import numpy as np


def phases(k_vectors, r, line=None):
    """(K, n) complex128 phase matrix exp(i k.r) of float32 k-vectors and positions"""
    k32 = np.ascontiguousarray(k_vectors, np.float32)
    r32 = np.ascontiguousarray(r, np.float32)
    if line is None:
        arg = np.dot(k32, r32.T).astype(np.float64)
    else:
        u, k0 = np.asarray(line["u"], np.float64), np.asarray(line["k0"], np.float64)
        kap = (k32.astype(np.float64) - k0) @ u
        kline = k0[None, :] + kap[:, None] * u[None, :]
        arg = kline @ r32.astype(np.float64).T
    return np.exp(1j * arg)


def sed64(data, mean_pos_all, k_vectors, idx=None, weights=None, line=None):
    """(T, K, 3) complex128: fft_t(sum_a w_a d[t, a, :] exp(i k.r_a)) / T over the group idx (None: every atom, an
    index list may repeat atoms).  data (T, N, 3) is projected as it is (velocities, or positions without the
    displacement flag); weights (N,) are per atom of the trajectory."""
    data = np.asarray(data)
    T = data.shape[0]
    g = np.arange(data.shape[1]) if idx is None else np.asarray(idx, np.int64)
    P = phases(k_vectors, np.asarray(mean_pos_all, np.float32)[g], line)            # (K, n)
    if weights is not None:
        P = P * np.asarray(weights, np.float32)[g].astype(np.float64)[None, :]
    Pr, Pi = np.ascontiguousarray(P.real.T), np.ascontiguousarray(P.imag.T)          # (n, K)
    q = np.empty((T, P.shape[0], 3), np.complex128)
    for c in range(3):
        d = data[:, g, c].astype(np.float64)
        q[:, :, c] = d @ Pr + 1j * (d @ Pi)
    return np.fft.fft(q, axis=0) / T


def intensity64(data, mean_pos_all, k_vectors, groups, weights=None, line=None):
    """(T, K) float64 incoherent intensity: sum over the groups and the components of |sed64|^2"""
    out = 0.0
    for g in groups:
        out = out + np.sum(np.abs(sed64(data, mean_pos_all, k_vectors, g, weights, line)) ** 2, axis=-1)
    return out


def row_rel(got, ref):
    """(K,) relative error of each k-row: its max |got - ref| over the row's own max |ref| (axis 1 is k)"""
    got, ref = np.asarray(got), np.asarray(ref)
    axes = tuple(i for i in range(ref.ndim) if i != 1)
    den = np.max(np.abs(ref), axis=axes)
    return np.max(np.abs(got - ref), axis=axes) / np.where(den > 0, den, 1.0)
