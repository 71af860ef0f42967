"""A float64 restatement of the SED of one atom group, for checking the projection kernels against more than the
float32 oracle (tests/test_gpu_lowrank_envelope.py, tests/test_gpu_dense_envelope.py).

The phase argument is the reference's own: the float32 product np.dot(k, r.T), which equals the device's FMA chain
fma(kz, rz, fma(ky, ry, kx rx)) (tests/test_oracle_golden.py::test_phase_argument_is_fma_chain).  It is not rebuilt
from separately rounded products: at a few hundred radians one ulp of it is 3e-5 rad.  Everything after it -- exp,
the weights, the projection, the FFT and the 1/T -- is float64 / complex128.

line=plan (a dict of psa_amd._hip.lowrank_plan) gives the "line only" SED instead: exp(i k~.r) in float64, k~ the
k-vector projected on the plan's line.  That is what the low-rank k-path route returns if its D term is lost; a test
that tells the two apart can see D.

project64 / scale_B / gamma are the pre-FFT form for the dense kernels: output element q[k, c, t] = sum_a w_a d[t, a, c]
exp(i k.r_a) has the natural scale B[c, t] = sum_a |w_a d[t, a, c]| (|exp| = 1), and gamma is the largest error of any
element in units of its own B.  Unlike a maximum over a global maximum it sees a kernel that is wrong only where the
output is small (quiet frames, slow atoms).  Its phase argument is the FMA chain written out (phase_argument): np.dot
is that chain only where BLAS takes its matrix-matrix kernel; with one atom or one k-vector it takes a matrix-vector
kernel that sums in another order (up to 3 ulp of the argument apart, 48 x 2^-24 in cos near a zero), and those shapes
are cases of the dense suite.  The device computes the chain whatever the shape."""
import numpy as np


def phase_argument(k_vectors, r):
    """(K, n) float32: fma(kz, rz, fma(ky, ry, kx rx)), each step the exact float64 product and sum rounded once to
    float32 (as tests/test_oracle_golden.py::test_phase_argument_is_fma_chain restates it)"""
    k = np.ascontiguousarray(k_vectors, np.float32).astype(np.float64)
    r = np.ascontiguousarray(r, np.float32).astype(np.float64)
    arg = (k[:, 0:1] * r[None, :, 0]).astype(np.float32)
    for i in (1, 2):
        arg = (k[:, i:i + 1] * r[None, :, i] + arg.astype(np.float64)).astype(np.float32)
    return arg


def phases(k_vectors, r, line=None, chain=False):
    """(K, n) complex128 phase matrix exp(i k.r) of float32 k-vectors and positions; chain: the argument from
    phase_argument instead of np.dot"""
    k32 = np.ascontiguousarray(k_vectors, np.float32)
    r32 = np.ascontiguousarray(r, np.float32)
    if line is None:
        arg = (phase_argument(k32, r32) if chain else np.dot(k32, r32.T)).astype(np.float64)
    else:
        u, k0 = np.asarray(line["u"], np.float64), np.asarray(line["k0"], np.float64)
        kap = (k32.astype(np.float64) - k0) @ u
        kline = k0[None, :] + kap[:, None] * u[None, :]
        arg = kline @ r32.astype(np.float64).T
    return np.exp(1j * arg)


def _group_data(data, mean_pos_all, g, displacements):
    """(T, n, 3) float64 data of the group g: the array as it is, or the float32 difference positions - mean (the
    reference's temporary in displacement mode)"""
    d = np.asarray(data)[:, g, :]
    if displacements:
        d = d.astype(np.float32) - np.asarray(mean_pos_all, np.float32)[g][None, :, :]
    return d.astype(np.float64)


def _group(data, idx):
    return np.arange(np.asarray(data).shape[1]) if idx is None else np.asarray(idx, np.int64)


def project64(data, mean_pos_all, k_vectors, idx=None, weights=None, displacements=False):
    """(K, 3, T) complex128: q[k, c, t] = sum_a w_a d[t, a, c] exp(i k.r_a) over the group idx (None: every atom; an
    index list may repeat atoms), the layout of Engine.debug_project_only.  displacements: d = positions - mean."""
    g = _group(data, idx)
    P = phases(k_vectors, np.asarray(mean_pos_all, np.float32)[g], chain=True)      # (K, n)
    if weights is not None:
        P = P * np.asarray(weights, np.float32)[g].astype(np.float64)[None, :]
    d = _group_data(data, mean_pos_all, g, displacements)                          # (T, n, 3)
    q = np.empty((P.shape[0], 3, d.shape[0]), np.complex128)
    for c in range(3):
        dc = np.ascontiguousarray(d[:, :, c].T)                                    # (n, T)
        q[:, c, :] = P.real @ dc + 1j * (P.imag @ dc)
    return q


def scale_B(data, mean_pos_all, idx=None, weights=None, displacements=False):
    """(3, T) float64: B[c, t] = sum_a |w_a d[t, a, c]| over the group, duplicates counted"""
    g = _group(data, idx)
    d = np.abs(_group_data(data, mean_pos_all, g, displacements))
    if weights is not None:
        d = d * np.abs(np.asarray(weights, np.float32)[g].astype(np.float64))[None, :, None]
    return np.ascontiguousarray(d.sum(axis=1).T)


def gamma(got, ref, B):
    """max over all elements (K, 3, T), real and imaginary parts taken separately, of |got - ref| / B[c, t].  Elements
    whose B is zero must be exactly zero in got (asserted) and are left out of the maximum."""
    got, ref, B = np.asarray(got), np.asarray(ref), np.asarray(B, np.float64)
    assert got.shape == ref.shape and B.shape == ref.shape[1:], (got.shape, ref.shape, B.shape)
    err = np.maximum(np.abs(got.real.astype(np.float64) - ref.real), np.abs(got.imag.astype(np.float64) - ref.imag))
    live = np.broadcast_to(B > 0, err.shape)
    assert not np.any(got[~live]), "elements whose scale B is zero must be exactly zero"
    if not live.any():
        return 0.0
    return float(np.max(err[live] / np.broadcast_to(B, err.shape)[live]))


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
