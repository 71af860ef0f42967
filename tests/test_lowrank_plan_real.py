"""The real-weights form of the low-rank plan (api_lowrank.hip): L[j, l] = L_l(kappa_j) and phi[j] = exp(i kappa_j x_c),
each rounded to float32 on its own, are the two factors of the combine matrix C = phi L that lowrank_combine_r_kernel
sums with (one packed FMA per node, one phase multiply per output element).  Their product must be the plan's fp64
cos/sin . L to the float32 rounding of the two factors, and row j of either must depend on k_j and the node interval
only -- the route's row determinism rests on that, as it does for C.  No GPU: the plan is host code."""
import numpy as np
import pytest

from test_lowrank_plan import _path


def _fp64_factors(p, vecs):
    """the plan's own fp64 arithmetic restated: barycentric Lagrange weights at kappa_j and cos/sin(kappa_j x_c)"""
    kap = (vecs.astype(np.float64) - p["k0"]) @ p["u"]
    bw = (-1.0) ** np.arange(64) * np.sin(np.pi * (2 * np.arange(64) + 1) / 128)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = bw[None, :] / (kap[:, None] - p["kappa"][None, :])
        L /= L.sum(axis=1, keepdims=True)
    hit = kap[:, None] == p["kappa"][None, :]
    L[hit.any(axis=1)] = hit[hit.any(axis=1)].astype(np.float64)
    return L, np.exp(1j * kap * p["x_c"])


@pytest.mark.parametrize("sign", [1, -1])
def test_factors_multiply_to_the_fp64_matrix(sign):
    """phi[j] L[j, l] in float64 against cos/sin(kappa_j x_c) L_l(kappa_j): two float32 roundings, 2^-24 relative each,
    so 2^-23 of max_l |L[j, l]| per entry (|phi| = 1) -- for the C3 path and its mirror image from -Gamma"""
    from psa_amd import _hip
    r0, vecs, _ = _path("C3")
    vecs = (sign * vecs).astype(np.float32)
    p = _hip.lowrank_plan(vecs, r0)
    assert p is not None and p["interval"] == (0 if sign > 0 else -1)
    assert p["L"].dtype == np.float32 and p["L"].shape == (len(vecs), 64)
    assert p["phi"].dtype == np.complex64 and p["phi"].shape == (len(vecs),)
    L64, phi64 = _fp64_factors(p, vecs)
    want = phi64[:, None] * L64
    got = p["phi"].astype(np.complex128)[:, None] * p["L"].astype(np.float64)
    scale = np.max(np.abs(L64), axis=1, keepdims=True)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)) / scale
    print(f"sign {sign:+d}: max |phi L - fp64| / max_l |L| = {err.max():.3e} (bound {2.0 ** -23:.3e}), "
          f"Lebesgue sum max {np.abs(L64).sum(axis=1).max():.2f}")
    assert err.max() <= 2.0 ** -23
    # each factor is the float32 nearest its fp64 value (the device sums with exactly these)
    assert np.max(np.abs(p["L"].astype(np.float64) - L64) / scale) <= 2.0 ** -24
    assert np.max(np.abs(p["phi"].astype(np.complex128) - phi64)) <= 2.0 ** -24 * np.sqrt(2.0)


@pytest.mark.parametrize("sign", [1, -1])
def test_sub_lists_get_the_same_rows(sign):
    """halves, and 96 + 160: L and phi of a part are the whole list's rows, bit for bit"""
    from psa_amd import _hip
    r0, vecs, _ = _path("C3")
    vecs = (sign * vecs).astype(np.float32)
    K = len(vecs)
    assert K == 256
    whole = _hip.lowrank_plan(vecs, r0)
    assert whole is not None
    for lo, hi in [(0, K // 2), (K // 2, K), (0, 96), (96, K)]:
        p = _hip.lowrank_plan(vecs[lo:hi], r0)
        assert p is not None
        assert np.array_equal(p["L"].view(np.uint32), whole["L"][lo:hi].view(np.uint32)), (lo, hi)
        assert np.array_equal(p["phi"].view(np.uint32), whole["phi"][lo:hi].view(np.uint32)), (lo, hi)
