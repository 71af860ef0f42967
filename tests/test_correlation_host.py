"""The time correlations without a GPU: the NumPy float32 twin of the route (tests/correlation_cases.twin) against the
time-domain float64 reference (tests/correlation64) inside the end-to-end bar on the families of the issue; the padded
float64 route against the time-domain sums; every planted fault caught by the same bar; `relaxation_time`; the Python
refusals, which come before anything is uploaded."""
import math

import numpy as np
import pytest

import correlation64 as R
import correlation_cases as CC
import lattice64
import self64
import self_cases as S

WALK = [(250, 250, 250, 125), (250, 64, 32, 64), (250, 63, 31, 40), (256, 64, 64, 1), (250, 64, 32, 33)]


@pytest.fixture(scope="module")
def walk_series():
    """z (40 x 3, T) of 40 random-walk atoms at three vectors, float64, T = 256 (the cases use the first T frames)"""
    pos = S.random_walk(40, 256, seed=3)[0]
    w = S.weights("sqrt_mass", 40, seed=4)
    z = self64.series64(pos, np.array([[1, 0, 2], [2, -1, 3], [0, 3, 1]]), S.inverse(S.CUBIC), None, w)
    return z.reshape(-1, 256)


@pytest.fixture(scope="module")
def coherent_series():
    """q_0 (5, 256) of 130 atoms wandering about their sites: a coherent sum with a large static part"""
    pos, vel = S.C.trajectory(130, 256, seed=5)
    return lattice64.project64(pos, vel, S.C.mixed_indices(5, seed=5), S.inverse(S.CUBIC), currents=False)[:, 0]


@pytest.mark.parametrize("case", WALK, ids=lambda c: "_".join(map(str, c)))
def test_twin_inside_the_bar_random_walk(walk_series, case):
    T, L, H, n_lags = case
    x = walk_series[:, :T]
    ref = R.correlate64(x, L, H, n_lags).T                                 # (n_lags, rows)
    got = CC.twin(x, L, H, n_lags).T
    frac = np.max(np.abs(got - ref) / ref[:1])
    print(f"{case}: twin against the time-domain sums, {frac:.1e} of F[0]; {CC.worst_fraction(got, ref, L):.2e} of the bar")
    assert np.all(np.abs(got - ref) <= CC.end_to_end_bar(ref, L))
    if H == L:                                                             # F[0] is the mean of |x|^2 over the frames used
        np.testing.assert_allclose(ref[0], np.mean(np.abs(x[:, :(T // L) * L]) ** 2, axis=1), rtol=1e-12)
    # the padded route in float64 agrees with the time-domain sums to rounding
    P, n_seg = CC.padded_length(L, n_lags), 1 + (T - L) // H
    X = np.zeros((x.shape[0], P))
    for s in range(n_seg):
        X += np.abs(np.fft.fft(x[:, s * H:s * H + L], n=P, axis=1)) ** 2
    F = CC.transform64(X.T[None], L, n_seg, n_lags, exact=False)[0]
    assert np.max(np.abs(F - ref) / ref[:1]) <= 1e-13


def test_twin_inside_the_bar_coherent(coherent_series):
    T, L, H, n_lags = 256, 64, 32, 48
    ref = R.correlate64(coherent_series, L, H, n_lags).T
    got = CC.twin(coherent_series, L, H, n_lags).T
    print(f"coherent: {np.max(np.abs(got - ref) / ref[:1]):.1e} of F[0]")
    assert np.all(np.abs(got - ref) <= CC.end_to_end_bar(ref, L))


@pytest.mark.parametrize("fault", [f for f in CC.FAULTS if f != "mul32"])
def test_planted_faults_are_caught(walk_series, fault):
    # (64, 32, 64): n_lags > P - L + 1 for P = 64, the last lag has one origin per segment, several segments
    T, L, H, n_lags = 250, 64, 32, 64
    x = walk_series[:, :T]
    ref = R.correlate64(x, L, H, n_lags).T
    assert np.all(np.abs(CC.twin(x, L, H, n_lags).T - ref) <= CC.end_to_end_bar(ref, L))
    bad = CC.twin(x, L, H, n_lags, fault=fault).T
    worst = CC.worst_fraction(bad, ref, L)
    print(f"{fault}: {worst:.1e} of the bar")
    assert worst > 10


def test_product_in_32_bits_is_caught():
    """o t reduced in 32 bits: harmless while P divides 2^32, so P = 3 x 2^15 and o0 t up to 5.9e9"""
    P, n_lags = 98304, 60000
    good, bad = CC.single_line(P - 1, P, n_lags), CC.single_line(P - 1, P, n_lags, "mul32")
    assert (P - 1) * (n_lags - 1) > 2 ** 32
    t = np.arange(n_lags)
    np.testing.assert_allclose(good, np.cos(2 * np.pi * t / P) / P, rtol=0, atol=1e-18)     # o0 = -1 mod P
    X = np.zeros((1, P, 1))
    X[0, P - 1, 0] = 1.0
    bar = CC.transform_bar(X, n_lags, 1, n_lags, good[None, :, None] / CC.origins(n_lags, 1, n_lags)[None, :, None])
    assert np.max(np.abs(bad - good) / CC.origins(n_lags, 1, n_lags) / bar[0, :, 0]) > 1e6


def test_transform_reference_is_the_definition():
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (2, 96, 3))
    got = CC.transform64(X, 50, 2, 50)
    t, o = np.arange(50)[:, None], np.arange(96)[None, :]
    want = np.stack([np.cos(2 * np.pi * o * t / 96) @ X[f] for f in range(2)]) / (96 * 2 * (50 - np.arange(50)))[None, :, None]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    assert np.all(CC.transform_bar(X, 50, 2, 50, got) > 0)


def test_fields_reference():
    """density, longitudinal and transverse at lag 0 are the mean squares of q_0, khat.q and half the perpendicular part"""
    pos, vel = S.C.trajectory(20, 64, seed=9, box=S.TRICLINIC)
    inv, ind = S.inverse(S.TRICLINIC), S.C.mixed_indices(4, seed=2)[[0, 2, 3]]
    q = lattice64.project64(pos, vel, ind, inv)
    den, lon, tra = R.fields64(q, ind, inv, 32, 16, 8)
    frames = slice(0, 64)
    tot = np.mean(np.sum(np.abs(q[:, 1:, frames]) ** 2, axis=1), axis=1)
    # every frame is used by two segments but the first and the last 16: compare where H = L instead
    den1, lon1, tra1 = R.fields64(q, ind, inv, 32, 32, 1)
    np.testing.assert_allclose(den1[0], np.mean(np.abs(q[:, 0]) ** 2, axis=1), rtol=1e-12)
    np.testing.assert_allclose(lon1[0] + 2 * tra1[0], tot, rtol=1e-12)
    assert den.shape == lon.shape == tra.shape == (8, 3)


def test_relaxation_time():
    from psa_amd import relaxation_time
    t = np.arange(200) * 0.05
    for tau in (0.7, 2.0):
        got = relaxation_time(np.exp(-t / tau), t)
        assert abs(got - tau) <= 0.05 ** 2 / tau                           # linear interpolation of a convex function
    F = np.stack([3 * np.exp(-t / 1.5), np.ones_like(t), np.exp(-t / 0.3)], axis=1)
    got = relaxation_time(F, t)
    assert got.shape == (3,) and abs(got[0] - 1.5) < 1e-2 and math.isnan(got[1]) and abs(got[2] - 0.3) < 1e-2
    assert relaxation_time(np.exp(-t / 2.0), t, level=0.5) == pytest.approx(2.0 * math.log(2), abs=1e-3)
    assert math.isnan(relaxation_time(np.ones(5), np.arange(5)))           # never crosses
    assert relaxation_time(np.ones(5), np.arange(5) + 2.0, level=1.5) == 2.0   # starts below the level: the first time
    assert math.isnan(relaxation_time(np.zeros(5), np.arange(5)))          # nothing to normalise by
    with pytest.raises(ValueError):
        relaxation_time(np.ones((4, 2)), np.arange(5))


def test_result_classes():
    from psa_amd import PowderTimeCorrelations, TimeCorrelations
    den = np.array([[2.0, 0.0], [1.0, 0.0]], np.float32)
    r = TimeCorrelations(den, None, None, np.arange(2) * 0.1, np.array([4, 3]), np.zeros(2), np.zeros((2, 3)), np.arange(3), 3.0, 0.1)
    n = r.normalized()
    assert n[1, 0] == 0.5 and np.isnan(n[:, 1]).all()
    with pytest.raises(ValueError):
        r.normalized("longitudinal")
    with pytest.raises(ValueError):
        r.normalized("speed")
    assert PowderTimeCorrelations.normalized is TimeCorrelations.normalized


def _calculator(n_frames=64, shard=None):
    from psa_amd import SEDCalculator, Trajectory
    pos = S.random_walk(8, n_frames, seed=1)[0]
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(8, np.int32), np.arange(n_frames, dtype=np.float32), S.CUBIC,
                    np.diag(S.CUBIC).copy(), np.zeros(3, np.float32), 0.002)
    calc = SEDCalculator(tr, 1, 1, 1)
    calc._shard = shard
    return calc


class _Untouchable:
    """an engine that fails the test when anything is asked of it: the refusals come before any upload"""
    def __getattr__(self, name):
        raise AssertionError(f"the engine was asked for {name}")


METHODS = [("calculate_lattice_correlations", np.array([[1, 0, 0]])), ("calculate_self_correlations", np.array([[1, 0, 0]])),
           ("calculate_powder_correlations", np.array([0.2, 0.6])), ("calculate_powder_self_correlations", np.array([0.2, 0.6]))]


@pytest.mark.parametrize("method,first", METHODS, ids=[m for m, _ in METHODS])
def test_python_refusals(method, first):
    from psa_amd import Segments
    calc = _calculator()
    calc._engine = _Untouchable()
    call = getattr(calc, method)
    with pytest.raises(ValueError, match="lags"):
        call(first, lags=65)                                               # > L = T
    with pytest.raises(ValueError, match="lags"):
        call(first, lags=33, segments=Segments(32, 16, "boxcar"))          # > L
    with pytest.raises(ValueError, match="lags"):
        call(first, lags=0)
    with pytest.raises(ValueError, match="lags"):
        call(first, lags=2.5)
    with pytest.raises(ValueError, match="boxcar"):
        call(first, segments=Segments(32, 16, "hann"))
    with pytest.raises(ValueError, match="boxcar"):
        call(first, segments=Segments(32, 16, tuple([1.0] * 31 + [0.5])))
    with pytest.raises(TypeError):
        call(first, segments=(32, 16))

    class Shard:
        nranks = 2
    with pytest.raises(NotImplementedError):
        getattr(_calculator(shard=Shard()), method)(first)
