"""A float64 NumPy restatement of the Lorentzian peak fit (include/psa_hip.h, psa_fit_peaks; kernels: psa_amd/csrc/peaks.hip),
the inputs of its tests, the comparison and the bound (tests/test_gpu_peaks.py, tests/test_peaks_host.py).  No SciPy.

A spectrum is phi (F, C) float32; row i is bin i of an F-point transform, f_i = i df.  Column j has a band [lo, hi) of
bins inside the positive half 1 .. ceil(F/2) - 1.

    window   p = lowest bin of the band where phi is largest; half = 0.5f phi[p]; l (r) consecutive bins below (above) p
             inside the band with phi >= half; h0 = max(1, (l + r + 1) / 2); n = clamp(ceil(window_hwhm h0), 4, 2047) or
             clamp(half_window_bins, 4, 2047); [a, b) = [max(lo, p - n), min(hi, p + n + 1)).  Integer and float32 only:
             the GPU must agree exactly.
    fit      least squares of  height hwhm^2 / ((f - f0)^2 + hwhm^2) + baseline  over [a, b) by Levenberg-Marquardt with
             Marquardt's diagonal scaling in x = (i - p) / h0, y = phi[i] / phi[p], from f0 = 0, hwhm = 1,
             baseline = min y, height = 1 - baseline; steps with hwhm <= 0 rejected; stop when the largest step is at
             most `tol` (f0, hwhm relative to hwhm; height, baseline relative to height).  Here tol = 1e-10 and
             float64 throughout; `arithmetic=np.float32` is the float32-arithmetic copy (every elementwise operation and
             every sum in float32, the 4 x 4 solve in float64) with the product's stop 1e-6.
    status   0 converged; 1 iteration cap; 2 no fit (band < 5 bins, phi[p] <= 0, non-finite value in the band: NaN);
             3 converged with f0 outside [a, b) or hwhm > b - a bins.

The bound, BOUND = 1e-4 on the four measures of `compare` (|df0| / hwhm, |dhwhm| / hwhm, |dheight| / height,
|dbaseline| / height, all over the reference's values), is measured, not derived: the float32-arithmetic copy agrees with
the float64 fit to <= 2.0e-6 on the clean Lorentzians of SHAPES (windows of 22 .. 4095 bins, one clipped at bin 1) and
<= 3.6e-7 on the (1024, 130) spectrum with 64-segment chi-square noise; the float64 fit stopped at the product's 1e-6
agrees to 3.2e-7.  1e-4 leaves two decades for another summation order and another last iteration, and is
two decades below the statistical error of such a spectrum (2 .. 4 % of hwhm).  tests/test_peaks_host.py holds every
asserted case to it on the CPU first (float32 copy against float64) and shows that the comparison can fail."""
import numpy as np

BOUND = 1e-4
N_MIN, N_MAX, MIN_BAND = 4, 2047, 5


# ------------------------------------------------------------------------------------------------- bands
def positive_half(F):
    """[1, ceil(F/2)): the bins a band may cover"""
    return 1, (F + 1) // 2


def bands(F, df, C, band=None, centers=None, search=None):
    """(C, 2) int32 bands [lo, hi) from frequencies: `band` = (fmin, fmax) for all columns (None: the positive half),
    `centers` (C,) with `search`: [center - search, center + search] cut to the global band.  lo = ceil(fmin / df),
    hi = floor(fmax / df) + 1, clipped to the positive half."""
    p_lo, p_hi = positive_half(F)
    g_lo, g_hi = p_lo, p_hi
    if band is not None:
        g_lo, g_hi = max(p_lo, int(np.ceil(band[0] / df))), min(p_hi, int(np.floor(band[1] / df)) + 1)
    out = np.empty((C, 2), np.int32)
    out[:] = (g_lo, g_hi)
    if centers is not None:
        c = np.asarray(centers, np.float64).reshape(C)
        out[:, 0] = np.maximum(g_lo, np.ceil((c - search) / df).astype(np.int64))
        out[:, 1] = np.minimum(g_hi, np.floor((c + search) / df).astype(np.int64) + 1)
    return out


# ------------------------------------------------------------------------------------------------- window
def window(col, lo, hi, window_hwhm=8.0, half_window_bins=0):
    """(p, h0, a, b) of one float32 column, or None where nothing is fitted (status 2)"""
    col = np.asarray(col, np.float32)
    seg = col[lo:hi]
    if hi - lo < MIN_BAND or not np.all(np.isfinite(seg)):
        return None
    p = lo + int(np.argmax(seg))
    if not col[p] > 0:
        return None
    half = np.float32(0.5) * col[p]
    below, above = col[lo:p][::-1] >= half, col[p + 1:hi] >= half
    l = int(np.argmin(below)) if not below.all() else below.size
    r = int(np.argmin(above)) if not above.all() else above.size
    h0 = max(np.float32(1), np.float32(0.5) * np.float32(l + r + 1))
    n = int(half_window_bins) if half_window_bins else int(min(np.ceil(np.float32(window_hwhm) * h0), np.float32(N_MAX)))
    n = min(max(n, N_MIN), N_MAX)
    return p, float(h0), max(lo, p - n), min(hi, p + n + 1)


# ------------------------------------------------------------------------------------------------- fit
def _sums(x, y, q, ar):
    """normal equations at q = (f0, w, A, c): J^T J (4, 4), J^T r (4,), r^T r -- elementwise work and sums in `ar`"""
    f0, w, A, c = (ar(v) for v in q)
    d = x - f0
    inv_D = ar(1) / (d * d + w * w)
    L = w * w * inv_D
    r = y - (A * L + c)
    t = ar(2) * A * L * inv_D
    J = np.stack([t * d, t * d * d / w, L, np.ones_like(x)])
    N = np.array([[np.sum(J[i] * J[j], dtype=ar) for j in range(4)] for i in range(4)], np.float64)
    g = np.array([np.sum(J[i] * r, dtype=ar) for i in range(4)], np.float64)
    return N, g, float(np.sum(r * r, dtype=ar))


def _step(N, g, lam):
    """(N + lam diag N) delta = g through Marquardt's scaling; None where the scaled matrix is not positive definite"""
    diag = np.diag(N)
    s = np.where(diag > 0, 1.0 / np.sqrt(np.where(diag > 0, diag, 1.0)), 1.0)
    M = N * s[:, None] * s[None, :]
    M[np.diag_indices(4)] = 1.0 + lam
    try:
        z = np.linalg.solve(np.linalg.cholesky(M).T, np.linalg.solve(np.linalg.cholesky(M), g * s))
    except np.linalg.LinAlgError:
        return None
    return z * s


def fit_column(col, lo, hi, df, window_hwhm=8.0, half_window_bins=0, max_iter=50, tol=1e-10, arithmetic=np.float64):
    """(fit (6,) float64, info (4,) int): f0, hwhm, height, baseline, rss, peak bin; status, iterations, a, b - a"""
    win = window(col, lo, hi, window_hwhm, half_window_bins)
    if win is None:
        return np.full(6, np.nan), np.array([2, 0, 0, 0])
    p, h0, a, b = win
    ar = arithmetic
    peak = ar(col[p])
    x = (np.arange(a, b) - p).astype(ar) / ar(h0)
    y = np.asarray(col[a:b], ar) / peak
    c0 = float(y.min())
    q = np.array([0.0, 1.0, 1.0 - c0, c0])
    lam, it, status = 1e-3, 0, 1
    N, g, rss = _sums(x, y, q, ar)
    while it < max_iter:
        it += 1
        d = _step(N, g, lam)
        if d is None or not q[1] + d[1] > 0:
            lam *= 10
            continue
        N2, g2, rss2 = _sums(x, y, q + d, ar)
        small = max(abs(d[0]), abs(d[1])) <= tol * q[1] and max(abs(d[2]), abs(d[3])) <= tol * abs(q[2])
        if rss2 <= rss * (1.0 + 64.0 * float(np.finfo(ar).eps)):      # downhill up to the rounding of the sums
            q, N, g, rss = q + d, N2, g2, rss2
            lam = max(0.1 * lam, 1e-12)
        else:
            lam *= 10
        if small:
            status = 0
            break
    f0_bin, w_bin = p + q[0] * h0, q[1] * h0
    if status == 0 and (f0_bin < a or f0_bin >= b or w_bin > b - a):
        status = 3
    pk = float(col[p])
    return (np.array([f0_bin * df, w_bin * df, q[2] * pk, q[3] * pk, rss * pk * pk, p], np.float64),
            np.array([status, it, a, b - a]))


def fit(spec, df, bands_=None, lo=None, hi=None, **kw):
    """every column of spec (F, C): (fit (C, 6) float64, info (C, 4) int64)"""
    spec = np.asarray(spec, np.float32)
    F, C = spec.shape
    if bands_ is None:
        p_lo, p_hi = positive_half(F)
        bands_ = np.tile(np.array([[p_lo if lo is None else lo, p_hi if hi is None else hi]]), (C, 1))
    out = [fit_column(spec[:, j], int(bands_[j][0]), int(bands_[j][1]), df, **kw) for j in range(C)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def fit32(spec, df, bands_=None, lo=None, hi=None, **kw):
    """the float32-arithmetic copy with the product's stop"""
    return fit(spec, df, bands_, lo, hi, tol=1e-6, arithmetic=np.float32, **kw)


# ------------------------------------------------------------------------------------------------- comparison
def compare(got, ref):
    """the four measures, each the largest over the columns given: |df0| / hwhm, |dhwhm| / hwhm, |dheight| / height,
    |dbaseline| / height, relative to the reference's hwhm and height.  got, ref: (..., >= 4) fits of the same columns"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got[..., :4]).all() and np.isfinite(ref[..., :4]).all()
    w, h = ref[..., 1], np.abs(ref[..., 2])
    return (float(np.max(np.abs(got[..., 0] - ref[..., 0]) / w)), float(np.max(np.abs(got[..., 1] - ref[..., 1]) / w)),
            float(np.max(np.abs(got[..., 2] - ref[..., 2]) / h)), float(np.max(np.abs(got[..., 3] - ref[..., 3]) / h)))


def within(got, ref, bound=BOUND):
    return max(compare(got, ref)) <= bound


def rss_agrees(got_fit, ref_fit, ref_info):
    """|rss - rss_ref| <= 1e-3 rss_ref + 1e-10 height^2 (b - a)"""
    got_fit, ref_fit = np.asarray(got_fit, np.float64), np.asarray(ref_fit, np.float64)
    return np.abs(got_fit[:, 4] - ref_fit[:, 4]) <= 1e-3 * ref_fit[:, 4] + 1e-10 * ref_fit[:, 2] ** 2 * np.asarray(ref_info)[:, 3]


# ------------------------------------------------------------------------------------------------- cases
def lorentzian(i, f0, w, A):
    return A * w * w / ((i - f0) ** 2 + w * w)


# (F, C) of the kernel test: fewer columns than a wavefront; a column count across 64 and across the four columns of a
# workgroup, odd F; more columns than peak_find's 256 would need slices for; the 4095-bin cap
SHAPES = [(256, 15), (100, 70), (1024, 130), (8192, 3)]


def clean_case(F, C, seed=0, mirror_height=0.3):
    """(phi (F, C) float32, truth (C, 4) float64 = f0, hwhm (bins), height, baseline): per column one Lorentzian, a weaker
    mirror peak (`mirror_height` of the height, elsewhere in the positive half; 0: none, the model itself), a baseline of 1 .. 5 % -- heights from 1e-6 to 1e3
    across the columns, widths from 1.3 bins up to what the half spectrum holds.  Column 0 is placed so that its window is
    clipped at bin 1 to exactly 64 bins (F >= 256); in the 8192-bin case column 0 sits in the middle of the half spectrum
    with 300 bins of half width: its window is the 4095-bin cap."""
    rng = np.random.default_rng(1000 * F + C + seed)
    top = (F + 1) // 2
    i = np.arange(F, dtype=np.float64)[:, None]
    w_max = max(2.0, top / 40.0)
    w = np.exp(rng.uniform(np.log(1.3), np.log(w_max), C))
    f0 = rng.uniform(0.2 * top, 0.8 * top, C)
    A = 10.0 ** np.linspace(-6, 3, C)[rng.permutation(C)]
    c = A * rng.uniform(0.01, 0.05, C)
    if F >= 256:
        f0[0], w[0] = 28.0, 4.4                       # 4 bins each side above half: h0 = 4.5, n = 36, window [1, 65)
    if F == 8192:
        f0[0], w[0] = 2048.0, 300.0
        f0[1], w[1] = 1000.3, 3.7                    # 2 * 30 + 1 = 61 bins
        f0[2], w[2] = 3000.6, 12.2                   # 2 * 100 + 1 bins
    mirror = np.where(f0 < 0.5 * top, f0 + 0.35 * top, f0 - 0.35 * top)
    if F == 8192:
        mirror[0] = -1e9                              # the cap case keeps one peak: a second one would sit inside its window
    phi = lorentzian(i, f0, w, A) + lorentzian(i, mirror, 1.5 * w, mirror_height * A) + c
    return np.ascontiguousarray(phi.astype(np.float32)), np.stack([f0, w, A, c], axis=1)


def noisy_case(F, C, segments=64, seed=0):
    """clean_case with the chi-square noise of an average over `segments` periodograms: every bin times a gamma variate of
    shape `segments` and mean 1"""
    phi, truth = clean_case(F, C, seed)
    rng = np.random.default_rng(77 + seed)
    return np.ascontiguousarray((phi * rng.gamma(segments, 1.0 / segments, phi.shape)).astype(np.float32)), truth


def ringdown(T, bin0, hwhm_bins):
    """(T,) float64 power spectrum |FFT / T|^2 of the complex ring-down exp(-Gamma t + i omega0 t), Gamma = 2 pi hwhm / T,
    omega0 = 2 pi bin0 / T per frame: a Lorentzian of half width hwhm_bins bins at bin0 (up to the aliasing of its tails)"""
    t = np.arange(T)
    z = np.exp((-2 * np.pi * hwhm_bins / T + 2j * np.pi * bin0 / T) * t)
    return np.abs(np.fft.fft(z) / T) ** 2
