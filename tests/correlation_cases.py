"""Inputs, bars and a NumPy float32 twin of the time-correlation route (psa_amd/csrc/correlation.hip,
api_correlation.hip), for the host tests and the GPU tests.  Nothing here calls the library, and no bar comes from what the
code under test gives.

The bars
  back-transform alone, per element, against the float64 sum of the same (already rounded) input X:
      |out - F64| <= gamma_64(P + 3) (1/P) sum_o |X[f,o,col]| / (n_seg (L - t)) + 2^-24 |F64|
      gamma_64(n) = n 2^-53 / (1 - n 2^-53)
    an operation count: the kernel's sum is one chain of P float64 FMAs (P roundings); the table entry is the float64
    nearest to the cosine (1); factor[t] = 1 / (P n_seg (L - t)) is one division of exact integers (1); the product
    factor[t] sum (1); the entry passes no column scale.  Then one rounding to float32.
  end to end, per column and field, against tests/correlation64:
      |F - F64| <= 1e-5 F64[0] L / (L - t)
    1e-5 is the project's parity bar for a spectrum, relative to its largest value; here the errors of the float32
    projection, FFT and power are relative to the lag-0 SUM C[0] = n_seg L F[0], and dividing C[t] by the origins
    n_seg (L - t) instead of n_seg L multiplies them by L / (L - t).
  shell form against the per-vector form averaged on the host in float64: 1e-6 F[0] L / (L - t), the spectra's bar for the
    same comparison with the same factor.
"""
import numpy as np

PARITY = 1e-5
SHELL = 1e-6
# (T, L, H, n_lags) of the end-to-end tests: no segments; the last lag down to one origin per segment; an odd L; one lag
SEGMENT_CASES = {"none": (250, 250, 250, 125), "64_32_64": (250, 64, 32, 64), "63_31_40": (250, 63, 31, 40), "64_64_1": (250, 64, 64, 1)}


def gamma64(n):
    u = 2.0 ** -53
    return n * u / (1.0 - n * u)


def padded_length(L, n_lags):
    P = 1
    while P < L + n_lags - 1:
        P *= 2
    return P


def origins(L, n_seg, n_lags):
    return n_seg * (L - np.arange(n_lags, dtype=np.float64))


def end_to_end_bar(F64, L, bar=PARITY):
    """(n_lags, cols): bar F64[0] L / (L - t)"""
    F64 = np.asarray(F64, np.float64)
    t = np.arange(F64.shape[0], dtype=np.float64)
    return bar * np.abs(F64[:1]) * (L / (L - t))[:, None]


def worst_fraction(got, F64, L, bar=PARITY):
    """largest |got - F64| as a fraction of the bar (0 where both the bar and the difference are 0)"""
    lim = end_to_end_bar(F64, L, bar)
    diff = np.abs(np.asarray(got, np.float64) - F64)
    return float(np.max(np.divide(diff, lim, out=np.where(diff > 0, np.inf, 0.0), where=lim > 0)))


# ---- the back-transform alone ---------------------------------------------------------------------------------------
def cos_table(P):
    """cos(2 pi j / P), j < P, as the float64 nearest to it (formed in extended precision where NumPy has it)"""
    pi = np.longdouble(np.pi) + np.longdouble(1.2246467991473532e-16)      # pi to the precision longdouble has
    tab = np.cos(2 * pi * np.arange(P, dtype=np.longdouble) / P)
    tab[0] = 1
    if P % 2 == 0:
        tab[P // 2] = -1
    if P % 4 == 0:
        tab[P // 4] = tab[3 * P // 4] = 0
    return tab


def transform64(X, L, n_seg, n_lags, exact=None):
    """(fields, n_lags, cols) float64: 1 / (P n_seg (L - t)) sum_o X[f,o,col] cos(2 pi (o t mod P) / P) of X
    (fields, P, cols), the index reduced in integers; summed in extended precision where the problem is small (`exact`
    None: up to 4e6 products), else by float64 matrix products"""
    X = np.asarray(X, np.float64)
    fields, P, cols = X.shape
    idx = (np.arange(n_lags, dtype=np.int64)[:, None] * np.arange(P, dtype=np.int64)[None, :]) % P
    tab = cos_table(P)
    exact = n_lags * P * cols * fields <= 4_000_000 if exact is None else exact
    M = tab[idx] if exact else tab.astype(np.float64)[idx]
    Xw = X.astype(np.longdouble) if exact else X
    out = np.stack([M @ Xw[f] for f in range(fields)])
    return np.asarray(out / (P * origins(L, n_seg, n_lags))[None, :, None], np.float64)


def transform_bar(X, L, n_seg, n_lags, F64):
    """the per-element bar of the back-transform alone (the header's first formula)"""
    X = np.asarray(X, np.float64)
    P = X.shape[1]
    mass = np.abs(X).sum(axis=1) / P                                        # (fields, cols)
    return gamma64(P + 3) * mass[:, None, :] / origins(L, n_seg, n_lags)[None, :, None] + 2.0 ** -24 * np.abs(F64)


def single_line(o0, P, n_lags, fault=None):
    """the back-transform of X = 1 at o0, 0 elsewhere (L = n_lags, n_seg = 1), before the division by the origins:
    cos(2 pi (o0 t mod P) / P) / P in closed form, float64; fault "mul32": o0 t reduced in 32 bits first"""
    prod = np.arange(n_lags, dtype=np.int64) * int(o0)
    if fault == "mul32":
        prod = prod & 0xFFFFFFFF
    return np.asarray(cos_table(P)[prod % P], np.float64) / P


# ---- a float32 twin of the route, with the faults a wrong implementation could have ------------------------------------
FAULTS = ("short_pad", "biased", "stale_tail", "sine", "mul32", "hop", "half_mirror", "taper")


def twin(x, L, H, n_lags, fault=None, P=None):
    """(rows, n_lags) float32 of series x (rows, T) complex64 by the route under test: segments zero-padded to P, a
    float32 FFT, |A|^2 in float32 summed over the segments in float64, the cosine back-transform with the index advanced
    modulo P, 1 / (P n_seg (L - t)) in float64, one rounding.  `fault`: one of FAULTS planted ("mul32" shows only where P is no power of two and o t passes 2^32: `single_line`)."""
    x = np.asarray(x, np.complex64)
    T = x.shape[-1]
    n_seg = 1 + (T - L) // H
    if P is None:
        P = padded_length(L, 1 if fault == "short_pad" else n_lags)
    win = np.ones(L, np.float32)
    if fault == "taper":
        win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(L) / L)).astype(np.float32)
    X = np.zeros(x.shape[:-1] + (P,), np.float64)
    stale = np.zeros(x.shape[:-1] + (P - L,), np.complex64)
    for s in range(n_seg):
        start = s * (H - 1 if fault == "hop" else H)                       # (a hop off by one)
        seg = np.zeros(x.shape[:-1] + (P,), np.complex64)
        seg[..., :L] = win * x[..., start:start + L]
        if fault == "stale_tail":
            seg[..., L:] = stale                                            # what the previous block's FFT left there
        A = np.fft.fft(seg, axis=-1).astype(np.complex64)
        stale = A[..., L:]
        X += (A.real * A.real + A.imag * A.imag).astype(np.float64)
    t = np.arange(n_lags, dtype=np.int64)[:, None]
    o = np.arange(P, dtype=np.int64)[None, :]
    ang = 2 * np.pi * ((t * o) % P).astype(np.float64) / P
    M = np.sin(ang) if fault == "sine" else np.cos(ang)
    div = n_seg * float(L) * np.ones(n_lags) if fault == "biased" else origins(L, n_seg, n_lags)
    scale = 0.5 if fault == "half_mirror" else 1.0                          # 1 / (2 n_half) on sums of one side only
    return (scale * (X @ M.T) / (P * div)).astype(np.float32)
