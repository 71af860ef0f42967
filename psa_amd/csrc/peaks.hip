// Lorentzian peak fits of spectrum columns (psa_fit_peaks, psa_sed_modes_fit; definition: include/psa_hip.h, host side:
// api_peaks.hip, float64 restatement: tests/fit64.py).  A spectrum is (F, C) float32, column j has the band
// [lo_j, hi_j) of FFT bins inside the positive half.
//
// peak_find_kernel: one thread per column (a wavefront reads 256 contiguous bytes of a row), the rows that any band
// covers split into gridDim.y slices.  A slice leaves (largest value, its lowest bin, "a non-finite value in the band")
// per column; rows ascend and only a strictly larger value replaces the best, so a tie keeps the lowest bin whatever
// the split.
//
// peak_fit_kernel: one wavefront per column, four columns per workgroup.  The wavefront folds the slices' partials
// (one lane per slice; larger value, then lower bin), walks down and up from the peak bin p in chunks of 64 bins to
// the first bin below half the maximum (__ballot, first cleared bit), derives the window [a, b) of at most 4095 bins,
// stages it once from its C-strided column into its 16 KiB of LDS, and runs Levenberg-Marquardt on chip in the units
// x = (i - p) / h0, y = phi[i] / phi[p]: lanes stride over the window, the 10 + 4 + 1 sums of the normal equations are
// float64 and folded by an xor butterfly (a fixed order: two calls give the same bits, and every lane ends with the
// same value), the scaled 4 x 4 system is solved by every lane alike.  No atomics, nothing shared between wavefronts.
#include <algorithm>
#include <climits>
#include <cmath>

#include "psa_ctx.h"

namespace psa {

constexpr int PEAKS_FIND_COLS = 256;    // columns per peak_find workgroup: one per thread
constexpr int PEAKS_MAX_SLICES = 64;    // row slices of peak_find: one lane each in peak_fit's fold
constexpr int PEAKS_FIT_COLS = 4;       // columns per peak_fit workgroup: one per wavefront
constexpr int PEAKS_WIN = 4096;         // floats of LDS per wavefront; a window has at most 2 * 2047 + 1 bins
constexpr int PEAKS_N_MIN = 4, PEAKS_N_MAX = 2047;
constexpr int PEAKS_MIN_BAND = 5;       // a band of fewer bins is not fitted

__global__ void __launch_bounds__(PEAKS_FIND_COLS)
peak_find_kernel(const float* __restrict__ spec, int64_t C, const int32_t* __restrict__ bands, int lo_all, int hi_all,
                 int row0, int rows_per_slice, int row_end, float* __restrict__ pmax, int* __restrict__ pidx,
                 int* __restrict__ pflag) {
    const int64_t col = (int64_t)blockIdx.x * PEAKS_FIND_COLS + threadIdx.x;
    if (col >= C) return;
    const int lo = bands ? bands[2 * col] : lo_all, hi = bands ? bands[2 * col + 1] : hi_all;
    const int s0 = row0 + (int)blockIdx.y * rows_per_slice;
    const int r0 = max(lo, s0), r1 = min(hi, min(row_end, s0 + rows_per_slice));
    float     best = -INFINITY;
    int       best_i = INT_MAX, bad = 0;
    const float* p = spec + (int64_t)r0 * C + col;
    int          r = r0;
    for (; r + 4 <= r1; r += 4, p += 4 * C) {                  // four independent loads in flight per thread
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[(int64_t)j * C];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bad |= !isfinite(v[j]);
            if (v[j] > best) best = v[j], best_i = r + j;
        }
    }
    for (; r < r1; ++r, p += C) {
        const float v = *p;
        bad |= !isfinite(v);
        if (v > best) best = v, best_i = r;
    }
    const int64_t o = (int64_t)blockIdx.y * C + col;
    pmax[o] = best;
    pidx[o] = best_i;
    pflag[o] = bad;
}

namespace {

struct Sums {          // normal equations of one parameter point: J^T J (upper triangle), J^T r, r^T r
    double n00, n01, n02, n03, n11, n12, n13, n22, n23, n33, g0, g1, g2, g3, rss;
};

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// the sums at (f0, w, A, c) over the staged window: model A w^2 / ((x - f0)^2 + w^2) + c, x = (i - i_peak) / h0
__device__ inline Sums window_sums(const float* win, int n_win, int i_peak, double inv_h0, double inv_peak, double f0, double w,
                                   double A, double c, int lane) {
    Sums         s = {};
    const double w2 = w * w;
    for (int i = lane; i < n_win; i += 64) {
        const double x = (double)(i - i_peak) * inv_h0, y = (double)win[i] * inv_peak;
        const double d = x - f0, inv_D = 1.0 / (d * d + w2), L = w2 * inv_D;
        const double r = y - (A * L + c);
        const double t = 2.0 * A * L * inv_D;            // common factor of the two shape derivatives
        const double j0 = t * d, j1 = t * d * d / w, j2 = L;
        s.n00 += j0 * j0, s.n01 += j0 * j1, s.n02 += j0 * j2, s.n03 += j0;
        s.n11 += j1 * j1, s.n12 += j1 * j2, s.n13 += j1;
        s.n22 += j2 * j2, s.n23 += j2, s.n33 += 1.0;
        s.g0 += j0 * r, s.g1 += j1 * r, s.g2 += j2 * r, s.g3 += r;
        s.rss += r * r;
    }
    s.n00 = wave_sum(s.n00), s.n01 = wave_sum(s.n01), s.n02 = wave_sum(s.n02), s.n03 = wave_sum(s.n03);
    s.n11 = wave_sum(s.n11), s.n12 = wave_sum(s.n12), s.n13 = wave_sum(s.n13);
    s.n22 = wave_sum(s.n22), s.n23 = wave_sum(s.n23), s.n33 = wave_sum(s.n33);
    s.g0 = wave_sum(s.g0), s.g1 = wave_sum(s.g1), s.g2 = wave_sum(s.g2), s.g3 = wave_sum(s.g3);
    s.rss = wave_sum(s.rss);
    return s;
}

// (N + lambda diag N) delta = g with Marquardt's scaling: M = S N S, S = diag(N)^-1/2 (1 where the diagonal is not
// positive: that parameter has no influence and does not move), Cholesky of M + lambda I.  false: not positive definite
__device__ inline bool lm_step(const Sums& s, double lambda, double* d0, double* d1, double* d2, double* d3) {
    const double s0 = s.n00 > 0.0 ? 1.0 / sqrt(s.n00) : 1.0, s1 = s.n11 > 0.0 ? 1.0 / sqrt(s.n11) : 1.0;
    const double s2 = s.n22 > 0.0 ? 1.0 / sqrt(s.n22) : 1.0, s3 = s.n33 > 0.0 ? 1.0 / sqrt(s.n33) : 1.0;
    const double m00 = 1.0 + lambda, m11 = m00, m22 = m00, m33 = m00;
    const double m01 = s.n01 * s0 * s1, m02 = s.n02 * s0 * s2, m03 = s.n03 * s0 * s3;
    const double m12 = s.n12 * s1 * s2, m13 = s.n13 * s1 * s3, m23 = s.n23 * s2 * s3;
    const double b0 = s.g0 * s0, b1 = s.g1 * s1, b2 = s.g2 * s2, b3 = s.g3 * s3;
    // Cholesky M = L L^T
    if (!(m00 > 0.0)) return false;
    const double l00 = sqrt(m00), l10 = m01 / l00, l20 = m02 / l00, l30 = m03 / l00;
    const double p11 = m11 - l10 * l10;
    if (!(p11 > 0.0)) return false;
    const double l11 = sqrt(p11), l21 = (m12 - l20 * l10) / l11, l31 = (m13 - l30 * l10) / l11;
    const double p22 = m22 - l20 * l20 - l21 * l21;
    if (!(p22 > 0.0)) return false;
    const double l22 = sqrt(p22), l32 = (m23 - l30 * l20 - l31 * l21) / l22;
    const double p33 = m33 - l30 * l30 - l31 * l31 - l32 * l32;
    if (!(p33 > 0.0)) return false;
    const double l33 = sqrt(p33);
    const double y0 = b0 / l00, y1 = (b1 - l10 * y0) / l11, y2 = (b2 - l20 * y0 - l21 * y1) / l22;
    const double y3 = (b3 - l30 * y0 - l31 * y1 - l32 * y2) / l33;
    const double z3 = y3 / l33, z2 = (y2 - l32 * z3) / l22, z1 = (y1 - l21 * z2 - l31 * z3) / l11;
    const double z0 = (y0 - l10 * z1 - l20 * z2 - l30 * z3) / l00;
    *d0 = z0 * s0, *d1 = z1 * s1, *d2 = z2 * s2, *d3 = z3 * s3;
    return true;
}

}  // namespace

// spec (F, C); bands (C, 2) or null with [lo_all, hi_all) for every column; the n_slices partials of peak_find;
// fit (C, 6): f0, hwhm (both times df), height, baseline, rss, peak bin; info (C, 4): status, iterations, a, b - a
__global__ void __launch_bounds__(64 * PEAKS_FIT_COLS)
peak_fit_kernel(const float* __restrict__ spec, int64_t C, const int32_t* __restrict__ bands, int lo_all, int hi_all,
                const float* __restrict__ pmax, const int* __restrict__ pidx, const int* __restrict__ pflag, int n_slices,
                double df, float window_hwhm, int half_window_bins, int max_iter, float* __restrict__ fit,
                int32_t* __restrict__ info) {
    __shared__ float win_all[PEAKS_FIT_COLS][PEAKS_WIN];
    const int     lane = threadIdx.x & 63;
    const int     wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t col = (int64_t)blockIdx.x * PEAKS_FIT_COLS + wave;
    float*        win = win_all[wave];
    const bool    present = col < C;

    int   lo = 0, hi = 0, p = 0, a = 0, n_win = 0;
    float peak = 0.f, h0 = 1.f, y_min = 0.f;
    bool  fitted = false;
    if (present) {
        lo = bands ? bands[2 * col] : lo_all, hi = bands ? bands[2 * col + 1] : hi_all;
        // fold the slices: larger value, then lower bin
        float v = lane < n_slices ? pmax[(int64_t)lane * C + col] : -INFINITY;
        int   vi = lane < n_slices ? pidx[(int64_t)lane * C + col] : INT_MAX;
        int   bad = lane < n_slices ? pflag[(int64_t)lane * C + col] : 0;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const float ov = __shfl_xor(v, m);
            const int   oi = __shfl_xor(vi, m);
            bad |= __shfl_xor(bad, m);
            if (ov > v || (ov == v && oi < vi)) v = ov, vi = oi;
        }
        peak = v, p = vi;
        fitted = hi - lo >= PEAKS_MIN_BAND && !bad && peak > 0.f;
    }
    if (fitted) {
        const float half = 0.5f * peak;
        int         l = 0, r = 0;
        for (int base = p - 1;; base -= 64) {                      // down: bins base, base - 1, ...
            const int  i = base - lane;
            const bool in = i >= lo && spec[(int64_t)i * C + col] >= half;
            const unsigned long long stop = ~__ballot(in);
            if (stop) { l += __ffsll((long long)stop) - 1; break; }
            l += 64;
        }
        for (int base = p + 1;; base += 64) {                      // up
            const int  i = base + lane;
            const bool in = i < hi && spec[(int64_t)i * C + col] >= half;
            const unsigned long long stop = ~__ballot(in);
            if (stop) { r += __ffsll((long long)stop) - 1; break; }
            r += 64;
        }
        h0 = fmaxf(1.f, 0.5f * (float)(l + r + 1));
        int n = half_window_bins > 0 ? half_window_bins : (int)fminf(ceilf(window_hwhm * h0), (float)PEAKS_N_MAX);
        n = min(max(n, PEAKS_N_MIN), PEAKS_N_MAX);
        a = max(lo, p - n);
        n_win = min(hi, p + n + 1) - a;
        y_min = INFINITY;
        for (int i = lane; i < n_win; i += 64) {
            const float v = spec[(int64_t)(a + i) * C + col];
            win[i] = v;
            y_min = fminf(y_min, v);
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) y_min = fminf(y_min, __shfl_xor(y_min, m));
    }
    __syncthreads();                                               // the staged windows are visible (all wavefronts arrive)
    if (!present) return;
    float*   f = fit + col * 6;
    int32_t* o = info + col * 4;
    if (!fitted) {
        if (lane < 6) f[lane] = NAN;
        if (lane < 4) o[lane] = lane == 0 ? 2 : 0;
        return;
    }

    const double inv_h0 = 1.0 / (double)h0, inv_peak = 1.0 / (double)peak;
    const int    i_peak = p - a;
    double       c = (double)y_min * inv_peak, A = 1.0 - c, f0 = 0.0, w = 1.0, lambda = 1e-3;
    Sums         s = window_sums(win, n_win, i_peak, inv_h0, inv_peak, f0, w, A, c, lane);
    int          it = 0, status = 1;
    while (it < max_iter) {
        ++it;
        double d0, d1, d2, d3;
        if (!lm_step(s, lambda, &d0, &d1, &d2, &d3) || !(w + d1 > 0.0)) {
            lambda *= 10.0;
            continue;
        }
        const Sums t = window_sums(win, n_win, i_peak, inv_h0, inv_peak, f0 + d0, w + d1, A + d2, c + d3, lane);
        const bool small = fmax(fabs(d0), fabs(d1)) <= 1e-6 * w && fmax(fabs(d2), fabs(d3)) <= 1e-6 * fabs(A);
        if (t.rss <= s.rss * (1.0 + 0x1p-46)) {                    // downhill up to the rounding of the sums
            f0 += d0, w += d1, A += d2, c += d3, s = t;
            lambda = fmax(0.1 * lambda, 1e-12);
        } else {
            lambda *= 10.0;
        }
        if (small) { status = 0; break; }
    }
    const double f0_bin = (double)p + f0 * (double)h0, w_bin = w * (double)h0;
    if (status == 0 && (f0_bin < (double)a || f0_bin >= (double)(a + n_win) || w_bin > (double)n_win)) status = 3;
    if (lane == 0) {
        f[0] = (float)(f0_bin * df);
        f[1] = (float)(w_bin * df);
        f[2] = (float)(A * (double)peak);
        f[3] = (float)(c * (double)peak);
        f[4] = (float)(s.rss * (double)peak * (double)peak);
        f[5] = (float)p;
        o[0] = status, o[1] = it, o[2] = a, o[3] = n_win;
    }
}

int peaks_slices(int64_t C, int64_t rows) {
    const int64_t col_blocks = (C + PEAKS_FIND_COLS - 1) / PEAKS_FIND_COLS;
    int64_t       s = (2048 + col_blocks - 1) / col_blocks;        // about eight workgroups per compute unit
    s = std::min<int64_t>(s, (rows + 15) / 16);                    // ... of at least 16 rows
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, PEAKS_MAX_SLICES));
}

int launch_peak_find(psa_ctx* c, const float* d_spec, int64_t C, const int32_t* d_bands, int lo, int hi, int row0, int row_end,
                     int n_slices, float* d_pmax, int* d_pidx, int* d_pflag) {
    const int64_t gx = (C + PEAKS_FIND_COLS - 1) / PEAKS_FIND_COLS;
    PSA_REQUIRE(C >= 1 && gx < (1ll << 31) && n_slices >= 1 && n_slices <= PEAKS_MAX_SLICES && row0 >= 0 && row_end > row0,
                "peak search: %lld columns, rows [%d, %d) in %d slices is out of range", (long long)C, row0, row_end, n_slices);
    const int rows_per_slice = (row_end - row0 + n_slices - 1) / n_slices;
    hipLaunchKernelGGL(peak_find_kernel, dim3((unsigned)gx, (unsigned)n_slices), dim3(PEAKS_FIND_COLS), 0, c->stream, d_spec, C,
                       d_bands, lo, hi, row0, rows_per_slice, row_end, d_pmax, d_pidx, d_pflag);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_peak_fit(psa_ctx* c, const float* d_spec, int64_t C, const int32_t* d_bands, int lo, int hi, const float* d_pmax,
                    const int* d_pidx, const int* d_pflag, int n_slices, double df, float window_hwhm, int half_window_bins,
                    int max_iter, float* d_fit, int32_t* d_info) {
    const int64_t gx = (C + PEAKS_FIT_COLS - 1) / PEAKS_FIT_COLS;
    PSA_REQUIRE(C >= 1 && gx < (1ll << 31) && n_slices >= 1 && n_slices <= PEAKS_MAX_SLICES && max_iter >= 1,
                "peak fit: %lld columns, %d slices, %d iterations is out of range", (long long)C, n_slices, max_iter);
    hipLaunchKernelGGL(peak_fit_kernel, dim3((unsigned)gx), dim3(64 * PEAKS_FIT_COLS), 0, c->stream, d_spec, C, d_bands, lo, hi,
                       d_pmax, d_pidx, d_pflag, n_slices, df, window_hwhm, half_window_bins, max_iter, d_fit, d_info);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
