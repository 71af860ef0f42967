// Kernels of the time correlations on the reciprocal lattice of the box (psa_lattice_correlations, psa_self_correlations;
// definition: include/psa_hip.h, host side: api_correlation.hip): F(k,t), F_s(k,t), C_L(k,t), C_T(k,t) as the linear,
// unbiased correlation of every segment,
//
//     F[t] = 1/(n_seg (L - t)) Re sum_s sum_{l = 0}^{L-1-t} x[sH + l + t] conj x[sH + l],        t = 0 .. n_lags - 1.
//
// The route is the spectral calls' with two passes added: every segment is zero-padded to P >= L + n_lags - 1 frames before
// the FFT (so lag t never meets lag P - t), the power |A_s[o]|^2 is summed where the spectra sum it (dynamic.hip's power
// pass per vector, lattice.hip's shell pass and self.hip's power pass in float64), and the sum is transformed back,
//
//     C[t] = 1/P sum_o X[o] cos(2 pi o t / P),
//
// which is real because only the part even in t is asked for.
//
//   correlation_pad        rows of q (n_rows, T) -> segments (n_rows, ns, P): the L frames of a segment as bit copies, the
//                          tail [L, P) zero.  COPY = false writes the tails alone: the self part's series kernel has written
//                          the heads with rows of pitch P.  The FFT runs in place, so a block's tail holds transform values
//                          afterwards: the tail is written for EVERY block, by the pass that also decides P - L -- a stale
//                          tail of an earlier block or call cannot be read.  One lane per element, adjacent lanes adjacent
//                          frames: 512 contiguous bytes per wavefront on both sides.
//   correlation_transform  out[f,t,col] = float32(factor[t] scale[col] sum_o X[f,o,col] tab[(o t) mod P]), everything before
//                          the one rounding in float64: tab[j] = cos(2 pi j / P) from the host, factor[t] = 1 / (P n_seg
//                          (L - t)), scale[col] the pass's own (1 / n_half of a shell, or none).  A direct sum: P n_lags
//                          FMAs per column and field, in the order o = 0 .. P - 1 in one lane -- no atomics, no partial
//                          sums, the same bits on every run.  o t reaches 2^33 at real sizes: the table index advances by
//                          t modulo P per step, in 32 bits (P <= 2^30, so index + t < 2^31).
//
// Two layouts of the transform, by the number of columns (the accumulators' layout (fields, P, cols) has adjacent columns
// adjacent):
//   columns form (cols >= CORR_COLS_MIN)   a wavefront per workgroup, a lane per column, CORR_LAGS = 8 lags per lane: one
//       coalesced load of X[o, col .. col + 63] (8 or 4 bytes per lane) feeds eight float64 FMAs.  The eight table indices
//       and the eight table values depend on (o, t) alone, are the same for all lanes and live in scalar registers: the
//       table is read by scalar loads, and the vector unit does the FMAs and the one load.  At 5197 vectors x 3 fields,
//       P = 2048, n_lags = 512 (the per-vector form: float32 power, 128 MB) this is 1.6e10 FMAs -- 0.4 ms at the device's
//       published 78.6 TFLOP/s of vector float64 -- and P n_lags / 8 cols 4 B = 8 GB of loads, most of which hit the L2:
//       the 64 lag tiles of a column tile run side by side over the same 2048 rows of 256 B.  Measured 4.5 ms, 1.4 % of
//       the call.
//   lags form (cols < CORR_COLS_MIN)       a lane per lag, blockIdx.y the column: X[o, col] is wave-uniform (a scalar load),
//       the table entry is a gather of 8 bytes per lane from a table of 8 P bytes (64 KiB at P = 8192: it stays in the
//       caches; no LDS copy is made -- at P = 65536 its 512 KiB would not fit the 160 KiB of a compute unit, and the gather
//       is not the bound at these sizes).
// The bound of an element (tests/correlation_cases.py), an operation count: the chain of P float64 FMAs (P roundings), the
// table entry (the float64 nearest to the cosine: 1), factor[t] (one division of exact integers: 1), the product
// factor[t] sum (1), and with a column scale the product factor[t] scale[col] (1 more):
// gamma_64(P + 3) (1/P) sum_o |X| / (n_seg (L - t)) without a column scale, gamma_64(P + 4) with one; then one float32 rounding.
#include <algorithm>

#include "psa_ctx.h"

namespace psa {

namespace {

template <bool COPY>
__global__ void __launch_bounds__(256)
correlation_pad_kernel(const float2* __restrict__ q, float2* __restrict__ seg, int64_t T, int64_t L, int64_t P, int64_t H, int64_t s0,
                       int ns, int n_lt, int64_t n_rows) {
    const int     s = blockIdx.x / n_lt;
    const int64_t first = COPY ? 0 : L;
    const int64_t l = first + (int64_t)(blockIdx.x - s * n_lt) * 256 + threadIdx.x;
    if (l >= P) return;
    for (int64_t row = blockIdx.y; row < n_rows; row += gridDim.y) {
        float2 v = make_float2(0.f, 0.f);
        if constexpr (COPY)
            if (l < L) v = q[row * T + (s0 + s) * H + l];
        seg[(row * ns + s) * P + l] = v;
    }
}

template <class TIn>
__global__ void __launch_bounds__(64)
correlation_transform_cols_kernel(const TIn* __restrict__ X, const double* __restrict__ tab, const double* __restrict__ factor,
                                  const double* __restrict__ scale, float* __restrict__ out, int P, int64_t cols, int n_lags) {
    const int64_t col = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int     t0 = blockIdx.y * CORR_LAGS, f = blockIdx.z;
    const TIn*    src = X + (int64_t)f * P * cols + min(col, cols - 1);
    int           step[CORR_LAGS], at[CORR_LAGS];
    double        sum[CORR_LAGS];
#pragma unroll
    for (int j = 0; j < CORR_LAGS; ++j) step[j] = min(t0 + j, n_lags - 1), at[j] = 0, sum[j] = 0.0;
    for (int o = 0; o < P; ++o, src += cols) {
        const double x = (double)*src;
#pragma unroll
        for (int j = 0; j < CORR_LAGS; ++j) {
            sum[j] = fma(x, tab[at[j]], sum[j]);
            at[j] += step[j];
            if (at[j] >= P) at[j] -= P;
        }
    }
    if (col >= cols) return;
    const double sc = scale ? scale[col] : 1.0;
#pragma unroll
    for (int j = 0; j < CORR_LAGS; ++j)
        if (t0 + j < n_lags) out[((int64_t)f * n_lags + t0 + j) * cols + col] = (float)(factor[t0 + j] * sc * sum[j]);
}

template <class TIn>
__global__ void __launch_bounds__(256)
correlation_transform_lags_kernel(const TIn* __restrict__ X, const double* __restrict__ tab, const double* __restrict__ factor,
                                  const double* __restrict__ scale, float* __restrict__ out, int P, int64_t cols, int n_lags) {
    const int  t = blockIdx.x * 256 + threadIdx.x, col = blockIdx.y, f = blockIdx.z;
    const int  step = min(t, n_lags - 1);
    const TIn* src = X + (int64_t)f * P * cols + col;
    int        at = 0;
    double     sum = 0.0;
    for (int o = 0; o < P; ++o, src += cols) {
        sum = fma((double)*src, tab[at], sum);
        at += step;
        if (at >= P) at -= P;
    }
    if (t >= n_lags) return;
    const double sc = scale ? scale[col] : 1.0;
    out[((int64_t)f * n_lags + t) * cols + col] = (float)(factor[t] * sc * sum);
}

template <class TIn>
int transform(psa_ctx* c, const TIn* d_X, const double* d_tab, const double* d_factor, const double* d_scale, float* d_out,
              int64_t fields, int64_t P, int64_t cols, int64_t n_lags) {
    PSA_REQUIRE(fields >= 1 && fields <= 3 && P >= 1 && P <= (1ll << 30) && cols >= 1 && n_lags >= 1 && n_lags <= P,
                "correlation transform outside its grid");
    if (cols >= CORR_COLS_MIN) {
        const int64_t gx = (cols + 63) / 64, gy = (n_lags + CORR_LAGS - 1) / CORR_LAGS;
        PSA_REQUIRE(gx < (1ll << 31) && gy <= 65535, "correlation transform outside its grid");
        hipLaunchKernelGGL(correlation_transform_cols_kernel<TIn>, dim3((unsigned)gx, (unsigned)gy, (unsigned)fields), dim3(64), 0,
                           c->stream, d_X, d_tab, d_factor, d_scale, d_out, (int)P, cols, (int)n_lags);
    } else {
        hipLaunchKernelGGL(correlation_transform_lags_kernel<TIn>, dim3((unsigned)((n_lags + 255) / 256), (unsigned)cols, (unsigned)fields),
                           dim3(256), 0, c->stream, d_X, d_tab, d_factor, d_scale, d_out, (int)P, cols, (int)n_lags);
    }
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace

int launch_correlation_pad(psa_ctx* c, const float2* d_q, float2* d_seg, int64_t T, int64_t L, int64_t P, int64_t H, int64_t s0,
                           int64_t ns, int64_t n_rows) {
    if (ns == 0 || n_rows == 0) return PSA_OK;
    PSA_REQUIRE(L >= 1 && P >= L && H >= 1 && s0 >= 0 && (s0 + ns - 1) * H + L <= T, "segment block outside the trajectory");
    const int64_t n_lt = ((d_q ? P : P - L) + 255) / 256;
    if (n_lt == 0) return PSA_OK;                                             // no tail
    PSA_REQUIRE(n_lt * ns < (1ll << 31), "correlation padding outside its grid");
    const dim3 grid((unsigned)(n_lt * ns), (unsigned)std::min<int64_t>(n_rows, 65535)), block(256);
    if (d_q)
        hipLaunchKernelGGL(correlation_pad_kernel<true>, grid, block, 0, c->stream, d_q, d_seg, T, L, P, H, s0, (int)ns, (int)n_lt, n_rows);
    else
        hipLaunchKernelGGL(correlation_pad_kernel<false>, grid, block, 0, c->stream, d_q, d_seg, T, L, P, H, s0, (int)ns, (int)n_lt, n_rows);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_correlation_transform(psa_ctx* c, const double* d_X, const double* d_tab, const double* d_factor, const double* d_scale,
                                 float* d_out, int64_t fields, int64_t P, int64_t cols, int64_t n_lags) {
    return transform(c, d_X, d_tab, d_factor, d_scale, d_out, fields, P, cols, n_lags);
}
int launch_correlation_transform(psa_ctx* c, const float* d_X, const double* d_tab, const double* d_factor, const double* d_scale,
                                 float* d_out, int64_t fields, int64_t P, int64_t cols, int64_t n_lags) {
    return transform(c, d_X, d_tab, d_factor, d_scale, d_out, fields, P, cols, n_lags);
}

}  // namespace psa
