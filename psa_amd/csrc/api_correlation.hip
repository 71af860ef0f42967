// psa_lattice_correlations, psa_self_correlations: the intermediate scattering function F(k,t), its self part F_s(k,t) and
// the current correlations C_L(k,t), C_T(k,t) on the reciprocal lattice of the box, per vector or averaged over shells of
// |k| (definition: include/psa_hip.h; kernels: correlation.hip).  Each is its spectral twin's call -- psa_lattice_spectra
// (api_lattice.hip) through the one run body (api_reciprocal.hip: spectra_run with n_lags set), psa_self_spectra
// (api_self.hip) through the same helpers: the same checks, plan, projection or series kernel, rocFFT and power passes --
// with three differences, of which this file adds the last:
//   the rows    every segment is zero-padded to P = the smallest power of two >= L + n_lags - 1 frames before its FFT
//               (correlation_length); the budget rules count P where the spectra count L;
//   the power   is left unscaled where it is summed: the per-vector pass's float32 (1 or 3, P, K) with the scale 1, the
//               shell pass's and the self pass's float64 accumulators.  The self pass runs without the mirror in the shell
//               form too: the cosine is even, so X[o] and X[(P - o) mod P] give the same C[t], and the half-space members
//               alone give the mean over the full sphere (C_{-n}[t] = conj C_n[t]) -- the column's scale is 1 / n_half;
//   the end     the back-transform into (1 or 3, n_lags, K or n_bins) float32: factor[t] = 1 / (P n_seg (L - t)) and the
//               column's scale in float64, one rounding.  Only n_lags x columns values cross to the host.
// Outside the budget, like the spectra's results: the power (the accumulators of the spectral calls), the tables and the
// result.
#include "api_internal.h"

namespace psa {

namespace {

// the back-transform of the power X (fields, P, cols) where it lies, through the one launch helper: the cosine table and
// the lag factors in float64 from the host, the columns' scales (null: none), the result into d_corr_out
template <class TIn>
int correlation_finish(psa_ctx* c, const TIn* d_X, int64_t fields, int64_t P, int64_t cols, int64_t L, int64_t n_seg, int64_t n_lags,
                       const double* col_scale) {
    // (the argument in extended precision where the host has it, so that every entry is the float64 nearest to the cosine;
    // j = 0, P/4, P/2, 3P/4 are set exactly)
    const long double   two_pi = 6.283185307179586476925286766559L;
    std::vector<double> tab((size_t)P), factor((size_t)n_lags);
    for (int64_t j = 0; j < P; ++j) tab[(size_t)j] = (double)std::cos(two_pi * (long double)j / (long double)P);
    tab[0] = 1.0;
    if (P % 2 == 0) tab[(size_t)(P / 2)] = -1.0;
    if (P % 4 == 0) tab[(size_t)(P / 4)] = tab[(size_t)(3 * P / 4)] = 0.0;
    for (int64_t t = 0; t < n_lags; ++t) factor[(size_t)t] = 1.0 / ((double)P * (double)n_seg * (double)(L - t));
    {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_corr_tab, tab.data(), tab.size() * sizeof(double)));
        PSA_TRY(upload(c, c->d_corr_factor, factor.data(), factor.size() * sizeof(double)));
        if (col_scale) PSA_TRY(upload(c, c->d_corr_scale, col_scale, (size_t)cols * sizeof(double)));
        // (tab and factor are pageable and die with this frame)
        PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    PSA_TRY(c->d_corr_out.reserve((size_t)fields * (size_t)n_lags * (size_t)cols * sizeof(float)));
    StageTimer st(c, PSA_T_PHASE);
    return launch_correlation_transform(c, d_X, c->d_corr_tab.as<double>(), c->d_corr_factor.as<double>(),
                                        col_scale ? c->d_corr_scale.as<double>() : nullptr, c->d_corr_out.as<float>(), fields, P, cols,
                                        n_lags);
}

int correlation_fetch(psa_ctx* c, float* out_host, size_t bytes) {
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_corr_out.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

int lattice_correlations_run(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of,
                             int64_t n_bins, const int32_t* idx, int64_t n_g, int32_t currents, int64_t n_lags, float* out_host,
                             size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    PSA_REQUIRE(n_lags >= 1, "n_lags = %lld: at least one lag (1 <= n_lags <= L)", (long long)n_lags);
    LatCall p;
    PSA_TRY(lattice_check(c, "psa_lattice_correlations", box_inverse, indices, K, bin_of, n_bins, idx, n_g, currents, n_lags, &p));
    const DynCall& d = p.d;
    const int64_t  rows = currents ? 3 : 1, cols = p.shell ? n_bins : K;
    SpectraRun     a;
    a.src = lattice_source(c, p, idx), a.n_bins = p.n_bins, a.out_host = out_host, a.out_bytes = out_bytes;
    a.finish = [&](const float* d_power, const double* d_acc) -> int {
        if (p.shell) {
            // the shell pass adds X_n[o] + X_n[(P - o) mod P] of a bin's n_half vectors: the mean over the full sphere
            std::vector<double> col_scale((size_t)n_bins, 0.0);
            for (int64_t b = 0; b < n_bins; ++b)
                if (p.count[(size_t)b]) col_scale[(size_t)b] = 1.0 / (2.0 * (double)p.count[(size_t)b]);
            PSA_TRY(correlation_finish(c, d_acc, rows, d.P, cols, d.L, d.n_seg, n_lags, col_scale.data()));
        } else {
            PSA_TRY(correlation_finish(c, d_power, rows, d.P, cols, d.L, d.n_seg, n_lags, nullptr));
        }
        return correlation_fetch(c, out_host, out_bytes);
    };
    return spectra_run(c, d, a);
}

int self_correlations_run(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                          const int32_t* idx, int64_t n_g, int64_t n_lags, float* out_host, size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    PSA_REQUIRE(n_lags >= 1, "n_lags = %lld: at least one lag (1 <= n_lags <= L)", (long long)n_lags);
    SelfCall p;
    PSA_TRY(self_check(c, "psa_self_correlations", box_inverse, indices, K, bin_of, n_bins, idx, n_g, true, n_lags, &p));
    const int64_t L = p.d.L, P = p.d.P, cols = p.cols;
    const size_t  want = (size_t)n_lags * (size_t)cols * sizeof(float);
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%lld,%lld) float32 result has %zu", out_bytes, (long long)n_lags,
                (long long)cols, want);
    if (p.d.n_g == 0) {                                      // an empty atom set: zeros
        std::memset(out_host, 0, out_bytes);
        return PSA_OK;
    }
    PSA_TRY(self_upload(c, p, idx, true));
    std::vector<int64_t> vcut;
    SelfPower            w;
    PSA_TRY(self_blocks(c, p, &vcut, &w));
    w.mirror = false, w.finish = false;
    float2* d_work = c->d_rc_work.as<float2>();
    PSA_TRY(self_power_run(c, w, [&](int64_t a0, int64_t na, int64_t vb, int64_t s0, int64_t ns, const float2** where) -> int {
        const int64_t t0 = vb * p.vt, nt = std::min(p.vt, p.n_tiles - t0), nv = vcut[(size_t)vb + 1] - vcut[(size_t)vb];
        PSA_TRY(self_series(c, p, idx, a0, na, t0, nt, s0, ns, d_work));          // the heads, rows of pitch P
        {
            StageTimer st(c, PSA_T_GATHER);
            PSA_TRY(launch_correlation_pad(c, nullptr, d_work, p.d.T, L, P, p.d.H, s0, ns, na * nv));   // the tails
        }
        StageTimer st(c, PSA_T_FFT);
        PSA_TRY(run_fft(c, d_work, P, na * nv * ns));
        *where = d_work;
        return PSA_OK;
    }));
    std::vector<double> col_scale;
    if (p.shell) {                                           // no mirror: the mean over the n_half members
        col_scale.assign((size_t)n_bins, 0.0);
        for (int64_t b = 0; b < n_bins; ++b)
            if (p.count[(size_t)b]) col_scale[(size_t)b] = 1.0 / (double)p.count[(size_t)b];
    }
    PSA_TRY(correlation_finish(c, c->d_rc_acc.as<double>(), 1, P, cols, L, p.d.n_seg, n_lags, p.shell ? col_scale.data() : nullptr));
    return correlation_fetch(c, out_host, want);
}

int correlation_debug_transform(psa_ctx* c, const double* X_host, int64_t fields, int64_t P, int64_t cols, int64_t L, int64_t n_seg,
                                int64_t n_lags, int32_t as_float32, float* out_host) {
    PSA_REQUIRE(X_host != nullptr && out_host != nullptr, "null argument");
    PSA_REQUIRE(fields >= 1 && fields <= 3 && P >= 1 && P <= (1ll << 30) && cols >= 1 && L >= 1 && n_seg >= 1,
                "fields in [1, 3], P in [1, 2^30], cols, L and n_seg positive (%lld, %lld, %lld, %lld, %lld)", (long long)fields,
                (long long)P, (long long)cols, (long long)L, (long long)n_seg);
    PSA_REQUIRE(n_lags >= 1 && n_lags <= L && n_lags <= P, "n_lags = %lld is outside [1, min(L, P) = %lld]", (long long)n_lags,
                (long long)std::min(L, P));
    PSA_REQUIRE(as_float32 == 0 || as_float32 == 1, "as_float32 is 0 or 1, got %d", (int)as_float32);
    const size_t n = (size_t)fields * (size_t)P * (size_t)cols;
    PSA_REQUIRE((double)fields * (double)P * (double)cols < (double)(1ll << 28) && (double)n_lags * (double)cols < (double)(1ll << 28),
                "a power of %lld x %lld x %lld elements is more than this entry serves", (long long)fields, (long long)P, (long long)cols);
    for (size_t i = 0; i < n; ++i) PSA_REQUIRE(std::isfinite(X_host[i]), "X[%zu] is not finite", i);
    if (as_float32) {
        std::vector<float> X32(n);
        for (size_t i = 0; i < n; ++i) X32[i] = (float)X_host[i];
        PSA_TRY(upload(c, c->d_corr_in, X32.data(), n * sizeof(float)));
        PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
        PSA_TRY(correlation_finish(c, c->d_corr_in.as<float>(), fields, P, cols, L, n_seg, n_lags, nullptr));
    } else {
        PSA_TRY(upload(c, c->d_corr_in, X_host, n * sizeof(double)));
        PSA_TRY(correlation_finish(c, c->d_corr_in.as<double>(), fields, P, cols, L, n_seg, n_lags, nullptr));
    }
    return correlation_fetch(c, out_host, (size_t)fields * (size_t)n_lags * (size_t)cols * sizeof(float));
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_lattice_correlations(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of,
                             int64_t n_bins, const int32_t* idx, int64_t n_g, int32_t currents, int64_t n_lags, float* out_host,
                             size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, lattice_correlations_run(c, box_inverse, indices, K, bin_of, n_bins, idx, n_g, currents, n_lags, out_host,
                                                    out_bytes),
                        "psa_lattice_correlations");
}

int psa_self_correlations(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                          const int32_t* idx, int64_t n_g, int64_t n_lags, float* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, self_correlations_run(c, box_inverse, indices, K, bin_of, n_bins, idx, n_g, n_lags, out_host, out_bytes),
                        "psa_self_correlations");
}

int psa_debug_correlation_transform(psa_ctx* c, const double* X_host, int64_t fields, int64_t P, int64_t cols, int64_t L, int64_t n_seg,
                                    int64_t n_lags, int32_t as_float32, float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, correlation_debug_transform(c, X_host, fields, P, cols, L, n_seg, n_lags, as_float32, out_host),
                        "psa_debug_correlation_transform");
}

}  // extern "C"
