// psa_sed_covariance: the spectral covariance of the B site groups' projections (definition: include/psa_hip.h; kernel:
// covariance.hip).  Per block of kb k-vectors the B groups are projected and transformed exactly as psa_sed_modes does
// without segments -- its own checks of the k-list and the groups, uploads, block rule and projections (api_modes.hip):
// plane cache, weights, displacement mode and the low-rank k-path route apply per group -- into the stacked buffer
// (B, kb, 3, T), and reduced over frequency by the two covariance kernels into the block's rows of the
// (n_w, K, 3B, 3B) complex128 result.
// Budget (PSA_OPT_MODES_WORK_BYTES = W): a k-vector costs its 24 B T bytes of q and its partial slabs
// (covariance_slab_floats: two slots per 4096 frequencies, at configuration 3 1.5 % of q), so kb = W / (both); the weight table
// and the result are outside.
#include "api_internal.h"

namespace psa {

namespace {

int check_freq_weights(const float* g, int32_t n_w, int64_t T) {
    PSA_REQUIRE(n_w >= 1 && n_w <= 2, "the spectral covariance takes 1 or 2 rows of frequency weights, got n_w = %d", (int)n_w);
    PSA_REQUIRE(g != nullptr, "null freq_weights");
    for (int64_t i = 0; i < (int64_t)n_w * T; ++i)
        PSA_REQUIRE(std::isfinite(g[i]), "freq_weights[%lld, %lld] is not finite", (long long)(i / T), (long long)(i % T));
    return PSA_OK;
}

int covariance_run(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                   const int64_t* group_off, int32_t B, const float* g, int32_t n_w, int32_t flags, double* out, size_t out_bytes) {
    PSA_TRY(check_slot(c, slot));
    PSA_REQUIRE((flags & ~PSA_F_DISPLACEMENTS) == 0, "psa_sed_covariance takes PSA_F_DISPLACEMENTS or 0, got flags 0x%x", (unsigned)flags);
    PSA_REQUIRE(out != nullptr, "null output");
    PSA_REQUIRE(mean_pos_all != nullptr, "null mean_pos_all");
    ModesCall m;
    PSA_TRY(modes_check_groups(c, slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, flags, &m));
    PSA_REQUIRE(3 * (int64_t)B <= 96, "the spectral covariance serves 3 B <= 96 rows (B = %d site groups give %lld)", (int)B,
                (long long)(3 * (int64_t)B));
    const int64_t T = m.T, n = 3 * (int64_t)B;
    PSA_TRY(check_freq_weights(g, n_w, T));
    PSA_REQUIRE(c->seg_L == 0, "psa_sed_covariance has no segment average: clear psa_set_segments first (length %lld is set)",
                (long long)c->seg_L);
    const size_t want = (size_t)n_w * (size_t)K * (size_t)(n * n) * sizeof(double2);
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%d,%lld,%lld,%lld) complex128 result has %zu", out_bytes, (int)n_w,
                (long long)K, (long long)n, (long long)n, want);
    if (K == 0) return PSA_OK;

    const int64_t slab_k = covariance_slab_floats(T, n, n_w) * (int64_t)sizeof(float), W = c->opt_modes_work_bytes;
    PSA_REQUIRE(W >= m.per_k + slab_k, "the work budget of %lld bytes (PSA_OPT_MODES_WORK_BYTES) cannot hold one k-vector: %d groups x 3 "
                "components x %lld frames and their partial sums need %lld bytes", (long long)W, (int)B, (long long)T,
                (long long)(m.per_k + slab_k));
    const int64_t kb = std::min<int64_t>({W / (m.per_k + slab_k), K, m.kb_max, ((1ll << 31) - 1) / covariance_chunks(T)});
    PSA_TRY(modes_upload(c, &m));
    {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_cov_g, g, (size_t)n_w * (size_t)T * sizeof(float)));
    }
    PSA_TRY(c->d_modes_work.reserve((size_t)kb * (size_t)m.per_k));
    PSA_TRY(c->d_cov_slab.reserve((size_t)kb * (size_t)slab_k));
    PSA_TRY(c->d_cov_out.reserve(want));

    float2*      d_work = c->d_modes_work.as<float2>();
    const double scale = 1.0 / ((double)T * (double)T);
    for (int64_t k0 = 0; k0 < K;) {
        const int64_t nk = modes_block(c, m, k0, kb);
        PSA_TRY(modes_project(c, m, k0, nk, d_work));
        {
            StageTimer st(c, PSA_T_FFT);
            PSA_TRY(run_fft(c, d_work, T, 3 * (int64_t)B * nk));
        }
        StageTimer st(c, PSA_T_EPILOGUE);
        PSA_TRY(launch_covariance(c, d_work, c->d_cov_g.as<float>(), c->d_cov_slab.as<float>(), c->d_cov_out.as<double2>(), T, nk, B, n_w, K,
                                  k0, scale));
        k0 += nk;
    }
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out, c->d_cov_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the two covariance kernels alone on spectra S_host (B, K, 3, T) the caller uploads, used as given
int debug_covariance(psa_ctx* c, const void* S_host, int32_t B, int64_t K, int64_t T, const float* g, int32_t n_w, double scale,
                     double* out_host) {
    const int64_t n = 3 * (int64_t)B;
    const size_t  want = (size_t)n_w * (size_t)K * (size_t)(n * n) * sizeof(double2);
    PSA_TRY(upload(c, c->d_modes_work, S_host, (size_t)B * (size_t)K * 3 * (size_t)T * sizeof(float2)));
    PSA_TRY(upload(c, c->d_cov_g, g, (size_t)n_w * (size_t)T * sizeof(float)));
    PSA_TRY(c->d_cov_slab.reserve((size_t)K * (size_t)covariance_slab_floats(T, n, n_w) * sizeof(float)));
    PSA_TRY(c->d_cov_out.reserve(want));
    PSA_TRY(launch_covariance(c, c->d_modes_work.as<float2>(), c->d_cov_g.as<float>(), c->d_cov_slab.as<float>(),
                              c->d_cov_out.as<double2>(), T, K, B, n_w, K, 0, scale));
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_cov_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_sed_covariance(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                       const int64_t* group_off, int32_t B, const float* freq_weights, int32_t n_w, int32_t flags, double* out_host,
                       size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, covariance_run(c, slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, freq_weights, n_w, flags, out_host,
                                          out_bytes),
                        "psa_sed_covariance");
}

int psa_debug_covariance(psa_ctx* c, const void* S_host, int32_t B, int64_t K, int64_t T, const float* freq_weights, int32_t n_w,
                         double scale, double* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_REQUIRE(S_host && freq_weights && out_host, "null spectra, freq_weights or output");
    PSA_REQUIRE(B >= 1 && 3 * (int64_t)B <= 96, "the spectral covariance serves 1 <= B and 3 B <= 96 rows, got B = %d", (int)B);
    PSA_REQUIRE(K >= 1 && K <= (int64_t)65535 * 4, "bad number of k-vectors %lld", (long long)K);
    PSA_REQUIRE(T >= 1 && T <= (1ll << 31) - 64, "bad number of frequencies %lld (1 .. 2^31 - 64)", (long long)T);
    PSA_REQUIRE(n_w >= 1 && n_w <= 2, "the spectral covariance takes 1 or 2 rows of frequency weights, got n_w = %d", (int)n_w);
    PSA_REQUIRE(std::isfinite(scale), "scale is not finite");
    return synchronised(c, debug_covariance(c, S_host, B, K, T, freq_weights, n_w, scale, out_host), "psa_debug_covariance");
}

}  // extern "C"
