// psa_sed_modes: the mode-projected SED (definition: include/psa_hip.h; kernel: modes.hip).  Per block of k-vectors the
// B site groups are projected with the machinery of psa_sed_project -- plane cache, weights, displacement mode and the
// low-rank k-path route apply per group as they do there -- into one stacked buffer (B, kb, 3, T), transformed by one
// batched rocFFT and contracted with the mode vectors in the pass that takes the modulus.  The contraction comes
// after the FFT on purpose: 3 B transforms per k-vector whatever M, no complex (K, M, T) array, and the modulus fused.
// Nothing of the SED entry points' result state is touched.  The pieces of a call -- checks and coefficient table, uploads
// and group sources, the block rule, the B projections of a block -- are shared with the segment average
// (api_modes_welch.hip).
#include "api_internal.h"

namespace psa {

// conj(eig) of k-vectors [0, K) as the kernel reads it: [k][pass][n = 3b + c][MT], zero beyond M
int pack_coef(const float* eig, int64_t K, int64_t M, int64_t B, int MT, std::vector<float>* coef) {
    const int64_t n3 = 3 * B, n_pass = (M + MT - 1) / MT;
    coef->assign((size_t)K * (size_t)n_pass * (size_t)n3 * (size_t)MT * 2, 0.f);
    for (int64_t k = 0; k < K; ++k)
        for (int64_t m = 0; m < M; ++m)
            for (int64_t n = 0; n < n3; ++n) {
                const float* e = eig + ((k * M + m) * n3 + n) * 2;
                PSA_REQUIRE(std::isfinite(e[0]) && std::isfinite(e[1]),
                            "eig[k=%lld, mode %lld, group %lld, component %lld] is not finite", (long long)k, (long long)m,
                            (long long)(n / 3), (long long)(n % 3));
                float* o = coef->data() + ((((size_t)k * n_pass + m / MT) * n3 + n) * MT + m % MT) * 2;
                o[0] = e[0];
                o[1] = -e[1];
            }
    return PSA_OK;
}

int modes_check(psa_ctx* c, const char* what, int slot_in, const float* mean_pos_all, const float* k_vectors, int64_t K,
                const int32_t* group_idx, const int64_t* group_off, int32_t B, const float* eig, int64_t M, int32_t flags,
                bool need_out, ModesCall* m) {
    PSA_TRY(check_slot(c, slot_in));
    const int64_t T = c->slot[slot_in].T, N = c->slot[slot_in].N;
    PSA_REQUIRE((flags & ~PSA_F_DISPLACEMENTS) == 0, "%s takes PSA_F_DISPLACEMENTS or 0, got flags 0x%x", what, (unsigned)flags);
    PSA_REQUIRE(eig != nullptr, "null eig");
    PSA_REQUIRE(!need_out, "null output");
    PSA_REQUIRE(mean_pos_all != nullptr, "null mean_pos_all");
    PSA_REQUIRE(M >= 1 && M < (1ll << 30), "need at least one mode vector per k-point (M = %lld)", (long long)M);
    PSA_REQUIRE(K >= 0 && K < (1ll << 29), "bad number of k-vectors %lld", (long long)K);
    PSA_REQUIRE(K == 0 || k_vectors != nullptr, "null k_vectors");
    PSA_TRY(validate_groups(N, group_idx, group_off, B));
    PSA_TRY(check_weights(c, N));
    if (group_idx) {
        std::vector<uint8_t> seen((size_t)N, 0);
        for (int32_t b = 0; b < B; ++b)
            for (int64_t i = group_off[b]; i < group_off[b + 1]; ++i) {
                PSA_REQUIRE(!seen[group_idx[i]], "atom %d is listed twice (group %d): the site groups of a mode projection must be disjoint",
                            (int)group_idx[i], (int)b);
                seen[group_idx[i]] = 1;
            }
    }
    m->MT = modes_tile(M);
    PSA_TRY(pack_coef(eig, K, M, B, m->MT, &m->coef));
    m->coef_k = (size_t)((M + m->MT - 1) / m->MT) * 3 * (size_t)B * (size_t)m->MT;
    m->per_k = (int64_t)B * 3 * T * (int64_t)sizeof(float2);
    int64_t n_max = 0;
    for (int32_t b = 0; b < B; ++b) n_max = std::max(n_max, group_idx ? group_off[b + 1] - group_off[b] : N);
    // a block of k-vectors: a group's phase table under 2 GiB (as project_groups), the contraction's grid
    m->kb_max = std::min<int64_t>(std::max<int64_t>(64, (((int64_t)2 << 30) / (8 * ((n_max + 63) / 64 * 64 + 64))) / 64 * 64),
                                  (int64_t)65535 * 4);
    m->T = T, m->N = N, m->K = K, m->M = M, m->B = B;
    m->list = ProjectArgs{slot_in, mean_pos_all, k_vectors, K, K, 0, group_idx, group_off, B, flags};
    return PSA_OK;
}

int modes_upload(psa_ctx* c, ModesCall* m) {
    const ProjectArgs& a = m->list;
    {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_kvec, a.k_vectors, (size_t)m->K * 3 * sizeof(float)));
        PSA_TRY(upload(c, c->d_mean_all, a.mean_pos_all, (size_t)m->N * 3 * sizeof(float)));
        if (a.group_idx) PSA_TRY(upload(c, c->d_idx, a.group_idx, (size_t)a.group_off[m->B] * sizeof(int32_t)));
        PSA_TRY(upload(c, c->d_modes_coef, m->coef.data(), m->coef.size() * sizeof(float)));
    }
    // where each group's data comes from (its cached planes, the float32 slot, the displacement array)
    c->plane_call_mark = c->plane_tick + 1;
    m->src.assign((size_t)m->B, GroupView{a.slot, (a.flags & PSA_F_DISPLACEMENTS) != 0});
    for (int32_t b = 0; b < m->B; ++b) {
        GroupView& v = m->src[(size_t)b];
        set_group(c, a.group_idx, a.group_off, b, m->N, &v);
        if (v.n_g) PSA_TRY(group_source(c, &v, a.mean_pos_all, m->K));
    }
    return PSA_OK;
}

int64_t modes_block(const psa_ctx* c, const ModesCall& m, int64_t k0, int64_t kb) {
    int64_t nk = std::min(kb, m.K - k0);
    // a k-path keeps the low-rank route where the budget allows: no tail shorter than PSA_OPT_K1_LOWRANK_MIN_LOCAL
    const int64_t lr_min = c->opt_k1_lowrank_min_local, rest = m.K - k0 - nk;
    if (rest > 0 && rest < lr_min && nk - (lr_min - rest) >= lr_min) nk -= lr_min - rest;
    return nk;
}

int modes_project(psa_ctx* c, const ModesCall& m, int64_t k0, int64_t nk, float2* d_work) {
    for (int32_t b = 0; b < m.B; ++b) {
        const GroupView& v = m.src[(size_t)b];
        float2*          d_q = d_work + (size_t)b * (size_t)nk * 3 * (size_t)m.T;
        if (v.n_g == 0) {                                     // an empty group contributes nothing
            PSA_HIP_CHECK(hipMemsetAsync(d_q, 0, (size_t)nk * 3 * (size_t)m.T * sizeof(float2), c->stream));
            continue;
        }
        PSA_TRY(project_block(c, v, &m.list, k0, nk, d_q));
    }
    return PSA_OK;
}

int modes_run(psa_ctx* c, int slot_in, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
              const int64_t* group_off, int32_t B, const float* eig, int64_t M, int32_t flags, float* out_host, size_t out_bytes,
              bool device_only) {
    ModesCall m;
    PSA_TRY(modes_check(c, "psa_sed_modes", slot_in, mean_pos_all, k_vectors, K, group_idx, group_off, B, eig, M, flags,
                        !out_host && !device_only, &m));
    const int64_t T = m.T;
    PSA_REQUIRE(c->seg_L == 0, "psa_sed_modes has no segment average: clear psa_set_segments first (length %lld is set)",
                (long long)c->seg_L);
    const size_t want = (size_t)T * (size_t)K * (size_t)M * sizeof(float);
    PSA_REQUIRE(out_bytes == want || !out_host, "out_bytes is %zu, the (%lld,%lld,%lld) float32 result has %zu", out_bytes, (long long)T,
                (long long)K, (long long)M, want);
    if (K == 0) return PSA_OK;

    // blocks of k-vectors: the stacked buffer within the budget
    int64_t kb = c->opt_modes_work_bytes / m.per_k;
    PSA_REQUIRE(kb >= 1, "the work budget of %lld bytes (PSA_OPT_MODES_WORK_BYTES) cannot hold one k-vector: %d groups x 3 "
                "components x %lld frames need %lld bytes", (long long)c->opt_modes_work_bytes, (int)B, (long long)T, (long long)m.per_k);
    kb = std::min<int64_t>({kb, K, m.kb_max});
    PSA_TRY(modes_upload(c, &m));
    PSA_TRY(c->d_modes_work.reserve((size_t)kb * (size_t)m.per_k));
    PSA_TRY(c->d_modes_out.reserve(want));

    float2* d_work = c->d_modes_work.as<float2>();
    for (int64_t k0 = 0; k0 < K;) {
        const int64_t nk = modes_block(c, m, k0, kb);
        PSA_TRY(modes_project(c, m, k0, nk, d_work));
        {
            StageTimer st(c, PSA_T_FFT);
            PSA_TRY(run_fft(c, d_work, T, 3 * (int64_t)B * nk));
        }
        {
            StageTimer st(c, PSA_T_EPILOGUE);
            PSA_TRY(launch_mode_power(c, d_work, c->d_modes_coef.as<float2>() + (size_t)k0 * m.coef_k, c->d_modes_out.as<float>(), T, nk,
                                      B, M, m.MT, K, k0, (float)(1.0 / ((double)T * (double)T))));
        }
        k0 += nk;
    }
    if (!out_host) return PSA_OK;
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_modes_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

}  // namespace psa

using namespace psa;

extern "C" {

int psa_sed_modes(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                  const int64_t* group_off, int32_t B, const void* eig, int64_t M, int32_t flags, float* out_host,
                  size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard     guard(c);
    const int rc = modes_run(c, slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, (const float*)eig, M, flags, out_host,
                             out_bytes, false);
    // the caller's arrays are only read during the call, whichever way it ends
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == PSA_OK) {
        set_error("hipStreamSynchronize failed after psa_sed_modes");
        return PSA_EHIP;
    }
    return rc;
}

int psa_debug_mode_power(psa_ctx* c, const void* S_host, const void* eig, int32_t B, int64_t K, int64_t M, int64_t T,
                         float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_REQUIRE(S_host && eig && out_host && B >= 1 && K >= 1 && K <= (int64_t)65535 * 4 && M >= 1 && M < (1ll << 30) && T >= 1,
                "bad argument");
    const int          MT = modes_tile(M);
    std::vector<float> coef;
    PSA_TRY(pack_coef((const float*)eig, K, M, B, MT, &coef));
    const size_t out_bytes = (size_t)T * (size_t)K * (size_t)M * sizeof(float);
    PSA_TRY(upload(c, c->d_modes_work, S_host, (size_t)B * (size_t)K * 3 * (size_t)T * sizeof(float2)));
    PSA_TRY(upload(c, c->d_modes_coef, coef.data(), coef.size() * sizeof(float)));
    PSA_TRY(c->d_modes_out.reserve(out_bytes));
    int rc = launch_mode_power(c, c->d_modes_work.as<float2>(), c->d_modes_coef.as<float2>(), c->d_modes_out.as<float>(), T, K, B, M, MT,
                               K, 0, 1.f);
    if (rc == PSA_OK && hipMemcpyAsync(out_host, c->d_modes_out.ptr, out_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        set_error("copy of the mode powers failed");
        rc = PSA_EHIP;
    }
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));     // the caller's arrays are only read during the call
    return rc;
}

}  // extern "C"
