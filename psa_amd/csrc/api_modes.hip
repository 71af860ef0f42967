// psa_sed_modes / psa_sed_modes_welch: the mode-projected SED, plain and averaged over Welch segments (definition:
// include/psa_hip.h; kernel: modes.hip).  Per block of kb k-vectors the B site groups are projected with the machinery of
// psa_sed_project -- plane cache, weights, displacement mode and the low-rank k-path route apply per group as they do
// there -- into one stacked buffer q (B, kb, 3, T).  Without segments q is transformed in place by one batched rocFFT and
// contracted with the mode vectors in the pass that takes the modulus: one boxcar segment of T frames, read by the
// contraction as (B, kb, 3, 1, T).  The contraction comes after the FFT on purpose: 3 B transforms per k-vector whatever
// M, no complex (K, M, T) array, and the modulus fused.  With segments q is cut, in sub-blocks of bk k-vectors x bs
// segments, into the segment buffer (B, bk, 3, bs, L) -- one launch_segment_window per group, since the rows of one
// k-vector's B groups lie kb 3 T apart in q --, transformed by one batched length-L rocFFT and contracted; the kernel keeps
// the sum over a sub-block's segments on chip, overwrites the sub-block's columns of the (L, K, M) result with the first
// segments and adds to them with later ones.  Nothing of the SED entry points' result state is touched.
// Budget (PSA_OPT_MODES_WORK_BYTES = W; q and the segment buffer share it, the result is outside): shrinking kb can cost a
// k-path the low-rank route, a small segment buffer only costs launches -- so q comes first.
// The segment buffer is promised min(what all K vectors' segments need, max(one (k, segment) unit, W / 8)), never more
// than W less one k-vector of q: an eighth takes at most an eighth of q's k-vectors and bounds the launches (where the
// budget binds it is tens to hundreds of megabytes per sub-block).  q takes kb = the rest / (24 B T) k-vectors, and the
// segment buffer then gets whatever q left over, at most kb k-vectors' segments.  It is cut into sub-blocks of as many
// k-vectors as fit (all kb if possible) x the segments that then fit: the contraction's grid grows with bk, not with bs
// (at configuration 3, 40 k-vectors x all 31 segments per launch left the contraction 2.5 wavefronts per SIMD and
// cost 4.6 ms a call; 256 k-vectors x 5 segments cost 3.3 ms).  Without segments there is no segment buffer: the budget
// is q's alone.
#include "api_internal.h"

namespace psa {

// what modes_check checks of the k-list and the site groups, and the sizes that follow from them (shared with
// psa_sed_covariance, which has no mode vectors)
int modes_check_groups(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                       const int64_t* group_off, int32_t B, int32_t flags, ModesCall* m) {
    const int64_t T = c->slot[slot].T, N = c->slot[slot].N;
    PSA_REQUIRE(K >= 0 && K < (1ll << 29), "bad number of k-vectors %lld", (long long)K);
    PSA_REQUIRE(K == 0 || k_vectors != nullptr, "null k_vectors");
    PSA_REQUIRE(T <= (1ll << 31) - 64, "T = %lld frames: the mode contraction indexes frequencies in 32 bits (T <= 2^31 - 64)",
                (long long)T);
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
    m->per_k = (int64_t)B * 3 * T * (int64_t)sizeof(float2);
    int64_t n_max = 0;
    for (int32_t b = 0; b < B; ++b) n_max = std::max(n_max, group_idx ? group_off[b + 1] - group_off[b] : N);
    // a block of k-vectors: a group's phase table under 2 GiB (as project_groups), the contraction's grid
    m->kb_max = std::min<int64_t>(std::max<int64_t>(64, (((int64_t)2 << 30) / (8 * ((n_max + 63) / 64 * 64 + 64))) / 64 * 64),
                                  (int64_t)65535 * 4);
    m->T = T, m->N = N, m->K = K, m->B = B;
    m->list = ProjectArgs{slot, mean_pos_all, k_vectors, K, K, 0, group_idx, group_off, B, flags};
    return PSA_OK;
}

namespace {

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

// every check that does not depend on segments, result size or budget (`what`: the entry point, for the flags message;
// need_out: the caller requires an output it was not given), then the coefficient table and the sizes
int modes_check(psa_ctx* c, const char* what, const ModesArgs& a, bool need_out, ModesCall* m) {
    PSA_TRY(check_slot(c, a.slot));
    const int64_t K = a.K, M = a.M;
    const int32_t B = a.B;
    PSA_REQUIRE((a.flags & ~PSA_F_DISPLACEMENTS) == 0, "%s takes PSA_F_DISPLACEMENTS or 0, got flags 0x%x", what, (unsigned)a.flags);
    PSA_REQUIRE(a.eig != nullptr, "null eig");
    PSA_REQUIRE(!need_out, "null output");
    PSA_REQUIRE(a.mean_pos_all != nullptr, "null mean_pos_all");
    PSA_REQUIRE(M >= 1 && M < (1ll << 30), "need at least one mode vector per k-point (M = %lld)", (long long)M);
    PSA_TRY(modes_check_groups(c, a.slot, a.mean_pos_all, a.k_vectors, K, a.group_idx, a.group_off, B, a.flags, m));
    m->MT = modes_tile(M);
    PSA_TRY(pack_coef(a.eig, K, M, B, m->MT, &m->coef));
    m->coef_k = (size_t)((M + m->MT - 1) / m->MT) * 3 * (size_t)B * (size_t)m->MT;
    m->M = M;
    return PSA_OK;
}

}  // namespace

// k-vectors, mean, lists, coefficients (if any); resolves the group sources
int modes_upload(psa_ctx* c, ModesCall* m) {
    const ProjectArgs& a = m->list;
    {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_kvec, a.k_vectors, (size_t)m->K * 3 * sizeof(float)));
        PSA_TRY(upload(c, c->d_mean_all, a.mean_pos_all, (size_t)m->N * 3 * sizeof(float)));
        if (a.group_idx) PSA_TRY(upload(c, c->d_idx, a.group_idx, (size_t)a.group_off[m->B] * sizeof(int32_t)));
        if (!m->coef.empty()) PSA_TRY(upload(c, c->d_modes_coef, m->coef.data(), m->coef.size() * sizeof(float)));
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

// k-vectors of the block that starts at k0 under a block size kb
int64_t modes_block(const psa_ctx* c, const ModesCall& m, int64_t k0, int64_t kb) {
    int64_t nk = std::min(kb, m.K - k0);
    // a k-path keeps the low-rank route where the budget allows: no tail shorter than PSA_OPT_K1_LOWRANK_MIN_LOCAL
    const int64_t lr_min = c->opt_k1_lowrank_min_local, rest = m.K - k0 - nk;
    if (rest > 0 && rest < lr_min && nk - (lr_min - rest) >= lr_min) nk -= lr_min - rest;
    return nk;
}

// the B groups into (B, nk, 3, T)
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

// Shared by the four entries.  The result, (T, K, M) or with segments (L, K, M), is left in c->d_modes_out.  `segments`: the
// context's segments are honoured (psa_sed_modes_welch) or refused (psa_sed_modes).  a.out may be null only with
// `device_only` (the fits), and is then not copied to.
int modes_run(psa_ctx* c, const ModesArgs& a, bool segments, bool device_only) {
    ModesCall m;
    PSA_TRY(modes_check(c, segments ? "psa_sed_modes_welch" : "psa_sed_modes", a, !a.out && !device_only, &m));
    PSA_REQUIRE(segments || c->seg_L == 0, "psa_sed_modes has no segment average: clear psa_set_segments first (length %lld is set)",
                (long long)c->seg_L);
    const int64_t T = m.T, K = m.K, M = m.M;
    const int32_t B = m.B;
    const bool    cut = c->seg_L != 0;                       // false: one boxcar segment of T frames, q transformed in place
    const int64_t L = cut ? c->seg_L : T, H = cut ? c->seg_hop : T;
    PSA_REQUIRE(L <= T, "segment length %lld exceeds the trajectory's %lld frames", (long long)L, (long long)T);
    const size_t want = (size_t)L * (size_t)K * (size_t)M * sizeof(float);
    PSA_REQUIRE(a.out_bytes == want || !a.out, "out_bytes is %zu, the (%lld,%lld,%lld) float32 result has %zu", a.out_bytes,
                (long long)L, (long long)K, (long long)M, want);
    if (K == 0) return PSA_OK;

    // the budget: q (kb k-vectors) first, the segment buffer (units of one k-vector x one segment) from the rest
    const int64_t n_seg = 1 + (T - L) / H, W = c->opt_modes_work_bytes;
    const int64_t unit = cut ? (int64_t)B * 3 * L * (int64_t)sizeof(float2) : 0;
    PSA_REQUIRE(W >= m.per_k + unit, "the work budget of %lld bytes (PSA_OPT_MODES_WORK_BYTES) cannot hold one k-vector and one "
                "(k-vector, segment) unit: %d groups x 3 components x (%lld frames + a segment of %lld) need %lld bytes",
                (long long)W, (int)B, (long long)T, (long long)(cut ? L : 0), (long long)(m.per_k + unit));
    int64_t seg_bytes = 0;
    if (cut) {
        const int64_t all = (double)K * (double)n_seg * (double)unit < 9e18 ? K * n_seg * unit : INT64_MAX;
        seg_bytes = std::min(std::min(all, std::max(unit, W / 8)), W - m.per_k);
    }
    const int64_t kb = std::min<int64_t>({(W - seg_bytes) / m.per_k, K, m.kb_max});
    int64_t       bk = 0, bs = n_seg;
    if (cut) {
        const int64_t units = std::min((W - kb * m.per_k) / unit, kb * n_seg);
        // many k-vectors x few segments rather than few x all: the contraction's grid is (L / 64) x (bk / 4) workgroups
        // whatever bs, and adding to the result of an earlier launch costs one read of 4 L bk M bytes
        if (units >= kb) bk = kb, bs = std::min(n_seg, units / kb);
        else bk = units, bs = 1;
        if (bk > 4) bk -= bk % 4;                            // whole tiles of the contraction's four k-vectors
        PSA_TRY(c->d_seg.reserve((size_t)bk * (size_t)bs * (size_t)unit));
    }
    PSA_TRY(modes_upload(c, &m));
    PSA_TRY(c->d_modes_work.reserve((size_t)kb * (size_t)m.per_k));
    PSA_TRY(c->d_modes_out.reserve(want));

    const double  U = cut ? c->seg_U : 1.0;
    const float   scale = (float)(1.0 / ((double)L * (double)L * (double)n_seg * U));
    float2*       d_work = c->d_modes_work.as<float2>();
    float2*       d_seg = cut ? c->d_seg.as<float2>() : nullptr;
    const float2* d_coef = c->d_modes_coef.as<float2>();
    float*        d_out = c->d_modes_out.as<float>();
    for (int64_t k0 = 0; k0 < K;) {
        const int64_t nk = modes_block(c, m, k0, kb);
        PSA_TRY(modes_project(c, m, k0, nk, d_work));
        if (!cut) {
            {
                StageTimer st(c, PSA_T_FFT);
                PSA_TRY(run_fft(c, d_work, T, 3 * (int64_t)B * nk));
            }
            StageTimer st(c, PSA_T_EPILOGUE);
            PSA_TRY(launch_mode_power(c, d_work, d_coef + (size_t)k0 * m.coef_k, d_out, T, 1, nk, B, M, m.MT, K, k0, scale, true));
        }
        for (int64_t k1 = 0; cut && k1 < nk; k1 += bk) {
            const int64_t nb = std::min(bk, nk - k1);
            for (int64_t s0 = 0; s0 < n_seg; s0 += bs) {
                const int64_t ns = std::min(bs, n_seg - s0);
                {
                    StageTimer st(c, PSA_T_EPILOGUE);
                    for (int32_t b = 0; b < B; ++b)
                        PSA_TRY(launch_segment_window(c, d_work + ((size_t)b * (size_t)nk + (size_t)k1) * 3 * (size_t)T,
                                                      c->d_seg_window.as<float>(), d_seg + (size_t)b * (size_t)nb * 3 * (size_t)ns * (size_t)L,
                                                      T, L, H, s0, ns, nb));
                }
                {
                    StageTimer st(c, PSA_T_FFT);
                    PSA_TRY(run_fft(c, d_seg, L, 3 * (int64_t)B * nb * ns));
                }
                StageTimer st(c, PSA_T_EPILOGUE);
                PSA_TRY(launch_mode_power(c, d_seg, d_coef + (size_t)(k0 + k1) * m.coef_k, d_out, L, ns, nb, B, M, m.MT, K, k0 + k1,
                                          scale, s0 == 0));
            }
        }
        k0 += nk;
    }
    if (!a.out) return PSA_OK;
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(a.out, c->d_modes_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

namespace {

// The contraction kernel alone on transformed segments S_host (B, K, 3, ns, L) the caller uploads, in one launch
// (seg_block = 0 or >= ns) or in launches of at most seg_block segments
int debug_mode_power(psa_ctx* c, const void* S_host, const void* eig, int32_t B, int64_t K, int64_t M, int64_t L, int64_t ns,
                     int64_t seg_block, float scale, float* out_host) {
    const int          MT = modes_tile(M);
    std::vector<float> coef;
    PSA_TRY(pack_coef((const float*)eig, K, M, B, MT, &coef));
    const size_t out_bytes = (size_t)L * (size_t)K * (size_t)M * sizeof(float);
    PSA_TRY(upload(c, c->d_modes_coef, coef.data(), coef.size() * sizeof(float)));
    PSA_TRY(c->d_modes_out.reserve(out_bytes));
    int rc = PSA_OK;
    if (seg_block == 0 || seg_block >= ns) {
        PSA_TRY(upload(c, c->d_modes_work, S_host, (size_t)B * (size_t)K * 3 * (size_t)ns * (size_t)L * sizeof(float2)));
        rc = launch_mode_power(c, c->d_modes_work.as<float2>(), c->d_modes_coef.as<float2>(), c->d_modes_out.as<float>(), L, ns, K, B, M,
                               MT, K, 0, scale, true);
    } else {
        // launches of at most seg_block segments: each block's rows (B K 3, nb, L) are packed on the host and uploaded
        std::vector<float2> part((size_t)B * (size_t)K * 3 * (size_t)seg_block * (size_t)L);
        const float2*       S = (const float2*)S_host;
        for (int64_t s0 = 0; s0 < ns && rc == PSA_OK; s0 += seg_block) {
            const int64_t nb = std::min(seg_block, ns - s0);
            for (int64_t r = 0; r < (int64_t)B * K * 3; ++r)
                std::memcpy(part.data() + (size_t)r * (size_t)nb * (size_t)L, S + ((size_t)r * (size_t)ns + (size_t)s0) * (size_t)L,
                            (size_t)nb * (size_t)L * sizeof(float2));
            PSA_TRY(upload(c, c->d_modes_work, part.data(), (size_t)B * (size_t)K * 3 * (size_t)nb * (size_t)L * sizeof(float2)));
            rc = launch_mode_power(c, c->d_modes_work.as<float2>(), c->d_modes_coef.as<float2>(), c->d_modes_out.as<float>(), L, nb, K, B,
                                   M, MT, K, 0, scale, s0 == 0);
            PSA_HIP_CHECK(hipStreamSynchronize(c->stream));     // `part` is packed again for the next launch
        }
    }
    if (rc == PSA_OK && hipMemcpyAsync(out_host, c->d_modes_out.ptr, out_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        set_error("copy of the mode powers failed");
        rc = PSA_EHIP;
    }
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));     // the caller's arrays are only read during the call
    return rc;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_sed_modes(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                  const int64_t* group_off, int32_t B, const void* eig, int64_t M, int32_t flags, float* out_host,
                  size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard           guard(c);
    const ModesArgs a{slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, (const float*)eig, M, flags, out_host, out_bytes};
    return synchronised(c, modes_run(c, a, false, false), "psa_sed_modes");
}

int psa_sed_modes_welch(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                        const int64_t* group_off, int32_t B, const void* eig, int64_t M, int32_t flags, float* out_host,
                        size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard           guard(c);
    const ModesArgs a{slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, (const float*)eig, M, flags, out_host, out_bytes};
    return synchronised(c, modes_run(c, a, true, false), "psa_sed_modes_welch");
}

int psa_debug_mode_power(psa_ctx* c, const void* S_host, const void* eig, int32_t B, int64_t K, int64_t M, int64_t T,
                         float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_REQUIRE(S_host && eig && out_host && B >= 1 && K >= 1 && K <= (int64_t)65535 * 4 && M >= 1 && M < (1ll << 30) && T >= 1,
                "bad argument");
    return debug_mode_power(c, S_host, eig, B, K, M, T, 1, 0, 1.f, out_host);
}

int psa_debug_mode_power_welch(psa_ctx* c, const void* S_host, const void* eig, int32_t B, int64_t K, int64_t M, int64_t L, int64_t ns,
                               int64_t seg_block, float scale, float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_REQUIRE(S_host && eig && out_host && B >= 1 && K >= 1 && K <= (int64_t)65535 * 4 && M >= 1 && M < (1ll << 30) && L >= 1 &&
                    ns >= 1 && ns < (1ll << 31) && seg_block >= 0,
                "bad argument");
    return debug_mode_power(c, S_host, eig, B, K, M, L, ns, seg_block, scale, out_host);
}

}  // extern "C"
