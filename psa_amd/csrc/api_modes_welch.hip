// psa_sed_modes_welch / psa_sed_modes_welch_fit: the mode-projected SED averaged over Welch segments (definition:
// include/psa_hip.h; kernel: modes_welch.hip).  Checks, coefficient table, uploads, group sources, the block rule and the
// B projections of a block are psa_sed_modes' own (api_modes.hip).  Per block of kb k-vectors the stacked buffer
// q (B, kb, 3, T) is cut, in sub-blocks of bk k-vectors x bs segments, into the segment buffer (B, bk, 3, bs, L) -- one
// launch_segment_window per group, since the rows of one k-vector's B groups lie kb 3 T apart in q --, transformed by
// one batched length-L rocFFT and contracted; the kernel keeps the sum over a sub-block's segments on chip, overwrites
// the sub-block's columns of the (L, K, M) result with the first segments and adds to them with later ones.
// Budget (PSA_OPT_MODES_WORK_BYTES = W; q and the segment buffer share it, the result is outside as for psa_sed_modes):
// shrinking kb can cost a k-path the low-rank route, a small segment buffer only costs launches -- so q comes first.
// The segment buffer is promised min(what all K vectors' segments need, max(one (k, segment) unit, W / 8)), never more
// than W less one k-vector of q: an eighth takes at most an eighth of q's k-vectors and bounds the launches (where the
// budget binds it is tens to hundreds of megabytes per sub-block).  q takes kb = the rest / (24 B T) k-vectors, and the
// segment buffer then gets whatever q left over, at most kb k-vectors' segments.  It is cut into sub-blocks of as many
// k-vectors as fit (all kb if possible) x the segments that then fit: the contraction's grid grows with bk, not with bs
// (at configuration 3, 40 k-vectors x all 31 segments per launch left the contraction 2.5 wavefronts per SIMD and
// cost 4.6 ms a call; 256 k-vectors x 5 segments cost 3.3 ms).
// With no segments set the call is one boxcar segment of T frames: q is transformed in place, as psa_sed_modes does, and
// read by the contraction as (B, kb, 3, 1, T); no segment buffer, the budget is q's alone.
#include "api_internal.h"

namespace psa {

int modes_welch_run(psa_ctx* c, int slot_in, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                    const int64_t* group_off, int32_t B, const float* eig, int64_t M, int32_t flags, float* out_host,
                    size_t out_bytes, bool device_only) {
    ModesCall m;
    PSA_TRY(modes_check(c, "psa_sed_modes_welch", slot_in, mean_pos_all, k_vectors, K, group_idx, group_off, B, eig, M, flags,
                        !out_host && !device_only, &m));
    const int64_t T = m.T;
    const bool    cut = c->seg_L != 0;                       // false: one boxcar segment of T frames, q transformed in place
    const int64_t L = cut ? c->seg_L : T, H = cut ? c->seg_hop : T;
    PSA_REQUIRE(L <= T, "segment length %lld exceeds the trajectory's %lld frames", (long long)L, (long long)T);
    const size_t want = (size_t)L * (size_t)K * (size_t)M * sizeof(float);
    PSA_REQUIRE(out_bytes == want || !out_host, "out_bytes is %zu, the (%lld,%lld,%lld) float32 result has %zu", out_bytes, (long long)L,
                (long long)K, (long long)M, want);
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
            PSA_TRY(launch_mode_welch(c, d_work, d_coef + (size_t)k0 * m.coef_k, d_out, T, 1, nk, B, M, m.MT, K, k0, scale, true));
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
                PSA_TRY(launch_mode_welch(c, d_seg, d_coef + (size_t)(k0 + k1) * m.coef_k, d_out, L, ns, nb, B, M, m.MT, K, k0 + k1,
                                          scale, s0 == 0));
            }
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

int psa_sed_modes_welch(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                        const int64_t* group_off, int32_t B, const void* eig, int64_t M, int32_t flags, float* out_host,
                        size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard     guard(c);
    const int rc = modes_welch_run(c, slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, (const float*)eig, M, flags, out_host,
                                   out_bytes, false);
    // the caller's arrays are only read during the call, whichever way it ends
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == PSA_OK) {
        set_error("hipStreamSynchronize failed after psa_sed_modes_welch");
        return PSA_EHIP;
    }
    return rc;
}

static int welch_fit(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                     const int64_t* group_off, int32_t B, const float* eig, int64_t M, int32_t flags, PeakArgs* a,
                     const psa_peak_opts* opts, float* out_host, size_t out_bytes) {
    PSA_TRY(check_slot(c, slot));
    PSA_REQUIRE(K >= 0 && K < (1ll << 29) && M >= 0 && M < (1ll << 30), "bad number of k-vectors %lld or mode vectors %lld",
                (long long)K, (long long)M);
    a->F = c->seg_L ? c->seg_L : c->slot[slot].T, a->C = K * M;
    PSA_TRY(check_peak_args(opts, a));
    PSA_TRY(modes_welch_run(c, slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, eig, M, flags, out_host, out_bytes, true));
    return peaks_run(c, c->d_modes_out.as<float>(), *a);
}

int psa_sed_modes_welch_fit(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                            const int32_t* group_idx, const int64_t* group_off, int32_t B, const void* eig, int64_t M, int32_t flags,
                            double df, const int32_t* bands, int32_t lo, int32_t hi, const psa_peak_opts* opts, float* fit,
                            int32_t* info, float* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard     guard(c);
    PeakArgs  a{0, 0, df, bands, lo, hi, {}, fit, info};
    const int rc = welch_fit(c, slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, (const float*)eig, M, flags, &a, opts,
                             out_host, out_bytes);
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == PSA_OK) {
        set_error("hipStreamSynchronize failed after psa_sed_modes_welch_fit");
        return PSA_EHIP;
    }
    return rc;
}

int psa_debug_mode_power_welch(psa_ctx* c, const void* S_host, const void* eig, int32_t B, int64_t K, int64_t M, int64_t L, int64_t ns,
                               int64_t seg_block, float scale, float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_REQUIRE(S_host && eig && out_host && B >= 1 && K >= 1 && K <= (int64_t)65535 * 4 && M >= 1 && M < (1ll << 30) && L >= 1 &&
                    ns >= 1 && ns < (1ll << 31) && seg_block >= 0,
                "bad argument");
    const int          MT = modes_tile(M);
    std::vector<float> coef;
    PSA_TRY(pack_coef((const float*)eig, K, M, B, MT, &coef));
    const size_t out_bytes = (size_t)L * (size_t)K * (size_t)M * sizeof(float);
    PSA_TRY(upload(c, c->d_modes_coef, coef.data(), coef.size() * sizeof(float)));
    PSA_TRY(c->d_modes_out.reserve(out_bytes));
    int rc = PSA_OK;
    if (seg_block == 0 || seg_block >= ns) {
        PSA_TRY(upload(c, c->d_modes_work, S_host, (size_t)B * (size_t)K * 3 * (size_t)ns * (size_t)L * sizeof(float2)));
        rc = launch_mode_welch(c, c->d_modes_work.as<float2>(), c->d_modes_coef.as<float2>(), c->d_modes_out.as<float>(), L, ns, K, B, M,
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
            rc = launch_mode_welch(c, c->d_modes_work.as<float2>(), c->d_modes_coef.as<float2>(), c->d_modes_out.as<float>(), L, nb, K, B,
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

}  // extern "C"
