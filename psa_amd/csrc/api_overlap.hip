// psa_self_overlap: per lag, group and time origin the number of atoms within the cut-off of where they were, and its
// first two moments over the origins (definition: include/psa_hip.h; kernels: overlap.hip).  Context, box, groups,
// unwrapping, origins and the block loop are those of psa_van_hove_self (api_msd.hip), whose pieces it is built on.
//
// Budget (PSA_OPT_DYNAMIC_WORK_BYTES = W): the table Q (n_lags, G, n_o_max) uint32, which lives across the blocks of a
// call, and beside it the unwrapped displacements u64 of a block, 24 T bytes per atom; a table that leaves no room for
// one atom is refused.  The chunk partials, the sums and the result lie outside it.  Per block: the unwrap pass, the
// count kernel over chunks of the block's atoms -- a chunk lies in one group --, the reduce into Q; after the last block
// the moments over the origins.
#include "api_internal.h"

namespace psa {

namespace {

int overlap_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                int32_t n_groups, const int64_t* lags, int64_t n_lags, int64_t origin_step, int32_t unwrap, double cutoff,
                uint64_t* out_sums, size_t out_bytes, uint32_t* out_origins, size_t origins_bytes) {
    PSA_REQUIRE(out_sums != nullptr && lags != nullptr, "null output or lags");
    AtomGroups p;
    PSA_TRY(msd_check(c, "psa_self_overlap", box, box_inverse, idx, group_start, n_groups, unwrap, &p));
    PSA_REQUIRE(std::isfinite(cutoff) && cutoff > 0.0, "the cut-off must be positive and finite, got %g", cutoff);
    PSA_REQUIRE(std::isfinite((float)(1.0 / cutoff)), "the cut-off %g has no float32 reciprocal", cutoff);
    float inv_a;
    PSA_TRY(histogram_args_check(p, lags, n_lags, OVERLAP_MAX_LAGS, origin_step, cutoff, 1, 1, &inv_a));
    const int64_t tau_min = *std::min_element(lags, lags + n_lags), n_o_max = (p.T - 1 - tau_min) / origin_step + 1;
    const size_t  want = (size_t)n_lags * (size_t)p.G * 2 * sizeof(uint64_t);
    const size_t  table = (size_t)n_lags * (size_t)p.G * (size_t)n_o_max * sizeof(uint32_t);
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%lld,%d,2) uint64 result has %zu", out_bytes, (long long)n_lags, (int)p.G, want);
    PSA_REQUIRE(out_origins ? origins_bytes == table : origins_bytes == 0, "origins_bytes is %zu, the (%lld,%d,%lld) uint32 table has %zu "
                "(0 without out_origins)", origins_bytes, (long long)n_lags, (int)p.G, (long long)n_o_max, out_origins ? table : (size_t)0);
    const int64_t n_g_max = *std::max_element(p.size.begin(), p.size.end());
    PSA_REQUIRE((unsigned __int128)n_g_max * (unsigned __int128)n_g_max * (unsigned __int128)n_o_max < ((unsigned __int128)1 << 63),
                "the sum of squares may pass 2^63: N_g^2 n_o = %lld^2 x %lld", (long long)n_g_max, (long long)n_o_max);
    const int64_t W = c->opt_dynamic_work_bytes, per_atom = 24 * p.T;
    PSA_REQUIRE((int64_t)table <= W && (W - (int64_t)table) / per_atom >= 1, "the work budget of %lld bytes (PSA_OPT_DYNAMIC_WORK_BYTES) "
                "cannot hold the table of %lld lags x %d groups x %lld origins (%zu bytes) beside the smallest block (one atom over %lld "
                "frames: %lld bytes): use a larger origin_step or fewer lags", (long long)W, (long long)n_lags, (int)p.G,
                (long long)n_o_max, table, (long long)p.T, (long long)per_atom);
    p.Ab = std::max<int64_t>(1, std::min(p.n_a, (W - (int64_t)table) / per_atom));
    if (p.n_a == 0) {                                        // every group empty: zeros
        std::memset(out_sums, 0, out_bytes);
        if (out_origins) std::memset(out_origins, 0, origins_bytes);
        return PSA_OK;
    }
    PSA_TRY(msd_upload_list(c, &p, idx));
    PSA_TRY(upload(c, c->d_msd_lags, lags, (size_t)n_lags * sizeof(int64_t)));
    PSA_TRY(c->d_ov_q.reserve(table));
    PSA_TRY(c->d_ov_sums.reserve(want));
    PSA_HIP_CHECK(hipMemsetAsync(c->d_ov_q.ptr, 0, table, c->stream));
    // workgroups per chunk: lag runs x origin tiles x pieces of a tile; the atoms are split over what is left of the target
    const int64_t NO = msd_origins(origin_step), n_ot = (n_o_max + NO - 1) / NO;
    const int64_t rows = (n_lags + OVERLAP_RUN - 1) / OVERLAP_RUN * n_ot * ((std::min(NO, n_o_max) + OVERLAP_LANES - 1) / OVERLAP_LANES);
    int64_t       n_os = 1, ca = 1;
    msd_split(p, rows, origin_step, p.Ab, &n_os, &ca);       // (no origin slabs: a workgroup owns its origins)
    for (int64_t a0 = 0; a0 < p.n_a; a0 += p.Ab) {
        const int64_t na = std::min(p.Ab, p.n_a - a0);
        PSA_TRY(msd_unwrap(c, p, box, box_inverse, a0, na, unwrap != 0, false));
        int32_t                    first[MSD_MAX_GROUPS + 1];
        const std::vector<int32_t> ch = msd_chunks(p, a0, na, ca, first);
        const int64_t              n_chunks = (int64_t)ch.size() / 4;
        PSA_REQUIRE(n_chunks <= 65535, "a block of %lld atoms is too large: lower PSA_OPT_DYNAMIC_WORK_BYTES", (long long)na);
        PSA_TRY(upload(c, c->d_rs_items, ch.data(), ch.size() * sizeof(int32_t)));
        PSA_TRY(c->d_rs_part.reserve((size_t)n_chunks * (size_t)n_lags * (size_t)n_o_max * sizeof(uint32_t)));
        {
            StageTimer st(c, PSA_T_TRANSPOSE);
            PSA_TRY(launch_overlap_count(c, c->d_msd_u.as<double>(), c->d_rs_items.ptr, n_chunks, c->d_msd_lags.as<int64_t>(), n_lags,
                                         c->d_rs_part.as<unsigned>(), p.T, origin_step, n_o_max, inv_a));
        }
        StageTimer st(c, PSA_T_EPILOGUE);
        PSA_TRY(launch_overlap_reduce(c, c->d_rs_part.as<unsigned>(), first, c->d_msd_lags.as<int64_t>(), c->d_ov_q.as<unsigned>(), p.T,
                                      n_lags, p.G, origin_step, n_o_max));
    }
    {
        StageTimer st(c, PSA_T_EPILOGUE);
        PSA_TRY(launch_overlap_moments(c, c->d_ov_q.as<unsigned>(), c->d_msd_lags.as<int64_t>(), c->d_ov_sums.as<unsigned long long>(), p.T,
                                       n_lags, p.G, origin_step, n_o_max));
    }
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_sums, c->d_ov_sums.ptr, want, hipMemcpyDeviceToHost, c->stream));
    if (out_origins) PSA_HIP_CHECK(hipMemcpyAsync(out_origins, c->d_ov_q.ptr, table, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_self_overlap(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                     int32_t n_groups, const int64_t* lags, int64_t n_lags, int64_t origin_step, int32_t unwrap, double cutoff,
                     uint64_t* out_sums, size_t out_bytes, uint32_t* out_origins, size_t origins_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, overlap_run(c, box, box_inverse, idx, group_start, n_groups, lags, n_lags, origin_step, unwrap, cutoff, out_sums,
                                       out_bytes, out_origins, origins_bytes),
                        "psa_self_overlap");
}

}  // extern "C"
