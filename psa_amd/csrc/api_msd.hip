// psa_displacement_moments, psa_van_hove_self, psa_debug_unwrap: the mean-square displacement's moments and the self van
// Hove histogram of atom groups, from unwrapped displacements (definition: include/psa_hip.h; kernels: msd.hip).
// Only the positions slot is read; atom weights and segments set on the context are ignored; nothing of the other entry
// points' state is touched.
//
// The atoms are processed in the order of the groups, one group after the other.  Budget (PSA_OPT_DYNAMIC_WORK_BYTES =
// W): the unwrapped displacements u64 of a block, 24 T bytes per atom; a block is a whole number of atoms, W / (24 T) of
// them, and a budget below one atom is refused.  The chunk partials, the accumulator and the result lie outside it.
// Per block: the unwrap pass, then the moments (or histogram) kernel over chunks of the block's atoms -- a chunk lies in
// one group -- and origin slabs, then the reduce into the accumulator that lives across blocks.
#include "api_internal.h"

namespace psa {

// (msd_check, msd_unwrap, msd_chunks, msd_split and msd_upload_list are shared with api_overlap.hip: api_internal.h)
int msd_check(psa_ctx* c, const char* entry, const double* box, const double* box_inverse, const int32_t* idx,
              const int64_t* group_start, int32_t n_groups, int32_t unwrap, AtomGroups* p) {
    PSA_TRY(group_list_check(c, entry, box, box_inverse, idx, group_start, n_groups, p));
    PSA_REQUIRE(unwrap == 0 || unwrap == 1, "unwrap is 0 or 1, got %d", (int)unwrap);
    const int64_t W = c->opt_dynamic_work_bytes, per_atom = 24 * p->T;
    PSA_REQUIRE(W / per_atom >= 1, "the work budget of %lld bytes (PSA_OPT_DYNAMIC_WORK_BYTES) cannot hold the smallest block: the "
                "unwrapped displacements of one atom over %lld frames need %lld bytes", (long long)W, (long long)p->T, (long long)per_atom);
    p->Ab = std::max<int64_t>(1, std::min(p->n_a, W / per_atom));
    return PSA_OK;
}

// the unwrap pass of atoms [a0, a0 + na) of the list into d_msd_u (and d_msd_img)
int msd_unwrap(psa_ctx* c, const AtomGroups& p, const double* box, const double* box_inverse, int64_t a0, int64_t na, bool unwrap,
               bool images) {
    StageTimer    st(c, PSA_T_GATHER);
    const int64_t n_ft = (p.T + MSD_UNWRAP_FRAMES - 1) / MSD_UNWRAP_FRAMES;
    PSA_TRY(c->d_msd_u.reserve((size_t)na * 3 * (size_t)p.T * sizeof(double)));
    if (images) PSA_TRY(c->d_msd_img.reserve((size_t)na * 3 * (size_t)p.T * sizeof(int32_t)));
    if (unwrap) {
        PSA_TRY(c->d_msd_sums.reserve((size_t)n_ft * (size_t)na * 3 * sizeof(int32_t)));
        PSA_TRY(c->d_msd_offs.reserve((size_t)n_ft * (size_t)na * 3 * sizeof(int32_t)));
    }
    return launch_msd_unwrap(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(), p.d_idx, a0, na, box, box_inverse, unwrap,
                             c->d_msd_sums.as<int>(), c->d_msd_offs.as<int>(), c->d_msd_u.as<double>(),
                             images ? c->d_msd_img.as<int>() : nullptr, p.T, p.N);
}

// The chunks of the block [a0, a0 + na): every group's part of it cut into runs of at most `ca` atoms, {first atom of the
// block, one past the last, group, 0}, group by group; first (G + 1): where each group's chunks begin in the table
std::vector<int32_t> msd_chunks(const AtomGroups& p, int64_t a0, int64_t na, int64_t ca, int32_t* first) {
    std::vector<int32_t> ch;
    for (int g = 0; g < p.G; ++g) {
        first[g] = (int32_t)(ch.size() / 4);
        const int64_t lo = std::max(p.start[(size_t)g], a0), hi = std::min(p.start[(size_t)g + 1], a0 + na);
        for (int64_t a = lo; a < hi; a += ca) {
            ch.push_back((int32_t)(a - a0));
            ch.push_back((int32_t)(std::min(a + ca, hi) - a0));
            ch.push_back(g);
            ch.push_back(0);
        }
    }
    first[p.G] = (int32_t)(ch.size() / 4);
    return ch;
}

// origin slabs and atoms per chunk of a launch with `rows` workgroups per (slab, chunk): atoms are split first, then the
// origin tiles; a chunk holds at most `ca_max` atoms
void msd_split(const AtomGroups& p, int64_t rows, int64_t step, int64_t ca_max, int64_t* n_os, int64_t* ca) {
    const int64_t n_ot = ((p.T - 1) / step + 1 + msd_origins(step) - 1) / msd_origins(step);
    const int64_t want = std::max<int64_t>(1, REALSPACE_TARGET_GROUPS / rows);           // (slab, chunk) pairs
    const int64_t chunks = std::min(want, p.Ab);
    *n_os = std::max<int64_t>(1, std::min(n_ot, want / chunks));
    *ca = std::max<int64_t>((p.Ab + chunks - 1) / chunks, (p.Ab + 59999) / 60000);      // the grid's y holds 65535
    *ca = std::max<int64_t>(1, std::min(*ca, ca_max));
}

// the atom list and the groups' sizes
int msd_upload_list(psa_ctx* c, AtomGroups* p, const int32_t* idx) {
    PSA_TRY(upload_atom_list(c, p, idx));
    StageTimer st(c, PSA_T_H2D);
    return upload(c, c->d_msd_sizes, p->size.data(), p->size.size() * sizeof(int64_t));
}

namespace {

int moments_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                int32_t n_groups, int64_t n_lags, int64_t origin_step, int32_t unwrap, double* out_host, size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    AtomGroups p;
    PSA_TRY(msd_check(c, "psa_displacement_moments", box, box_inverse, idx, group_start, n_groups, unwrap, &p));
    PSA_REQUIRE(n_lags >= 1 && n_lags <= p.T, "n_lags = %lld is outside [1, T = %lld]", (long long)n_lags, (long long)p.T);
    PSA_REQUIRE(origin_step >= 1, "origin_step must be at least 1, got %lld", (long long)origin_step);
    const size_t want = (size_t)n_lags * (size_t)p.G * 4 * sizeof(double);
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%lld,%d,4) float64 result has %zu", out_bytes, (long long)n_lags, (int)p.G, want);
    if (p.n_a == 0) {                                        // every group empty: zeros
        std::memset(out_host, 0, out_bytes);
        return PSA_OK;
    }
    PSA_TRY(msd_upload_list(c, &p, idx));
    PSA_TRY(c->d_rs_acc.reserve(want));
    PSA_TRY(c->d_msd_out.reserve(want));
    PSA_HIP_CHECK(hipMemsetAsync(c->d_rs_acc.ptr, 0, want, c->stream));
    int64_t n_os = 1, ca = 1;
    msd_split(p, (n_lags + MSD_LAGS - 1) / MSD_LAGS, origin_step, p.Ab, &n_os, &ca);
    for (int64_t a0 = 0; a0 < p.n_a; a0 += p.Ab) {
        const int64_t na = std::min(p.Ab, p.n_a - a0);
        PSA_TRY(msd_unwrap(c, p, box, box_inverse, a0, na, unwrap != 0, false));
        int32_t                    first[MSD_MAX_GROUPS + 1];
        const std::vector<int32_t> ch = msd_chunks(p, a0, na, ca, first);
        const int64_t              n_chunks = (int64_t)ch.size() / 4;
        PSA_REQUIRE(n_chunks <= 65535, "a block of %lld atoms is too large: lower PSA_OPT_DYNAMIC_WORK_BYTES", (long long)na);
        PSA_TRY(upload(c, c->d_rs_items, ch.data(), ch.size() * sizeof(int32_t)));
        PSA_TRY(c->d_rs_part.reserve((size_t)n_chunks * (size_t)n_os * want / (size_t)p.G));
        {
            StageTimer st(c, PSA_T_TRANSPOSE);
            PSA_TRY(launch_msd_moments(c, c->d_msd_u.as<double>(), c->d_rs_items.ptr, n_chunks, c->d_rs_part.as<double>(), p.T, n_lags,
                                       origin_step, n_os));
        }
        StageTimer st(c, PSA_T_EPILOGUE);
        PSA_TRY(launch_msd_moments_reduce(c, c->d_rs_part.as<double>(), first, c->d_rs_acc.as<double>(), n_lags,
                                          n_os, p.G));
    }
    {
        StageTimer st(c, PSA_T_EPILOGUE);
        PSA_TRY(launch_msd_moments_finish(c, c->d_rs_acc.as<double>(), c->d_msd_sizes.as<int64_t>(), c->d_msd_out.as<double>(), p.T,
                                          n_lags, p.G, origin_step));
    }
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_msd_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

int van_hove_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                 int32_t n_groups, const int64_t* lags, int64_t n_vh, int64_t origin_step, int32_t unwrap, double dr, int32_t n_r,
                 uint64_t* out_host, size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr && lags != nullptr, "null output or lags");
    AtomGroups p;
    PSA_TRY(msd_check(c, "psa_van_hove_self", box, box_inverse, idx, group_start, n_groups, unwrap, &p));
    float inv_dr;
    PSA_TRY(histogram_args_check(p, lags, n_vh, MSD_MAX_VH_LAGS, origin_step, dr, n_r, MSD_MAX_BINS, &inv_dr));
    const size_t want = (size_t)n_vh * (size_t)p.G * (size_t)(n_r + 1) * sizeof(uint64_t);
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%lld,%d,%d) uint64 result has %zu", out_bytes, (long long)n_vh, (int)p.G,
                (int)(n_r + 1), want);
    if (p.n_a == 0) {
        std::memset(out_host, 0, out_bytes);
        return PSA_OK;
    }
    PSA_TRY(msd_upload_list(c, &p, idx));
    PSA_TRY(upload(c, c->d_msd_lags, lags, (size_t)n_vh * sizeof(int64_t)));
    PSA_TRY(c->d_rs_acc.reserve(want));
    PSA_HIP_CHECK(hipMemsetAsync(c->d_rs_acc.ptr, 0, want, c->stream));
    // a workgroup's 32-bit counters: its chunk's atoms x the origins of lag 0 stay below 2^32
    const int64_t n_o0 = (p.T - 1) / origin_step + 1;
    int64_t       n_os = 1, ca = 1;
    msd_split(p, n_vh, origin_step, ((1ll << 32) - 1) / n_o0, &n_os, &ca);
    for (int64_t a0 = 0; a0 < p.n_a; a0 += p.Ab) {
        const int64_t na = std::min(p.Ab, p.n_a - a0);
        PSA_TRY(msd_unwrap(c, p, box, box_inverse, a0, na, unwrap != 0, false));
        int32_t                    first[MSD_MAX_GROUPS + 1];
        const std::vector<int32_t> ch = msd_chunks(p, a0, na, ca, first);
        const int64_t              n_chunks = (int64_t)ch.size() / 4;
        PSA_REQUIRE(n_chunks <= 65535, "a block of %lld atoms is too large: lower PSA_OPT_DYNAMIC_WORK_BYTES", (long long)na);
        PSA_TRY(upload(c, c->d_rs_items, ch.data(), ch.size() * sizeof(int32_t)));
        PSA_TRY(c->d_rs_part.reserve((size_t)n_chunks * (size_t)n_os * (size_t)n_vh * (size_t)(n_r + 1) * sizeof(uint32_t)));
        {
            StageTimer st(c, PSA_T_TRANSPOSE);
            PSA_TRY(launch_msd_hist(c, c->d_msd_u.as<double>(), c->d_rs_items.ptr, n_chunks, c->d_msd_lags.as<int64_t>(), n_vh,
                                    c->d_rs_part.as<unsigned>(), p.T, origin_step, n_os, inv_dr, n_r));
        }
        StageTimer st(c, PSA_T_EPILOGUE);
        HistRows   rows;
        PSA_TRY(rows_of_groups(first, p.G, n_os, &rows));
        PSA_TRY(launch_hist_reduce(c, c->d_rs_part.as<unsigned>(), rows, p.G, n_vh, n_r + 1, c->d_rs_acc.as<unsigned long long>()));
    }
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_rs_acc.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the unwrap pass alone, block by block under the same rule: u (T, n_g, 3) float64 and the image counts (T, n_g, 3) int32
int debug_unwrap_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, int64_t n_g, int32_t unwrap,
                     double* out_u, int32_t* out_images) {
    PSA_REQUIRE(out_u != nullptr, "null output");
    PSA_REQUIRE(idx == nullptr || (n_g >= 0 && n_g < (1ll << 31)), "bad number of atoms %lld", (long long)n_g);
    const int64_t start[2] = {0, n_g};
    AtomGroups       p;
    PSA_TRY(msd_check(c, "psa_debug_unwrap", box, box_inverse, idx, start, 1, unwrap, &p));
    if (p.n_a == 0) return PSA_OK;
    PSA_TRY(msd_upload_list(c, &p, idx));
    std::vector<double>  hu;
    std::vector<int32_t> hi;
    for (int64_t a0 = 0; a0 < p.n_a; a0 += p.Ab) {
        const int64_t na = std::min(p.Ab, p.n_a - a0);
        const size_t  n = (size_t)na * 3 * (size_t)p.T;
        PSA_TRY(msd_unwrap(c, p, box, box_inverse, a0, na, unwrap != 0, out_images != nullptr));
        hu.resize(n);
        PSA_HIP_CHECK(hipMemcpyAsync(hu.data(), c->d_msd_u.ptr, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (out_images) {
            hi.resize(n);
            PSA_HIP_CHECK(hipMemcpyAsync(hi.data(), c->d_msd_img.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        }
        PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
        for (int64_t a = 0; a < na; ++a)
            for (int comp = 0; comp < 3; ++comp)
                for (int64_t t = 0; t < p.T; ++t) {
                    const size_t src = ((size_t)a * 3 + (size_t)comp) * (size_t)p.T + (size_t)t;
                    const size_t dst = ((size_t)t * (size_t)p.n_a + (size_t)(a0 + a)) * 3 + (size_t)comp;
                    out_u[dst] = hu[src];
                    if (out_images) out_images[dst] = hi[src];
                }
    }
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_displacement_moments(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                             int32_t n_groups, int64_t n_lags, int64_t origin_step, int32_t unwrap, double* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, moments_run(c, box, box_inverse, idx, group_start, n_groups, n_lags, origin_step, unwrap, out_host, out_bytes),
                        "psa_displacement_moments");
}

int psa_van_hove_self(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                      int32_t n_groups, const int64_t* lags, int64_t n_vh, int64_t origin_step, int32_t unwrap, double dr, int32_t n_r,
                      uint64_t* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, van_hove_run(c, box, box_inverse, idx, group_start, n_groups, lags, n_vh, origin_step, unwrap, dr, n_r, out_host,
                                        out_bytes),
                        "psa_van_hove_self");
}

int psa_debug_unwrap(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, int64_t n_g, int32_t unwrap,
                     double* out_u, int32_t* out_images) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, debug_unwrap_run(c, box, box_inverse, idx, n_g, unwrap, out_u, out_images), "psa_debug_unwrap");
}

}  // extern "C"
