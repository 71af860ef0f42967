// psa_lattice_spectra: the dynamic structure factor and the current correlations on the reciprocal lattice of the
// simulation box, per vector or averaged over shells of |k| (definition: include/psa_hip.h; kernels: lattice.hip).  The
// flow is psa_dynamic_spectra's (api_dynamic.hip), with its checks of the slots, the atom set and the weights, its segments
// and its budget rule (PSA_OPT_DYNAMIC_WORK_BYTES): per block of kb vectors the projection kernel writes q (kb, NC, T);
// the window pass, the rocFFT and -- in the per-vector form -- dynamic.hip's power pass follow unchanged.  In the shell
// form the power pass is replaced by the shell pass, which adds every sub-block's vectors to a float64 accumulator
// (1 or 3, L, n_bins) on the device, and one last launch scales and rounds it: (L, n_bins) crosses to the host, not (L, K).
//
// The plan.  The projection kernel wants the vectors of a tile close in index space (a tile's table holds one entry per
// distinct (axis, index) pair), the shell pass wants every bin's vectors of a block in one contiguous range.  So the
// vectors are processed in an order of the host's choosing:
//   per-vector form   block by block as given, inside a block sorted by (n_1, n_2, n_3); a vector's row of q is its place
//                     in the caller's list, so everything after the projection sees the caller's order;
//   shell form        the whole list sorted by (bin, n_1, n_2, n_3), then cut into blocks; a vector's row of q is its
//                     place in that order.
// A block is cut into tiles of LAT_KS vectors.  Per tile: its entries (axis << 8 | m + 128), ascending; per vector the
// three entries it reads and its row.  A vector's sum over atoms does not depend on which tile or block it is in.
// Every block starts a new tile, and a tile's slot and row tables have LAT_KS entries whatever it holds: a budget that
// leaves a handful of vectors per block costs 4 KiB of plan and a 256-lane workgroup per handful -- correct, and slow.
// Outside the budget, like d_dyn_out: the result and the shell form's accumulator, 8 (1 or 3) L n_bins bytes.
#include <numeric>

#include "api_internal.h"

namespace psa {

// the refusals that concern the box and the vector list (K >= 1, both pointers checked by the caller)
int lattice_inputs(const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins) {
    const double* B = box_inverse;
    for (int i = 0; i < 9; ++i) PSA_REQUIRE(std::isfinite(B[i]), "box_inverse[%d] is not finite", i);
    const double det = B[0] * (B[4] * B[8] - B[5] * B[7]) - B[1] * (B[3] * B[8] - B[5] * B[6]) + B[2] * (B[3] * B[7] - B[4] * B[6]);
    PSA_REQUIRE(std::isfinite(det) && det != 0.0, "box_inverse is singular");
    for (int64_t i = 0; i < 3 * K; ++i)
        PSA_REQUIRE(indices[i] >= -LAT_MAX_INDEX && indices[i] <= LAT_MAX_INDEX, "indices[%lld, %lld] = %d: |n_j| <= %d is served",
                    (long long)(i / 3), (long long)(i % 3), (int)indices[i], LAT_MAX_INDEX);
    if (bin_of != nullptr) {
        PSA_REQUIRE(n_bins >= 1 && n_bins < (1ll << 24), "need at least one bin (n_bins = %lld)", (long long)n_bins);
        for (int64_t k = 0; k < K; ++k) {
            PSA_REQUIRE(bin_of[k] >= 0 && bin_of[k] < n_bins, "bin_of[%lld] = %d is outside [0, %lld)", (long long)k, (int)bin_of[k],
                        (long long)n_bins);
            const int32_t* n = indices + 3 * k;
            const int32_t  lead = n[0] != 0 ? n[0] : n[1] != 0 ? n[1] : n[2];
            PSA_REQUIRE(lead > 0, "indices[%lld] = (%d, %d, %d) is not a half-space member (first non-zero index positive): the "
                        "shell form folds -n onto n", (long long)k, (int)n[0], (int)n[1], (int)n[2]);
        }
    }
    return PSA_OK;
}

void lattice_box_parts(const double* B, float* hi, float* lo) {
    for (int i = 0; i < 9; ++i) {
        hi[i] = (float)B[i];
        lo[i] = (float)(B[i] - (double)hi[i]);
    }
}

// the processing order: with bins the whole list by (bin, n_1, n_2, n_3); without, every run of kb vectors by (n_1, n_2, n_3)
void lattice_order(const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t kb, std::vector<int64_t>* out) {
    std::vector<int64_t>& order = *out;
    order.resize((size_t)K);
    std::iota(order.begin(), order.end(), (int64_t)0);
    auto by_index = [&](int64_t a, int64_t b) {
        const int32_t *x = indices + 3 * a, *y = indices + 3 * b;
        return x[0] != y[0] ? x[0] < y[0] : x[1] != y[1] ? x[1] < y[1] : x[2] != y[2] ? x[2] < y[2] : a < b;
    };
    if (bin_of)
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return bin_of[a] != bin_of[b] ? bin_of[a] < bin_of[b] : by_index(a, b); });
    else
        for (int64_t k0 = 0; k0 < K; k0 += kb) std::sort(order.begin() + k0, order.begin() + std::min(K, k0 + kb), by_index);
}

// One tile: its nt vectors are members[0 .. nt) of the list.  Appends the tile's entries (axis << 8 | m + 128), ascending,
// to ent and writes per vector the three entries it reads (9 bits each, counted from the tile's first); returns their number R.
int lattice_tile_entries(const int32_t* indices, const int64_t* members, int64_t nt, std::vector<uint16_t>* ent, uint32_t* slot) {
    int  where[3][2 * LAT_MAX_INDEX + 1];
    bool used[3][2 * LAT_MAX_INDEX + 1] = {};
    for (int64_t i = 0; i < nt; ++i)
        for (int j = 0; j < 3; ++j) used[j][indices[3 * members[i] + j] + LAT_MAX_INDEX] = true;
    int R = 0;
    for (int j = 0; j < 3; ++j)
        for (int m = 0; m <= 2 * LAT_MAX_INDEX; ++m)
            if (used[j][m]) {
                where[j][m] = R++;
                ent->push_back((uint16_t)((j << 8) | (m - LAT_MAX_INDEX + 128)));
            }
    for (int64_t i = 0; i < nt; ++i) {
        const int32_t* n = indices + 3 * members[i];
        slot[i] = (uint32_t)where[0][n[0] + LAT_MAX_INDEX] | (uint32_t)where[1][n[1] + LAT_MAX_INDEX] << 9 |
                  (uint32_t)where[2][n[2] + LAT_MAX_INDEX] << 18;
    }
    return R;
}

void lattice_bins(const std::vector<int64_t>& count, double n_seg, double U, double L, std::vector<int32_t>* bin_start,
                  std::vector<double>* scale) {
    const size_t n_bins = count.size();
    bin_start->assign(n_bins + 1, 0);
    scale->assign(n_bins, 0.0);
    for (size_t b = 0; b < n_bins; ++b) {
        (*bin_start)[b + 1] = (int32_t)((*bin_start)[b] + count[b]);
        if (count[b]) (*scale)[b] = 1.0 / (2.0 * (double)count[b] * n_seg * U * L * L);
    }
}

int lattice_check(psa_ctx* c, const char* entry, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of,
                  int64_t n_bins, const int32_t* idx, int64_t n_g, int32_t currents, int64_t n_lags, LatCall* p) {
    PSA_REQUIRE(box_inverse != nullptr, "null box_inverse");
    PSA_REQUIRE(indices != nullptr, "null indices");
    DynCall& d = p->d;
    PSA_TRY(dynamic_inputs(c, entry, K, idx, n_g, currents, &d));
    PSA_TRY(lattice_inputs(box_inverse, indices, K, bin_of, n_bins));
    const double* B = box_inverse;
    p->shell = bin_of != nullptr;
    p->n_bins = p->shell ? n_bins : 0;
    d.n_lags = n_lags;
    PSA_TRY(dynamic_plan(c, &d));

    lattice_box_parts(B, p->box_hi, p->box_lo);
    // the processing order
    std::vector<int64_t> order;
    lattice_order(indices, K, p->shell ? bin_of : nullptr, d.kb, &order);

    // k / |k| in float64, k = 2 pi sum_j n_j Hinv[:, j], in the order of the rows of q
    const double two_pi = 6.283185307179586476925286766559;
    d.khat.assign((size_t)K * 3, 0.f);
    for (int64_t r = 0; r < K; ++r) {
        const int32_t* n = indices + 3 * (p->shell ? order[r] : r);
        double         k[3];
        for (int cc = 0; cc < 3; ++cc) k[cc] = two_pi * ((double)n[0] * B[3 * cc] + (double)n[1] * B[3 * cc + 1] + (double)n[2] * B[3 * cc + 2]);
        const double norm = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
        for (int cc = 0; cc < 3; ++cc)
            if (norm > 0.0) d.khat[(size_t)r * 3 + cc] = (float)(k[cc] / norm);
    }

    // blocks, tiles, entries
    p->block_tile0.assign(1, 0);
    p->tile_off.assign(1, 0);
    for (int64_t k0 = 0; k0 < K; k0 += d.kb) {
        const int64_t nk = std::min(d.kb, K - k0);
        for (int64_t t0 = 0; t0 < nk; t0 += LAT_KS) {
            const int64_t nt = std::min<int64_t>(LAT_KS, nk - t0);
            uint32_t      slots[LAT_KS] = {};
            lattice_tile_entries(indices, order.data() + k0 + t0, nt, &p->ent, slots);
            p->tile_off.push_back((int32_t)p->ent.size());
            for (int64_t i = 0; i < LAT_KS; ++i) {
                const int64_t v = i < nt ? order[k0 + t0 + i] : 0;
                p->slot.push_back(slots[i]);
                p->dest.push_back(i < nt ? (int32_t)(p->shell ? t0 + i : v - k0) : -1);
            }
        }
        p->block_tile0.push_back((int64_t)p->tile_off.size() - 1);
    }
    PSA_REQUIRE(p->ent.size() < (1ull << 31) && p->tile_off.size() < (1ull << 22), "the vector list needs too many tiles");

    if (p->shell) {
        p->count.assign((size_t)n_bins, 0);
        for (int64_t k = 0; k < K; ++k) ++p->count[(size_t)bin_of[k]];
        lattice_bins(p->count, (double)d.n_seg, d.cut ? c->seg_U : 1.0, (double)d.L, &p->bin_start, &p->scale);
    }
    return PSA_OK;
}

int lattice_upload(psa_ctx* c, const LatCall& p, const int32_t* idx) {
    StageTimer st(c, PSA_T_H2D);
    PSA_TRY(upload(c, c->d_lat_tiles, p.tile_off.data(), p.tile_off.size() * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_lat_ent, p.ent.data(), p.ent.size() * sizeof(uint16_t)));
    PSA_TRY(upload(c, c->d_lat_slot, p.slot.data(), p.slot.size() * sizeof(uint32_t)));
    PSA_TRY(upload(c, c->d_lat_dest, p.dest.data(), p.dest.size() * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_lat_khat, p.d.khat.data(), p.d.khat.size() * sizeof(float)));
    if (idx) PSA_TRY(upload(c, c->d_lat_idx, idx, (size_t)p.d.n_g * sizeof(int32_t)));
    if (p.shell) {
        PSA_TRY(upload(c, c->d_lat_bins, p.bin_start.data(), p.bin_start.size() * sizeof(int32_t)));
        PSA_TRY(upload(c, c->d_lat_scale, p.scale.data(), p.scale.size() * sizeof(double)));
    }
    return PSA_OK;
}

// the shell form's float64 accumulator, zeroed; and its last launch: scale in float64, one rounding into d_out
int lattice_shell_begin(psa_ctx* c, size_t bytes, double** d_acc) {
    PSA_TRY(c->d_lat_acc.reserve(bytes));
    *d_acc = c->d_lat_acc.as<double>();
    PSA_HIP_CHECK(hipMemsetAsync(*d_acc, 0, bytes, c->stream));
    return PSA_OK;
}
namespace {

int lattice_shell_finish(psa_ctx* c, int64_t rows, int64_t L, int64_t n_bins, float* d_out) {
    StageTimer st(c, PSA_T_EPILOGUE);
    return launch_lattice_finish(c, c->d_lat_acc.as<double>(), c->d_lat_scale.as<double>(), d_out, rows * L * n_bins, n_bins);
}

}  // namespace

// block b of the plan over all frames into d_q (nk, NC, T)
int lattice_project(psa_ctx* c, const LatCall& p, const int32_t* idx, int64_t block, float2* d_q) {
    StageTimer st(c, PSA_T_PROJECT);
    const DynCall& d = p.d;
    return launch_lattice_project(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(),
                                  d.NC == 4 ? c->slot[PSA_SLOT_VELOCITIES].buf.as<float>() : nullptr,
                                  c->weights_N ? c->d_weights.as<float>() : nullptr, idx ? c->d_lat_idx.as<int>() : nullptr, p.box_hi,
                                  p.box_lo, c->d_lat_tiles.as<int>(), c->d_lat_ent.as<unsigned short>(), c->d_lat_slot.as<unsigned>(),
                                  c->d_lat_dest.as<int>(), d_q, d.T, d.N, d.n_g, p.block_tile0[(size_t)block],
                                  p.block_tile0[(size_t)block + 1] - p.block_tile0[(size_t)block], d.NC == 4);
}

namespace {

int lattice_run(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                const int32_t* idx, int64_t n_g, int32_t currents, float* out_host, size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    LatCall p;
    PSA_TRY(lattice_check(c, "psa_lattice_spectra", box_inverse, indices, K, bin_of, n_bins, idx, n_g, currents, 0, &p));
    const DynCall& d = p.d;
    const int64_t  L = d.L, T = d.T, rows = currents ? 3 : 1, cols = p.shell ? n_bins : K;
    const size_t   want = (size_t)rows * (size_t)L * (size_t)cols * sizeof(float);
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%lld,%lld,%lld) float32 result has %zu", out_bytes, (long long)rows,
                (long long)L, (long long)cols, want);
    if (d.n_g == 0) {                                        // an empty atom set: zeros
        std::memset(out_host, 0, out_bytes);
        return PSA_OK;
    }
    PSA_TRY(lattice_upload(c, p, idx));
    PSA_TRY(c->d_lat_q.reserve((size_t)d.kb * (size_t)d.per_k));
    if (d.cut) PSA_TRY(c->d_seg.reserve((size_t)d.bk * (size_t)d.bs * (size_t)d.unit));
    PSA_TRY(c->d_lat_out.reserve(want));
    double* d_acc = nullptr;
    if (p.shell) PSA_TRY(lattice_shell_begin(c, want * 2, &d_acc));

    const double U = d.cut ? c->seg_U : 1.0;
    const float  scale = (float)(1.0 / ((double)L * (double)L * (double)d.n_seg * U));
    float2*      d_q = c->d_lat_q.as<float2>();
    float2*      d_seg = d.cut ? c->d_seg.as<float2>() : nullptr;
    float*       d_out = c->d_lat_out.as<float>();
    PowerPass    pass;
    pass.NC = d.NC, pass.L = L, pass.n_seg = d.n_seg, pass.K = K, pass.scale = scale;
    pass.d_khat = c->d_lat_khat.as<float>(), pass.d_out = d_out;
    if (p.shell) pass.d_bins = c->d_lat_bins.as<int>(), pass.d_acc = d_acc, pass.n_bins = n_bins;
    int64_t      block = 0;
    for (int64_t k0 = 0; k0 < K; k0 += d.kb, ++block) {
        const int64_t nk = std::min(d.kb, K - k0);
        PSA_TRY(lattice_project(c, p, idx, block, d_q));
        // without segments q is transformed where it lies: one sub-block (bk = kb) of the one segment
        PSA_TRY(power_block(c, pass, k0, nk, d.bk, d.bs, [&](int64_t k1, int64_t nb, int64_t s0, int64_t ns, const float2** where) -> int {
            float2* buf = d.cut ? d_seg : d_q;
            if (d.cut) {
                StageTimer st(c, PSA_T_EPILOGUE);
                PSA_TRY(launch_segment_window_rows(c, d_q + (size_t)k1 * (size_t)d.NC * (size_t)T, c->d_seg_window.as<float>(), d_seg, T, L,
                                                   d.H, s0, ns, nb * d.NC));
            }
            StageTimer st(c, PSA_T_FFT);
            PSA_TRY(run_fft(c, buf, L, (int64_t)d.NC * nb * ns));
            *where = buf;
            return PSA_OK;
        }));
    }
    if (p.shell) PSA_TRY(lattice_shell_finish(c, rows, L, n_bins, d_out));
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, d_out, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the projection kernel alone, block by block under the same rule: q (K, NC, T) before any FFT, rows in the caller's order
int lattice_debug_project(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx, int64_t n_g,
                          int32_t currents, void* out_host) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    LatCall p;
    PSA_TRY(lattice_check(c, "psa_lattice_spectra", box_inverse, indices, K, nullptr, 0, idx, n_g, currents, 0, &p));
    const DynCall& d = p.d;
    if (d.n_g == 0) {
        std::memset(out_host, 0, (size_t)K * (size_t)d.per_k);
        return PSA_OK;
    }
    PSA_TRY(lattice_upload(c, p, idx));
    PSA_TRY(c->d_lat_q.reserve((size_t)d.kb * (size_t)d.per_k));
    int64_t block = 0;
    for (int64_t k0 = 0; k0 < K; k0 += d.kb, ++block) {
        const int64_t nk = std::min(d.kb, K - k0);
        PSA_TRY(lattice_project(c, p, idx, block, c->d_lat_q.as<float2>()));
        PSA_HIP_CHECK(hipMemcpyAsync((char*)out_host + (size_t)k0 * (size_t)d.per_k, c->d_lat_q.ptr, (size_t)nk * (size_t)d.per_k,
                                     hipMemcpyDeviceToHost, c->stream));
    }
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the shell pass and the finish pass alone on transformed segments (K, NC, n_seg, L) of the caller's, the vectors in the
// processing order (sorted by bin): what lattice_run does after its FFT in the shell form, cut into sub-blocks of k_block
// vectors x seg_block segments (0: all); norm = n_seg U L^2 of the bins' scales
int lattice_debug_shell(psa_ctx* c, const void* seg_host, const float* khat, const int32_t* bin_of, int64_t K, int64_t n_bins,
                        int32_t currents, int64_t n_seg, int64_t L, int64_t k_block, int64_t seg_block, double norm, float* out_host) {
    PSA_REQUIRE(seg_host != nullptr && bin_of != nullptr && out_host != nullptr && (khat != nullptr || !currents), "null argument");
    PSA_REQUIRE(currents == 0 || currents == 1, "currents is 0 (density only) or 1 (density and currents), got %d", (int)currents);
    PSA_REQUIRE(K >= 1 && K < (1ll << 29) && n_seg >= 1 && L >= 1 && k_block >= 0 && seg_block >= 0,
                "K, n_seg and L are positive, k_block and seg_block not negative (%lld, %lld, %lld, %lld, %lld)", (long long)K,
                (long long)n_seg, (long long)L, (long long)k_block, (long long)seg_block);
    PSA_REQUIRE(n_bins >= 1 && n_bins < (1ll << 24), "need at least one bin (n_bins = %lld)", (long long)n_bins);
    PSA_REQUIRE(std::isfinite(norm) && norm > 0.0, "the norm n_seg U L^2 must be positive");
    const int     NC = currents ? 4 : 1;
    const int64_t rows = currents ? 3 : 1, bk = k_block == 0 ? K : std::min(k_block, K), bs = seg_block == 0 ? n_seg : std::min(seg_block, n_seg);
    PSA_REQUIRE((double)bk * NC * (double)bs * (double)L < (double)(1ll << 28) && (double)n_bins * (double)L < (double)(1ll << 28),
                "a sub-block of %lld x %d x %lld x %lld elements is more than this entry serves", (long long)bk, NC, (long long)bs,
                (long long)L);
    std::vector<int64_t> count((size_t)n_bins, 0);
    for (int64_t k = 0; k < K; ++k) {
        PSA_REQUIRE(bin_of[k] >= 0 && bin_of[k] < n_bins, "bin_of[%lld] = %d is outside [0, %lld)", (long long)k, (int)bin_of[k],
                    (long long)n_bins);
        PSA_REQUIRE(k == 0 || bin_of[k - 1] <= bin_of[k], "bin_of[%lld] = %d after %d: the vectors come sorted by bin", (long long)k,
                    (int)bin_of[k], (int)bin_of[k - 1]);
        ++count[(size_t)bin_of[k]];
    }
    for (int64_t i = 0; currents && i < 3 * K; ++i) PSA_REQUIRE(std::isfinite(khat[i]), "khat[%lld] is not finite", (long long)i);
    std::vector<int32_t> bin_start;
    std::vector<double>  scale;
    lattice_bins(count, norm, 1.0, 1.0, &bin_start, &scale);
    const std::vector<float> zeros((size_t)K * 3, 0.f);
    PSA_TRY(upload(c, c->d_lat_khat, currents ? khat : zeros.data(), (size_t)K * 3 * sizeof(float)));
    PSA_TRY(upload(c, c->d_lat_bins, bin_start.data(), bin_start.size() * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_lat_scale, scale.data(), scale.size() * sizeof(double)));
    const size_t want = (size_t)rows * (size_t)L * (size_t)n_bins * sizeof(float);
    PSA_TRY(c->d_lat_out.reserve(want));
    double* d_acc = nullptr;
    PSA_TRY(lattice_shell_begin(c, want * 2, &d_acc));
    PowerPass pass;
    pass.NC = NC, pass.L = L, pass.n_seg = n_seg, pass.K = K;
    pass.d_khat = c->d_lat_khat.as<float>(), pass.d_out = c->d_lat_out.as<float>();
    pass.d_bins = c->d_lat_bins.as<int>(), pass.d_acc = d_acc, pass.n_bins = n_bins;
    PSA_TRY(power_block(c, pass, 0, K, bk, bs, [&](int64_t k1, int64_t nb, int64_t s0, int64_t ns, const float2** where) -> int {
        PSA_TRY(upload_segments(c, c->d_lat_q, seg_host, k1 * NC, nb * NC, n_seg, s0, ns, L));
        *where = c->d_lat_q.as<float2>();
        return PSA_OK;
    }));
    PSA_TRY(lattice_shell_finish(c, rows, L, n_bins, pass.d_out));
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_lat_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_lattice_spectra(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                        const int32_t* idx, int64_t n_g, int32_t currents, float* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, lattice_run(c, box_inverse, indices, K, bin_of, n_bins, idx, n_g, currents, out_host, out_bytes),
                        "psa_lattice_spectra");
}

int psa_debug_lattice_shell(psa_ctx* c, const void* seg_host, const float* khat, const int32_t* bin_of, int64_t K, int64_t n_bins,
                            int32_t currents, int64_t n_seg, int64_t L, int64_t k_block, int64_t seg_block, double norm, float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, lattice_debug_shell(c, seg_host, khat, bin_of, K, n_bins, currents, n_seg, L, k_block, seg_block, norm, out_host),
                        "psa_debug_lattice_shell");
}

int psa_debug_lattice_project(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx, int64_t n_g,
                              int32_t currents, void* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, lattice_debug_project(c, box_inverse, indices, K, idx, n_g, currents, out_host), "psa_debug_lattice_project");
}

}  // extern "C"
