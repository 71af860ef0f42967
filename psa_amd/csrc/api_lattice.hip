// psa_lattice_spectra: the dynamic structure factor and the current correlations on the reciprocal lattice of the
// simulation box, per vector or averaged over shells of |k| (definition: include/psa_hip.h; kernels: lattice.hip).  Over
// the shared core (api_reciprocal.hip: checks, segments, budget, the run body, the shell pair, the debug loops) this file
// adds the lattice: the refusals that concern the box and the index list, the plan below, its upload and the projection
// launch.  The partial spectra (api_partial.hip) and the lattice time correlations (api_correlation.hip) run on the same
// plan; the self part (api_self.hip) uses its order and tile entries.
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

int lattice_plan(const psa_ctx* c, const double* box_inverse, const int32_t* indices, const int32_t* bin_of, int64_t n_bins,
                 int64_t row_mult, LatCall* p) {
    DynCall&      d = p->d;
    const int64_t K = d.K;
    const double* B = box_inverse;
    p->shell = bin_of != nullptr;
    p->n_bins = p->shell ? n_bins : 0;
    lattice_box_parts(B, p->box_hi, p->box_lo);
    // the processing order
    std::vector<int64_t> order;
    lattice_order(indices, K, bin_of, d.kb, &order);

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

    // blocks, tiles, entries; a vector's row of q counts series sets of one species, so the table holds row_mult row
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
                const int64_t row = i < nt ? (p->shell ? t0 + i : order[k0 + t0 + i] - k0) : -1;
                p->slot.push_back(slots[i]);
                p->dest.push_back(row < 0 ? -1 : (int32_t)(row * row_mult));
            }
        }
        p->block_tile0.push_back((int64_t)p->tile_off.size() - 1);
    }
    PSA_REQUIRE(p->ent.size() < (1ull << 31) && p->tile_off.size() < (1ull << 22), "the vector list needs too many tiles");

    if (p->shell) {
        bin_counts(bin_of, K, n_bins, &p->count);
        lattice_bins(p->count, (double)d.n_seg, d.cut ? c->seg_U : 1.0, (double)d.L, &p->bin_start, &p->scale);
    }
    return PSA_OK;
}

int lattice_check(psa_ctx* c, const char* entry, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of,
                  int64_t n_bins, const int32_t* idx, int64_t n_g, int32_t currents, int64_t n_lags, LatCall* p) {
    PSA_REQUIRE(box_inverse != nullptr, "null box_inverse");
    PSA_REQUIRE(indices != nullptr, "null indices");
    PSA_TRY(dynamic_inputs(c, entry, K, idx, n_g, currents, &p->d));
    PSA_TRY(lattice_inputs(box_inverse, indices, K, bin_of, n_bins));
    p->d.n_lags = n_lags;
    PSA_TRY(dynamic_plan(c, &p->d));
    return lattice_plan(c, box_inverse, indices, bin_of, n_bins, 1, p);
}

int lattice_upload(psa_ctx* c, const LatCall& p, const int32_t* idx) {
    StageTimer st(c, PSA_T_H2D);
    PSA_TRY(upload(c, c->d_rc_tiles, p.tile_off.data(), p.tile_off.size() * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_rc_ent, p.ent.data(), p.ent.size() * sizeof(uint16_t)));
    PSA_TRY(upload(c, c->d_rc_slot, p.slot.data(), p.slot.size() * sizeof(uint32_t)));
    PSA_TRY(upload(c, c->d_rc_dest, p.dest.data(), p.dest.size() * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_rc_khat, p.d.khat.data(), p.d.khat.size() * sizeof(float)));
    if (idx) PSA_TRY(upload(c, c->d_rc_idx, idx, (size_t)p.d.n_g * sizeof(int32_t)));
    if (p.shell) {
        PSA_TRY(upload(c, c->d_rc_bins, p.bin_start.data(), p.bin_start.size() * sizeof(int32_t)));
        PSA_TRY(upload(c, c->d_rc_scale, p.scale.data(), p.scale.size() * sizeof(double)));
    }
    return PSA_OK;
}

int lattice_project(psa_ctx* c, const LatCall& p, bool listed, int64_t a0, int64_t n_g, int64_t block, float2* d_q) {
    const DynCall& d = p.d;
    return launch_lattice_project(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(),
                                  d.NC == 4 ? c->slot[PSA_SLOT_VELOCITIES].buf.as<float>() : nullptr,
                                  c->weights_N ? c->d_weights.as<float>() : nullptr, listed ? c->d_rc_idx.as<int>() + a0 : nullptr,
                                  p.box_hi, p.box_lo, c->d_rc_tiles.as<int>(), c->d_rc_ent.as<unsigned short>(),
                                  c->d_rc_slot.as<unsigned>(), c->d_rc_dest.as<int>(), d_q, d.T, d.N, n_g, p.block_tile0[(size_t)block],
                                  p.block_tile0[(size_t)block + 1] - p.block_tile0[(size_t)block], d.NC == 4);
}

BlockSource lattice_source(psa_ctx* c, const LatCall& p, const int32_t* idx) {
    BlockSource src;
    src.upload = [c, &p, idx]() -> int { return lattice_upload(c, p, idx); };
    src.project = [c, &p, idx](int64_t block, int64_t, int64_t, float2* d_q) -> int {
        return lattice_project(c, p, idx != nullptr, 0, p.d.n_g, block, d_q);
    };
    return src;
}

namespace {

int lattice_run(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                const int32_t* idx, int64_t n_g, int32_t currents, float* out_host, size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    LatCall p;
    PSA_TRY(lattice_check(c, "psa_lattice_spectra", box_inverse, indices, K, bin_of, n_bins, idx, n_g, currents, 0, &p));
    SpectraRun a;
    a.src = lattice_source(c, p, idx), a.n_bins = p.n_bins, a.out_host = out_host, a.out_bytes = out_bytes;
    return spectra_run(c, p.d, a);
}

// the projection kernel alone: q (K, NC, T), rows in the caller's order
int lattice_debug_project(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx, int64_t n_g,
                          int32_t currents, void* out_host) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    LatCall p;
    PSA_TRY(lattice_check(c, "psa_lattice_spectra", box_inverse, indices, K, nullptr, 0, idx, n_g, currents, 0, &p));
    return debug_project_run(c, p.d, lattice_source(c, p, idx), out_host);
}

// the shell pass and the finish pass alone on transformed segments (K, NC, n_seg, L) of the caller's, the vectors in the
// processing order (sorted by bin); norm = n_seg U L^2 of the bins' scales
int lattice_debug_shell(psa_ctx* c, const void* seg_host, const float* khat, const int32_t* bin_of, int64_t K, int64_t n_bins,
                        int32_t currents, int64_t n_seg, int64_t L, int64_t k_block, int64_t seg_block, double norm, float* out_host) {
    PSA_REQUIRE(seg_host != nullptr && bin_of != nullptr && out_host != nullptr && (khat != nullptr || !currents), "null argument");
    DebugPower a{.seg_host = seg_host, .bin_of = bin_of, .K = K, .n_bins = n_bins, .currents = currents, .n_seg = n_seg, .L = L,
                 .k_block = k_block, .seg_block = seg_block, .norm = norm, .out_host = out_host};
    PSA_TRY(debug_power_check(&a));
    return debug_power_run(c, a, khat);
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
