// psa_partial_spectra: the species-resolved (partial) dynamic structure factor and current correlations on the reciprocal
// lattice of the simulation box, per vector or averaged over shells of |k| (definition: include/psa_hip.h; kernels:
// lattice.hip for the projection, partial.hip for the pair passes).  The flow is psa_lattice_spectra's (api_lattice.hip)
// with S species' series per vector: q is (kb, S, NC, T) and the segment buffer (nb, S, NC, ns, L), so the window pass and
// the rocFFT see only more rows, and the unchanged projection kernel fills q with one launch per species -- that species'
// slice of the uploaded atom list, its own n_g, the q pointer advanced by a NC T, and a row table that holds S row.  What
// differs is the pass after the FFT, which takes the products of a pair of species (partial.hip) under the same host loop
// (power_block).  The budget rule (PSA_OPT_DYNAMIC_WORK_BYTES, dynamic_plan) counts S NC series per vector.
// Outside the budget, as for psa_lattice_spectra: the result (1 or 3, P, L, K or n_bins) and the shell form's float64
// accumulator of twice its bytes.
#include "api_internal.h"

namespace psa {

namespace {

struct ParCall {
    DynCall  d;                                      // sizes, segments, block rule (kappa unused; khat in row order)
    int      S = 1, P = 1;
    bool     shell = false;
    int64_t  n_bins = 0;
    float    box_hi[9], box_lo[9];
    std::vector<int64_t>  start;                     // (S + 1) the species' offsets into the atom list
    std::vector<int64_t>  block_tile0;               // first tile of block b (n_blocks + 1)
    std::vector<int32_t>  tile_off, dest;            // (n_tiles + 1); (n_tiles LAT_KS): S row, or -1
    std::vector<uint16_t> ent;
    std::vector<uint32_t> slot;                      // (n_tiles LAT_KS)
    std::vector<int32_t>  bin_start;                 // (n_bins + 1) in the processing order
    std::vector<double>   scale;                     // (n_bins) 1 / (2 n_half n_seg U L^2); an empty bin: 0
};

int species_count(int32_t n_species) {
    PSA_REQUIRE(n_species >= 1 && n_species <= PARTIAL_MAX_SPECIES, "1 to %d species are served, got %d", PARTIAL_MAX_SPECIES,
                (int)n_species);
    return PSA_OK;
}

// every refusal, the sizes, the block rule and the plan
int partial_check(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                  const int32_t* idx, const int64_t* species_start, int32_t n_species, int32_t currents, ParCall* p) {
    PSA_REQUIRE(box_inverse != nullptr, "null box_inverse");
    PSA_REQUIRE(indices != nullptr, "null indices");
    PSA_REQUIRE(idx != nullptr && species_start != nullptr, "null atom list or species offsets");
    PSA_TRY(species_count(n_species));
    const int S = n_species;
    PSA_REQUIRE(species_start[0] == 0, "species_start[0] is %lld: the offsets begin at 0", (long long)species_start[0]);
    for (int a = 0; a < S; ++a)
        PSA_REQUIRE(species_start[a] <= species_start[a + 1], "species_start[%d] = %lld after %lld: the offsets are not ascending", a + 1,
                    (long long)species_start[a + 1], (long long)species_start[a]);
    const int64_t n_g = species_start[S];
    DynCall& d = p->d;
    PSA_TRY(dynamic_inputs(c, "psa_partial_spectra", K, idx, n_g, currents, &d));
    std::vector<int8_t> owner((size_t)d.N, (int8_t)-1);
    for (int a = 0; a < S; ++a)
        for (int64_t i = species_start[a]; i < species_start[a + 1]; ++i) {
            int8_t& o = owner[(size_t)idx[i]];
            PSA_REQUIRE(o < 0 || o == a, "atom %d is listed in species %d and in species %d: the species are disjoint", (int)idx[i],
                        (int)o, a);
            o = (int8_t)a;
        }
    PSA_TRY(lattice_inputs(box_inverse, indices, K, bin_of, n_bins));
    p->S = S, p->P = S * (S + 1) / 2;
    p->start.assign(species_start, species_start + S + 1);
    p->shell = bin_of != nullptr;
    p->n_bins = p->shell ? n_bins : 0;
    d.n_species = S;
    PSA_TRY(dynamic_plan(c, &d));

    const double* B = box_inverse;
    lattice_box_parts(B, p->box_hi, p->box_lo);
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

    // blocks, tiles, entries; a vector's row of q counts series sets of one species, so the table holds S row
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
                p->dest.push_back(row < 0 ? -1 : (int32_t)(row * S));
            }
        }
        p->block_tile0.push_back((int64_t)p->tile_off.size() - 1);
    }
    PSA_REQUIRE(p->ent.size() < (1ull << 31) && p->tile_off.size() < (1ull << 22), "the vector list needs too many tiles");
    PSA_REQUIRE((double)d.kb * S < (double)(1ll << 31), "a block of %lld vectors x %d species is more than the row table serves",
                (long long)d.kb, S);

    if (p->shell) {
        std::vector<int64_t> count((size_t)n_bins, 0);
        for (int64_t k = 0; k < K; ++k) ++count[(size_t)bin_of[k]];
        lattice_bins(count, (double)d.n_seg, d.cut ? c->seg_U : 1.0, (double)d.L, &p->bin_start, &p->scale);
    }
    return PSA_OK;
}

int partial_upload(psa_ctx* c, const ParCall& p, const int32_t* idx) {
    StageTimer st(c, PSA_T_H2D);
    PSA_TRY(upload(c, c->d_par_tiles, p.tile_off.data(), p.tile_off.size() * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_par_ent, p.ent.data(), p.ent.size() * sizeof(uint16_t)));
    PSA_TRY(upload(c, c->d_par_slot, p.slot.data(), p.slot.size() * sizeof(uint32_t)));
    PSA_TRY(upload(c, c->d_par_dest, p.dest.data(), p.dest.size() * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_par_khat, p.d.khat.data(), p.d.khat.size() * sizeof(float)));
    PSA_TRY(upload(c, c->d_par_idx, idx, (size_t)p.d.n_g * sizeof(int32_t)));
    if (p.shell) {
        PSA_TRY(upload(c, c->d_par_bins, p.bin_start.data(), p.bin_start.size() * sizeof(int32_t)));
        PSA_TRY(upload(c, c->d_par_scale, p.scale.data(), p.scale.size() * sizeof(double)));
    }
    return PSA_OK;
}

// block b of the plan over all frames into d_q (nk, S, NC, T): one launch of the lattice kernel per species (an empty one
// writes its zeros)
int partial_project(psa_ctx* c, const ParCall& p, int64_t block, float2* d_q) {
    StageTimer st(c, PSA_T_PROJECT);
    const DynCall& d = p.d;
    for (int a = 0; a < p.S; ++a)
        PSA_TRY(launch_lattice_project(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(),
                                       d.NC == 4 ? c->slot[PSA_SLOT_VELOCITIES].buf.as<float>() : nullptr,
                                       c->weights_N ? c->d_weights.as<float>() : nullptr, c->d_par_idx.as<int>() + p.start[(size_t)a],
                                       p.box_hi, p.box_lo, c->d_par_tiles.as<int>(), c->d_par_ent.as<unsigned short>(),
                                       c->d_par_slot.as<unsigned>(), c->d_par_dest.as<int>(), d_q + (size_t)a * (size_t)d.NC * (size_t)d.T,
                                       d.T, d.N, p.start[(size_t)a + 1] - p.start[(size_t)a], p.block_tile0[(size_t)block],
                                       p.block_tile0[(size_t)block + 1] - p.block_tile0[(size_t)block], d.NC == 4));
    return PSA_OK;
}

// the shell form's float64 accumulator, zeroed; and its last launch: scale in float64, one rounding into d_out
int partial_shell_begin(psa_ctx* c, size_t bytes, double** d_acc) {
    PSA_TRY(c->d_par_acc.reserve(bytes));
    *d_acc = c->d_par_acc.as<double>();
    PSA_HIP_CHECK(hipMemsetAsync(*d_acc, 0, bytes, c->stream));
    return PSA_OK;
}
int partial_shell_finish(psa_ctx* c, int64_t n, int64_t n_bins, float* d_out) {
    StageTimer st(c, PSA_T_EPILOGUE);
    return launch_lattice_finish(c, c->d_par_acc.as<double>(), c->d_par_scale.as<double>(), d_out, n, n_bins);
}

int partial_run(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                const int32_t* idx, const int64_t* species_start, int32_t n_species, int32_t currents, float* out_host, size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    ParCall p;
    PSA_TRY(partial_check(c, box_inverse, indices, K, bin_of, n_bins, idx, species_start, n_species, currents, &p));
    const DynCall& d = p.d;
    const int64_t  L = d.L, T = d.T, S = p.S, rows = currents ? 3 : 1, cols = p.shell ? n_bins : K;
    const size_t   want = (size_t)rows * (size_t)p.P * (size_t)L * (size_t)cols * sizeof(float);
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%lld,%d,%lld,%lld) float32 result has %zu", out_bytes, (long long)rows, p.P,
                (long long)L, (long long)cols, want);
    if (d.n_g == 0) {                                        // every species empty: zeros
        std::memset(out_host, 0, out_bytes);
        return PSA_OK;
    }
    PSA_TRY(partial_upload(c, p, idx));
    PSA_TRY(c->d_par_q.reserve((size_t)d.kb * (size_t)d.per_k));
    if (d.cut) PSA_TRY(c->d_seg.reserve((size_t)d.bk * (size_t)d.bs * (size_t)d.unit));
    PSA_TRY(c->d_par_out.reserve(want));
    double* d_acc = nullptr;
    if (p.shell) PSA_TRY(partial_shell_begin(c, want * 2, &d_acc));

    const double U = d.cut ? c->seg_U : 1.0;
    float2*      d_q = c->d_par_q.as<float2>();
    float2*      d_seg = d.cut ? c->d_seg.as<float2>() : nullptr;
    float*       d_out = c->d_par_out.as<float>();
    PowerPass    pass;
    pass.NC = d.NC, pass.n_species = p.S, pass.L = L, pass.n_seg = d.n_seg, pass.K = K;
    pass.scale = (float)(1.0 / ((double)L * (double)L * (double)d.n_seg * U));
    pass.d_khat = c->d_par_khat.as<float>(), pass.d_out = d_out;
    if (p.shell) pass.d_bins = c->d_par_bins.as<int>(), pass.d_acc = d_acc, pass.n_bins = n_bins;
    const int64_t series = S * d.NC;                          // per vector
    int64_t       block = 0;
    for (int64_t k0 = 0; k0 < K; k0 += d.kb, ++block) {
        const int64_t nk = std::min(d.kb, K - k0);
        PSA_TRY(partial_project(c, p, block, d_q));
        // without segments q is transformed where it lies: one sub-block (bk = kb) of the one segment
        PSA_TRY(power_block(c, pass, k0, nk, d.bk, d.bs, [&](int64_t k1, int64_t nb, int64_t s0, int64_t ns, const float2** where) -> int {
            float2* buf = d.cut ? d_seg : d_q;
            if (d.cut) {
                StageTimer st(c, PSA_T_EPILOGUE);
                PSA_TRY(launch_segment_window_rows(c, d_q + (size_t)k1 * (size_t)series * (size_t)T, c->d_seg_window.as<float>(), d_seg, T, L,
                                                   d.H, s0, ns, nb * series));
            }
            StageTimer st(c, PSA_T_FFT);
            PSA_TRY(run_fft(c, buf, L, series * nb * ns));
            *where = buf;
            return PSA_OK;
        }));
    }
    if (p.shell) PSA_TRY(partial_shell_finish(c, rows * p.P * L * n_bins, n_bins, d_out));
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, d_out, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the projection alone, block by block under the same rule: q (K, S, NC, T) before any FFT, rows in the caller's order
int partial_debug_project(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx,
                          const int64_t* species_start, int32_t n_species, int32_t currents, void* out_host) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    ParCall p;
    PSA_TRY(partial_check(c, box_inverse, indices, K, nullptr, 0, idx, species_start, n_species, currents, &p));
    const DynCall& d = p.d;
    if (d.n_g == 0) {
        std::memset(out_host, 0, (size_t)K * (size_t)d.per_k);
        return PSA_OK;
    }
    PSA_TRY(partial_upload(c, p, idx));
    PSA_TRY(c->d_par_q.reserve((size_t)d.kb * (size_t)d.per_k));
    int64_t block = 0;
    for (int64_t k0 = 0; k0 < K; k0 += d.kb, ++block) {
        const int64_t nk = std::min(d.kb, K - k0);
        PSA_TRY(partial_project(c, p, block, c->d_par_q.as<float2>()));
        PSA_HIP_CHECK(hipMemcpyAsync((char*)out_host + (size_t)k0 * (size_t)d.per_k, c->d_par_q.ptr, (size_t)nk * (size_t)d.per_k,
                                     hipMemcpyDeviceToHost, c->stream));
    }
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the pair pass alone on transformed segments (K, S, NC, n_seg, L) of the caller's: what partial_run does after its FFT,
// cut into sub-blocks of k_block vectors x seg_block segments (0: all).  bin_of null: the per-vector form with the scale
// (float) (1 / norm); else the shell form, the vectors sorted by bin, with the bins' scales 1 / (2 n_b norm).
int partial_debug_power(psa_ctx* c, const void* seg_host, const float* khat, const int32_t* bin_of, int64_t K, int64_t n_bins,
                        int32_t n_species, int32_t currents, int64_t n_seg, int64_t L, int64_t k_block, int64_t seg_block, double norm,
                        float* out_host) {
    PSA_REQUIRE(seg_host != nullptr && out_host != nullptr && (khat != nullptr || !currents), "null argument");
    PSA_TRY(species_count(n_species));
    PSA_REQUIRE(currents == 0 || currents == 1, "currents is 0 (density only) or 1 (density and currents), got %d", (int)currents);
    PSA_REQUIRE(K >= 1 && K < (1ll << 29) && n_seg >= 1 && L >= 1 && k_block >= 0 && seg_block >= 0,
                "K, n_seg and L are positive, k_block and seg_block not negative (%lld, %lld, %lld, %lld, %lld)", (long long)K,
                (long long)n_seg, (long long)L, (long long)k_block, (long long)seg_block);
    PSA_REQUIRE(std::isfinite(norm) && norm > 0.0, "the norm n_seg U L^2 must be positive");
    const bool    shell = bin_of != nullptr;
    const int     NC = currents ? 4 : 1, S = n_species, P = S * (S + 1) / 2;
    const int64_t rows = currents ? 3 : 1, cols = shell ? n_bins : K, series = (int64_t)S * NC;
    const int64_t bk = k_block == 0 ? K : std::min(k_block, K), bs = seg_block == 0 ? n_seg : std::min(seg_block, n_seg);
    PSA_REQUIRE(!shell || (n_bins >= 1 && n_bins < (1ll << 24)), "need at least one bin (n_bins = %lld)", (long long)n_bins);
    PSA_REQUIRE((double)bk * (double)series * (double)bs * (double)L < (double)(1ll << 28) &&
                    (double)P * (double)cols * (double)L < (double)(1ll << 28),
                "a sub-block of %lld x %lld x %lld x %lld elements is more than this entry serves", (long long)bk, (long long)series,
                (long long)bs, (long long)L);
    for (int64_t i = 0; currents && i < 3 * K; ++i) PSA_REQUIRE(std::isfinite(khat[i]), "khat[%lld] is not finite", (long long)i);
    const std::vector<float> zeros((size_t)K * 3, 0.f);
    PSA_TRY(upload(c, c->d_par_khat, currents ? khat : zeros.data(), (size_t)K * 3 * sizeof(float)));
    const size_t want = (size_t)rows * (size_t)P * (size_t)L * (size_t)cols * sizeof(float);
    PSA_TRY(c->d_par_out.reserve(want));
    PowerPass pass;
    pass.NC = NC, pass.n_species = S, pass.L = L, pass.n_seg = n_seg, pass.K = K, pass.scale = (float)(1.0 / norm);
    pass.d_khat = c->d_par_khat.as<float>(), pass.d_out = c->d_par_out.as<float>();
    if (shell) {
        std::vector<int64_t> count((size_t)n_bins, 0);
        for (int64_t k = 0; k < K; ++k) {
            PSA_REQUIRE(bin_of[k] >= 0 && bin_of[k] < n_bins, "bin_of[%lld] = %d is outside [0, %lld)", (long long)k, (int)bin_of[k],
                        (long long)n_bins);
            PSA_REQUIRE(k == 0 || bin_of[k - 1] <= bin_of[k], "bin_of[%lld] = %d after %d: the vectors come sorted by bin", (long long)k,
                        (int)bin_of[k], (int)bin_of[k - 1]);
            ++count[(size_t)bin_of[k]];
        }
        std::vector<int32_t> bin_start;
        std::vector<double>  scale;
        lattice_bins(count, norm, 1.0, 1.0, &bin_start, &scale);
        PSA_TRY(upload(c, c->d_par_bins, bin_start.data(), bin_start.size() * sizeof(int32_t)));
        PSA_TRY(upload(c, c->d_par_scale, scale.data(), scale.size() * sizeof(double)));
        double* d_acc = nullptr;
        PSA_TRY(partial_shell_begin(c, want * 2, &d_acc));
        pass.d_bins = c->d_par_bins.as<int>(), pass.d_acc = d_acc, pass.n_bins = n_bins;
    }
    PSA_TRY(power_block(c, pass, 0, K, bk, bs, [&](int64_t k1, int64_t nb, int64_t s0, int64_t ns, const float2** where) -> int {
        PSA_TRY(upload_segments(c, c->d_par_q, seg_host, k1 * series, nb * series, n_seg, s0, ns, L));
        *where = c->d_par_q.as<float2>();
        return PSA_OK;
    }));
    if (shell) PSA_TRY(partial_shell_finish(c, rows * P * L * n_bins, n_bins, pass.d_out));
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_par_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_partial_spectra(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                        const int32_t* idx, const int64_t* species_start, int32_t n_species, int32_t currents, float* out_host,
                        size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, partial_run(c, box_inverse, indices, K, bin_of, n_bins, idx, species_start, n_species, currents, out_host,
                                       out_bytes), "psa_partial_spectra");
}

int psa_debug_partial_project(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx,
                              const int64_t* species_start, int32_t n_species, int32_t currents, void* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, partial_debug_project(c, box_inverse, indices, K, idx, species_start, n_species, currents, out_host),
                        "psa_debug_partial_project");
}

int psa_debug_partial_power(psa_ctx* c, const void* seg_host, const float* khat, const int32_t* bin_of, int64_t K, int64_t n_bins,
                            int32_t n_species, int32_t currents, int64_t n_seg, int64_t L, int64_t k_block, int64_t seg_block,
                            double norm, float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, partial_debug_power(c, seg_host, khat, bin_of, K, n_bins, n_species, currents, n_seg, L, k_block, seg_block,
                                               norm, out_host), "psa_debug_partial_power");
}

}  // extern "C"
