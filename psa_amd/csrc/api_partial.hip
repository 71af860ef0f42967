// psa_partial_spectra: the species-resolved (partial) dynamic structure factor and current correlations on the reciprocal
// lattice of the simulation box, per vector or averaged over shells of |k| (definition: include/psa_hip.h; kernels:
// lattice.hip for the projection, partial.hip for the pair passes).  It is psa_lattice_spectra's call (api_lattice.hip:
// plan, upload, projection) through the same run body (api_reciprocal.hip) with S species' series per vector: q is
// (kb, S, NC, T) and the segment buffer (nb, S, NC, ns, L).  This file adds the refusals that concern the species, the
// row table that holds S row, one projection launch per species -- that species' slice of the uploaded atom list, its own
// n_g, the q pointer advanced by a NC T -- and the choice of the pair passes after the FFT.  The result is
// (1 or 3, P, L, K or n_bins), P = S (S + 1) / 2.
#include "api_internal.h"

namespace psa {

namespace {

struct ParCall : LatCall {
    int                  S = 1;
    std::vector<int64_t> start;                      // (S + 1) the species' offsets into the atom list
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
    p->S = S;
    p->start.assign(species_start, species_start + S + 1);
    d.n_species = S;
    PSA_TRY(dynamic_plan(c, &d));
    PSA_TRY(lattice_plan(c, box_inverse, indices, bin_of, n_bins, S, p));
    PSA_REQUIRE((double)d.kb * S < (double)(1ll << 31), "a block of %lld vectors x %d species is more than the row table serves",
                (long long)d.kb, S);
    return PSA_OK;
}

// block b of the plan over all frames into d_q (nk, S, NC, T): one launch of the lattice kernel per species
BlockSource partial_source(psa_ctx* c, const ParCall& p, const int32_t* idx) {
    BlockSource src;
    src.upload = [c, &p, idx]() -> int { return lattice_upload(c, p, idx); };
    src.project = [c, &p](int64_t block, int64_t, int64_t, float2* d_q) -> int {
        for (int a = 0; a < p.S; ++a)
            PSA_TRY(lattice_project(c, p, true, p.start[(size_t)a], p.start[(size_t)a + 1] - p.start[(size_t)a], block,
                                    d_q + (size_t)a * (size_t)p.d.NC * (size_t)p.d.T));
        return PSA_OK;
    };
    return src;
}

int partial_run(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                const int32_t* idx, const int64_t* species_start, int32_t n_species, int32_t currents, float* out_host, size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    ParCall p;
    PSA_TRY(partial_check(c, box_inverse, indices, K, bin_of, n_bins, idx, species_start, n_species, currents, &p));
    SpectraRun a;
    a.src = partial_source(c, p, idx), a.pairs = true, a.n_bins = p.n_bins, a.out_host = out_host, a.out_bytes = out_bytes;
    return spectra_run(c, p.d, a);
}

// the projection alone: q (K, S, NC, T), rows in the caller's order
int partial_debug_project(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx,
                          const int64_t* species_start, int32_t n_species, int32_t currents, void* out_host) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    ParCall p;
    PSA_TRY(partial_check(c, box_inverse, indices, K, nullptr, 0, idx, species_start, n_species, currents, &p));
    return debug_project_run(c, p.d, partial_source(c, p, idx), out_host);
}

// the pair pass alone on transformed segments (K, S, NC, n_seg, L) of the caller's.  bin_of null: the per-vector form with
// the scale (float) (1 / norm); else the shell form
int partial_debug_power(psa_ctx* c, const void* seg_host, const float* khat, const int32_t* bin_of, int64_t K, int64_t n_bins,
                        int32_t n_species, int32_t currents, int64_t n_seg, int64_t L, int64_t k_block, int64_t seg_block, double norm,
                        float* out_host) {
    PSA_REQUIRE(seg_host != nullptr && out_host != nullptr && (khat != nullptr || !currents), "null argument");
    PSA_TRY(species_count(n_species));
    DebugPower a{.seg_host = seg_host, .bin_of = bin_of, .K = K, .n_bins = n_bins, .n_species = n_species, .currents = currents,
                 .n_seg = n_seg, .L = L, .k_block = k_block, .seg_block = seg_block, .norm = norm, .out_host = out_host};
    PSA_TRY(debug_power_check(&a));
    a.scale = (float)(1.0 / norm);
    return debug_power_run(c, a, khat);
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
