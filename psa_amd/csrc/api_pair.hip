// psa_pair_histogram, psa_debug_pair_fractions: the histogram of minimum-image pair distances between species over time
// origins -- g(r), its partials and the distinct van Hove function (definition: include/psa_hip.h; kernels: pair.hip).
// Only the positions slot is read; atom weights and segments set on the context are ignored; nothing of the other entry
// points' state is touched.
//
// Budget (PSA_OPT_DYNAMIC_WORK_BYTES = W): the centred fractional coordinates of the listed atoms at a block of origin
// frames and at their partner frames, 24 n_a bytes per origin; a block is a whole number of origins, W / (24 n_a) of
// them, and a budget below one origin is refused.  The item table, the partials, the accumulator and the result lie
// outside it.  Per lag and block: the fraction pass (twice for tau > 0), the pair kernel over the items, the reduce into
// the accumulator that lives across blocks and lags.
#include "api_internal.h"

namespace psa {

namespace {

constexpr int64_t PAIR_MAX_RUN = 256;           // most beta-tiles of an item

int pair_check(psa_ctx* c, const char* entry, const double* box, const double* box_inverse, const int32_t* idx,
               const int64_t* group_start, int32_t n_groups, AtomGroups* p) {
    PSA_TRY(group_list_check(c, entry, box, box_inverse, idx, group_start, n_groups, p));
    const int64_t W = c->opt_dynamic_work_bytes, per_origin = 24 * std::max<int64_t>(p->n_a, 1);
    PSA_REQUIRE(W / per_origin >= 1, "the work budget of %lld bytes (PSA_OPT_DYNAMIC_WORK_BYTES) cannot hold the smallest block: the "
                "fractional coordinates of %lld atoms at an origin and at its partner frame need %lld bytes", (long long)W,
                (long long)p->n_a, (long long)per_origin);
    p->Ab = W / per_origin;                                  // origins of a block
    return PSA_OK;
}

// The items of a launch over n_ob origins, species pair by species pair; rows: the items the reduce sums into (alpha, beta).
// sym (tau = 0): items for alpha <= beta only, alpha = beta the upper triangle of tiles -- the items of (min, max) serve
// both orders, and alpha = beta counts every evaluated pair twice.  An item's samples -- PAIR_TILE alpha-atoms x its
// beta-atoms x its origins -- stay below 2^32: run x origins per slab <= 65535.
std::vector<PairItem> pair_items(const AtomGroups& p, bool sym, int64_t n_ob, HistRows* rows) {
    const int S = p.G;
    const auto tiles = [&](int g) { return (p.size[(size_t)g] + PAIR_TILE - 1) / PAIR_TILE; };
    int64_t tile_pairs = 0;
    for (int a = 0; a < S; ++a)
        for (int b = sym ? a : 0; b < S; ++b) tile_pairs += sym && a == b ? tiles(a) * (tiles(a) + 1) / 2 : tiles(a) * tiles(b);
    const int64_t run = std::max<int64_t>(1, std::min(PAIR_MAX_RUN, tile_pairs / REALSPACE_TARGET_GROUPS));
    int64_t       n_os = std::max<int64_t>(1, std::min(n_ob, REALSPACE_TARGET_GROUPS / std::max<int64_t>(1, tile_pairs / run)));
    const int64_t per_slab = 65535 / run;                    // most origins of a slab: per_slab run <= 65535
    n_os = std::max(n_os, (n_ob + per_slab - 1) / per_slab);  // the least n_os with ceil(n_ob / n_os) <= per_slab
    std::vector<PairItem> items;
    for (int a = 0; a < S; ++a)
        for (int b = 0; b < S; ++b) {
            const int out = a * S + b, twin = b * S + a;
            rows->factor[out] = sym && a == b ? 2 : 1;
            if (sym && b < a) {                              // the items of (beta, alpha), listed before
                rows->lo[out] = rows->lo[twin], rows->hi[out] = rows->hi[twin];
                continue;
            }
            rows->lo[out] = (int)items.size();
            for (int64_t i = 0; i < tiles(a); ++i)
                for (int64_t j = sym && a == b ? i : 0; j < tiles(b); j += run)
                    for (int64_t slab = 0; slab < n_os; ++slab) {
                        PairItem it;
                        it.a_lo = (int)(p.start[(size_t)a] + i * PAIR_TILE);
                        it.a_n = (int)std::min<int64_t>(PAIR_TILE, p.start[(size_t)a + 1] - it.a_lo);
                        it.b_lo = (int)(p.start[(size_t)b] + j * PAIR_TILE);
                        it.b_hi = (int)std::min(p.start[(size_t)b] + (j + run) * PAIR_TILE, p.start[(size_t)b + 1]);
                        it.slab = (int)slab, it.n_os = (int)n_os;
                        it.diag = a == b ? (sym ? 1 : 2) : 0;
                        it.pair = a * S + b;
                        items.push_back(it);
                    }
            rows->hi[out] = (int)items.size();
        }
    return items;
}

int pair_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
             const int64_t* lags, int64_t n_vh, int64_t origin_step, double dr, int32_t n_r, uint64_t* out_host, size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr && lags != nullptr, "null output or lags");
    AtomGroups p;
    PSA_TRY(pair_check(c, "psa_pair_histogram", box, box_inverse, idx, group_start, n_groups, &p));
    float inv_dr;
    PSA_TRY(histogram_args_check(p, lags, n_vh, PAIR_MAX_LAGS, origin_step, dr, n_r, PAIR_MAX_BINS, &inv_dr));
    PSA_TRY(served_radius_check(box_inverse, "r_max = n_r dr", (double)n_r * dr));
    const int    S = p.G;
    const size_t per_lag = (size_t)S * (size_t)S * (size_t)(n_r + 1) * sizeof(uint64_t), want = (size_t)n_vh * per_lag;
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%lld,%d,%d,%d) uint64 result has %zu", out_bytes, (long long)n_vh, S, S,
                (int)(n_r + 1), want);
    if (p.n_a == 0) {                                        // every species empty: zeros
        std::memset(out_host, 0, out_bytes);
        return PSA_OK;
    }
    PSA_TRY(upload_atom_list(c, &p, idx));
    PSA_TRY(c->d_rs_acc.reserve(want));
    PSA_HIP_CHECK(hipMemsetAsync(c->d_rs_acc.ptr, 0, want, c->stream));
    const float* d_pos = c->slot[PSA_SLOT_POSITIONS].buf.as<float>();
    for (int64_t j = 0; j < n_vh; ++j) {
        const int64_t tau = lags[j], n_o = (p.T - 1 - tau) / origin_step + 1;
        const bool    sym = tau == 0;
        const int64_t B = std::min<int64_t>({n_o, p.Ab, 65535});            // origins of a block (the fraction pass's grid holds 65535)
        HistRows      rows;
        const std::vector<PairItem> items = pair_items(p, sym, B, &rows);
        if (items.empty()) continue;
        PSA_TRY(upload(c, c->d_rs_items, items.data(), items.size() * sizeof(PairItem)));
        PSA_TRY(c->d_rs_part.reserve(items.size() * (size_t)(n_r + 1) * sizeof(uint32_t)));
        PSA_TRY(c->d_pair_c.reserve((size_t)(sym ? 1 : 2) * (size_t)B * 3 * (size_t)p.n_a * sizeof(float)));
        for (int64_t k0 = 0; k0 < n_o; k0 += B) {
            const int64_t nb = std::min(B, n_o - k0);
            float*        cA = c->d_pair_c.as<float>(), *cB = sym ? cA : cA + nb * 3 * p.n_a;
            {
                StageTimer st(c, PSA_T_GATHER);
                PSA_TRY(launch_pair_frac(c, d_pos, p.d_idx, p.n_a, box_inverse, cA, k0 * origin_step, origin_step, nb, p.T, p.N));
                if (!sym) PSA_TRY(launch_pair_frac(c, d_pos, p.d_idx, p.n_a, box_inverse, cB, k0 * origin_step + tau, origin_step, nb, p.T, p.N));
            }
            {
                StageTimer st(c, PSA_T_TRANSPOSE);
                PSA_TRY(launch_pair_hist(c, cA, cB, c->d_rs_items.ptr, (int64_t)items.size(), c->d_rs_part.as<unsigned>(), box, p.n_a,
                                         nb, inv_dr, n_r));
            }
            StageTimer st(c, PSA_T_EPILOGUE);
            PSA_TRY(launch_hist_reduce(c, c->d_rs_part.as<unsigned>(), rows, S * S, 1, n_r + 1,
                                       c->d_rs_acc.as<unsigned long long>() + (size_t)j * (per_lag / sizeof(uint64_t))));
        }
    }
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_rs_acc.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the item table alone, on the host: {beta-tiles of a run, origin slabs, items, the most samples of an item}
int debug_plan_run(const int64_t* sizes, int32_t S, int32_t sym, int64_t n_ob, int64_t* out) {
    PSA_REQUIRE(sizes != nullptr && out != nullptr, "null sizes or output");
    PSA_REQUIRE(S >= 1 && S <= PAIR_MAX_SPECIES && n_ob >= 1 && n_ob <= 65535 && (sym == 0 || sym == 1), "bad plan arguments");
    AtomGroups p;
    p.G = S, p.start = {0};
    for (int g = 0; g < S; ++g) {
        PSA_REQUIRE(sizes[g] >= 0 && p.start.back() + sizes[g] < (1ll << 31), "bad species size");
        p.size.push_back(sizes[g]);
        p.start.push_back(p.start.back() + sizes[g]);
    }
    HistRows                    rows;
    const std::vector<PairItem> items = pair_items(p, sym != 0, n_ob, &rows);
    out[0] = out[1] = out[3] = 0, out[2] = (int64_t)items.size();
    for (const PairItem& it : items) {
        const int64_t origins = it.slab < n_ob ? (n_ob - 1 - it.slab) / it.n_os + 1 : 0;
        out[0] = std::max<int64_t>(out[0], (it.b_hi - it.b_lo + PAIR_TILE - 1) / PAIR_TILE);
        out[1] = it.n_os;
        out[3] = std::max(out[3], (int64_t)PAIR_TILE * (it.b_hi - it.b_lo) * origins);   // lanes past a_n count nothing: an upper bound
    }
    return PSA_OK;
}

// the fraction pass alone, frame block by frame block under the same budget rule: c (T, n_g, 3) float32
int debug_fractions_run(psa_ctx* c, const double* box_inverse, const int32_t* idx, int64_t n_g, float* out) {
    PSA_REQUIRE(out != nullptr && box_inverse != nullptr, "null output or box_inverse");
    PSA_REQUIRE(idx == nullptr || (n_g >= 0 && n_g < (1ll << 31)), "bad number of atoms %lld", (long long)n_g);
    double H[9], det;                                        // the box of this inverse, for the shared checks
    PSA_TRY(invertible_check(box_inverse, "box_inverse", &det));
    inverse3(box_inverse, det, H);
    const int64_t start[2] = {0, n_g};
    AtomGroups       p;
    PSA_TRY(pair_check(c, "psa_debug_pair_fractions", H, box_inverse, idx, start, 1, &p));
    if (p.n_a == 0) return PSA_OK;
    PSA_TRY(upload_atom_list(c, &p, idx));
    const int64_t      Bf = std::min<int64_t>({p.T, 2 * p.Ab, 65535});
    std::vector<float> h;
    PSA_TRY(c->d_pair_c.reserve((size_t)Bf * 3 * (size_t)p.n_a * sizeof(float)));
    for (int64_t f0 = 0; f0 < p.T; f0 += Bf) {
        const int64_t nf = std::min(Bf, p.T - f0);
        const size_t  n = (size_t)nf * 3 * (size_t)p.n_a;
        PSA_TRY(launch_pair_frac(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(), p.d_idx, p.n_a, box_inverse, c->d_pair_c.as<float>(), f0, 1, nf, p.T, p.N));
        h.resize(n);
        PSA_HIP_CHECK(hipMemcpyAsync(h.data(), c->d_pair_c.ptr, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
        for (int64_t f = 0; f < nf; ++f)
            for (int j = 0; j < 3; ++j)
                for (int64_t a = 0; a < p.n_a; ++a)
                    out[((size_t)(f0 + f) * (size_t)p.n_a + (size_t)a) * 3 + (size_t)j] = h[((size_t)f * 3 + (size_t)j) * (size_t)p.n_a + (size_t)a];
    }
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_pair_histogram(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                       int32_t n_groups, const int64_t* lags, int64_t n_lags, int64_t origin_step, double dr, int32_t n_r,
                       uint64_t* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, pair_run(c, box, box_inverse, idx, group_start, n_groups, lags, n_lags, origin_step, dr, n_r, out_host, out_bytes),
                        "psa_pair_histogram");
}

int psa_debug_pair_plan(const int64_t* sizes, int32_t n_groups, int32_t sym, int64_t n_origins, int64_t* out) {
    return debug_plan_run(sizes, n_groups, sym, n_origins, out);
}

int psa_debug_pair_fractions(psa_ctx* c, const double* box_inverse, const int32_t* idx, int64_t n_g, float* out) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, debug_fractions_run(c, box_inverse, idx, n_g, out), "psa_debug_pair_fractions");
}

}  // extern "C"
