// psa_bond_persistence: the lifetimes of the bonds of the neighbour shells and of the cages they form, over time origins and
// lags (definition: include/psa_hip.h; kernels: persist.hip; host core: api_shell.h).  It is psa_angle_histogram's call with
// the tag pass and, per visited frame, a fraction pass and the step pass in place of the angle pass; a partial row holds the
// counters of every listed lag, one behind the other, so the one reduce of a block adds them all: behind the counts the tags,
// the two masks and the lagged fractions (288 n_a bytes per origin), inside the budget.
#include "api_shell.h"

namespace psa {

namespace {

// behind the counts of a block: the tags (64) int32, the survivor and the alive masks, the lagged fractions (3) float32 and 4
// bytes of padding
constexpr ShellLayout PERSIST_LAYOUT{4 * ANGLE_MAX_NEIGHBOURS, 8, 8, 12, 4};
static_assert(PERSIST_LAYOUT.bytes() == 288, "288 bytes per atom and origin");
static_assert(PERSIST_LAYOUT.bytes() % 8 == 0, "the work behind the counts is a multiple of 8 bytes per row");
// an item's samples of the step pass, 64 centres x the origins of its slab x 64 neighbours, fit 32 bits in every counter
static_assert((uint64_t)ANGLE_ITEM_CENTRES * ANGLE_MAX_SLAB * ANGLE_MAX_NEIGHBOURS < (1ull << 32), "an item's samples fit 32 bits");

struct PersistOut {
    uint64_t *bonds, *alive, *unbroken;
    size_t    pair_bytes;
    uint64_t* lost;
    size_t    lost_bytes;
    uint64_t* truncated;
    size_t    truncated_bytes;
    uint64_t *alive_masks, *unbroken_masks;
    size_t    masks_bytes;
};

int persist_run(ShellCall& s, const double* r_break, const int64_t* lags, int32_t n_lags, int64_t sample_step, int32_t continuous,
                const PersistOut& out) {
    PSA_REQUIRE(out.bonds != nullptr && out.alive != nullptr && out.unbroken != nullptr && out.lost != nullptr && out.truncated != nullptr,
                "null output");
    PSA_REQUIRE(lags != nullptr && r_break != nullptr, "null lags or r_break");
    PSA_REQUIRE(n_lags >= 1 && n_lags <= PERSIST_MAX_LAGS, "the number of lags is in [1, %d], got %d", PERSIST_MAX_LAGS, (int)n_lags);
    PSA_REQUIRE(sample_step >= 1, "sample_step must be at least 1, got %lld", (long long)sample_step);
    PSA_REQUIRE(continuous == 0 || continuous == 1, "continuous is 0 or 1, got %d", (int)continuous);
    PSA_TRY(shell_check(&s, "psa_bond_persistence", PERSIST_LAYOUT));
    psa_ctx*          c = s.c;
    const AtomGroups& p = s.p;
    const int         S = p.G, NC = ANGLE_MAX_NEIGHBOURS + 1;
    for (int j = 0; j < n_lags; ++j) {
        PSA_REQUIRE(lags[j] >= 0 && lags[j] <= p.T - 1, "lag %lld is outside [0, T - 1 = %lld]", (long long)lags[j], (long long)(p.T - 1));
        PSA_REQUIRE(j == 0 || lags[j] > lags[j - 1], "lags must be strictly ascending: lags[%d] = %lld after %lld", j, (long long)lags[j],
                    (long long)lags[j ? j - 1 : 0]);
        PSA_REQUIRE(lags[j] % sample_step == 0, "lag %lld is no multiple of sample_step = %lld", (long long)lags[j], (long long)sample_step);
    }
    AngleSpecies rb = s.sp;                                  // the species with float32(1 / r_break) in place of 1 / r_cut
    for (int a = 0; a < S; ++a)
        for (int b = 0; b < S; ++b) {
            const double r = r_break[a * S + b], rc = s.r_cut[a * S + b];
            PSA_REQUIRE(std::isfinite(r) && r >= rc, "r_break[%d][%d] = %g must be finite and at least r_cut[%d][%d] = %g", a, b, r, a, b, rc);
            PSA_TRY(cutoff_symmetric("r_break", r_break, S, a, b));
            PSA_REQUIRE((r == 0.0) == (rc == 0.0), "r_break[%d][%d] = %g and r_cut[%d][%d] = %g: one is 0 (no bond) and the other is not", a, b,
                        r, a, b, rc);
            PSA_TRY(cutoff_reciprocal(s.box_inverse, "r_break", a, b, r, &rb.inv_rc[a * S + b]));
        }
    const size_t pairs = (size_t)n_lags * (size_t)S * (size_t)S, want_p = pairs * sizeof(uint64_t);
    const size_t want_l = (size_t)n_lags * (size_t)S * (size_t)NC * sizeof(uint64_t), want_t = (size_t)n_lags * (size_t)S * sizeof(uint64_t);
    const size_t want_m = (size_t)n_lags * (size_t)s.n_o * (size_t)p.n_a * sizeof(uint64_t);
    PSA_REQUIRE(out.pair_bytes == want_p, "pair_bytes is %zu, each (%d,%d,%d) uint64 result has %zu", out.pair_bytes, (int)n_lags, S, S, want_p);
    PSA_REQUIRE(out.lost_bytes == want_l, "lost_bytes is %zu, the (%d,%d,%d) uint64 result has %zu", out.lost_bytes, (int)n_lags, S, NC, want_l);
    PSA_REQUIRE(out.truncated_bytes == want_t, "truncated_bytes is %zu, the (%d,%d) uint64 result has %zu", out.truncated_bytes, (int)n_lags, S,
                want_t);
    const bool masks = out.alive_masks != nullptr || out.unbroken_masks != nullptr;
    PSA_REQUIRE(!masks || out.masks_bytes == want_m, "masks_bytes is %zu, each (%d,%lld,%lld) uint64 per-atom result has %zu", out.masks_bytes,
                (int)n_lags, (long long)s.n_o, (long long)p.n_a, want_m);
    for (uint64_t* o : {out.bonds, out.alive, out.unbroken}) std::memset(o, 0, want_p);
    std::memset(out.lost, 0, want_l);
    std::memset(out.truncated, 0, want_t);
    for (uint64_t* o : {out.alive_masks, out.unbroken_masks})
        if (o != nullptr) std::memset(o, 0, want_m);         // a truncated centre, an origin outside O_tau: 0
    if (p.n_a == 0) return PSA_OK;                           // every species empty: zeros
    // the visited frames in ascending order and the listed lag each is (-1: none).  Continuous: every multiple of sample_step up
    // to the last lag (and lag 0 where it is listed: no test of it can fail); else the listed lags alone
    struct Visit { int64_t f; int j; };
    std::vector<Visit> visits;
    if (continuous) {
        int j = 0;
        if (lags[0] == 0) visits.push_back({0, j++});
        for (int64_t v = sample_step; v <= lags[n_lags - 1]; v += sample_step) {
            const bool listed = j < n_lags && lags[j] == v;
            visits.push_back({v, listed ? j : -1});
            j += listed;
        }
    } else {
        for (int j = 0; j < n_lags; ++j) visits.push_back({lags[j], j});
    }
    // a partial row and a species' accumulator row hold the counters of every lag, one behind the other: shell_run's one
    // reduce per block adds them all
    const int64_t row = persist_row_words(S), cols = (int64_t)n_lags * row, step = s.origin_step;
    const float*  d_pos = c->slot[PSA_SLOT_POSITIONS].buf.as<float>();
    std::vector<uint64_t> acc;
    const ShellPass       passes = [&](const AngleWork& wk, int64_t n_items, int64_t k0, int64_t nb) -> int {
        ShellCarve          cv = wk.carve();
        int*                d_tags = cv.take<int>();
        unsigned long long* d_surv = cv.take<unsigned long long>();
        unsigned long long* d_alive = cv.take<unsigned long long>();
        float*              d_cl = cv.take<float>();
        unsigned*           d_part = c->d_rs_part.as<unsigned>();
        // a lag none of whose origins lies in this block is not visited: its counters are zeros
        PSA_HIP_CHECK(hipMemsetAsync(d_part, 0, (size_t)n_items * (size_t)cols * sizeof(uint32_t), c->stream));
        PSA_TRY(launch_persist_tags(c, wk.count, wk.list, d_tags, d_surv, p.n_a, nb));
        for (const Visit& v : visits) {
            // the origins of the block with o + f <= T - 1: a prefix, shorter with every later frame
            const int64_t n_f = std::min(nb, (p.T - 1 - v.f) / step + 1 - k0);
            if (n_f <= 0) break;
            PSA_TRY(launch_pair_frac(c, d_pos, p.d_idx, p.n_a, s.box_inverse, d_cl, k0 * step + v.f, step, n_f, p.T, p.N));
            PSA_TRY(launch_persist_step(c, wk.count, d_tags, c->d_rs_items.ptr, n_items, d_cl, d_surv, d_alive,
                                        v.j >= 0 ? d_part + (size_t)v.j * (size_t)row : nullptr, cols, rb, s.box, p.n_a, n_f, continuous != 0));
            if (v.j < 0 || !masks) continue;
            const size_t lag_at = (size_t)v.j * (size_t)s.n_o * (size_t)p.n_a;
            PSA_TRY(copy_atom_rows(c, p.n_a, k0, n_f, {{out.alive_masks ? out.alive_masks + lag_at : nullptr, d_alive, sizeof(uint64_t)},
                                                       {out.unbroken_masks && continuous ? out.unbroken_masks + lag_at : nullptr, d_surv,
                                                        sizeof(uint64_t)}}));
        }
        return PSA_OK;
    };
    PSA_TRY(shell_run(s, cols, PERSIST_LAYOUT, passes, nullptr, &acc));
    for (int j = 0; j < n_lags; ++j)
        for (int a = 0; a < S; ++a) {
            const uint64_t* r = acc.data() + ((size_t)a * (size_t)n_lags + (size_t)j) * (size_t)row;
            const size_t    at = ((size_t)j * (size_t)S + (size_t)a) * (size_t)S;
            std::memcpy(out.bonds + at, r, (size_t)S * sizeof(uint64_t));
            std::memcpy(out.alive + at, r + S, (size_t)S * sizeof(uint64_t));
            std::memcpy(out.unbroken + at, r + 2 * S, (size_t)S * sizeof(uint64_t));
            std::memcpy(out.lost + ((size_t)j * (size_t)S + (size_t)a) * (size_t)NC, r + 3 * S, (size_t)NC * sizeof(uint64_t));
            out.truncated[(size_t)j * (size_t)S + (size_t)a] = r[(size_t)row - 1];
        }
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_bond_persistence(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                         int32_t n_groups, const double* r_cut, const double* r_break, int64_t origin_step, const int64_t* lags,
                         int32_t n_lags, int64_t sample_step, int32_t continuous, uint64_t* bonds, uint64_t* alive, uint64_t* unbroken,
                         size_t pair_bytes, uint64_t* lost, size_t lost_bytes, uint64_t* truncated, size_t truncated_bytes,
                         uint64_t* alive_masks, uint64_t* unbroken_masks, size_t masks_bytes) {
    PSA_TRY(enter(c));
    Guard            guard(c);
    ShellCall        s{c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step};
    const PersistOut out{bonds, alive, unbroken, pair_bytes, lost, lost_bytes, truncated, truncated_bytes, alive_masks, unbroken_masks, masks_bytes};
    return synchronised(c, persist_run(s, r_break, lags, n_lags, sample_step, continuous, out), "psa_bond_persistence");
}

}  // extern "C"
