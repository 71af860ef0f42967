// psa_angle_histogram, psa_debug_neighbour_lists, psa_bond_order, psa_local_order, psa_debug_qlm, psa_solid_clusters,
// psa_debug_cluster_labels, psa_bond_persistence, psa_common_neighbours: the bond-angle
// distributions of species triplets, the coordination statistics of species pairs, the Steinhardt order parameters q_l and
// the local order parameters (q-bar_l, w_l, solid-like bonds) of the neighbour shells over time origins (definition:
// include/psa_hip.h; kernels: angle.hip, order.hip, qlm.hip -- their shared parts in shell.h -- and pair.hip's fraction
// pass).  Only the positions slot is read; atom weights and segments set on the context are ignored; nothing of the other
// entry points' state is touched.
//
// Budget (PSA_OPT_DYNAMIC_WORK_BYTES = W): per origin of a block the centred fractional coordinates of the listed atoms
// (12 n_a bytes), their neighbour counts (4 n_a) and their neighbour lists (64 x 16 n_a): 1040 n_a bytes; a block is a
// whole number of origins, W / (1040 n_a) of them, and a budget below one origin is refused.  The item table, the bin
// edges, the partials, the accumulator and the result lie outside it.  Per block: the fraction pass, the neighbour pass,
// the angle pass over the items, the reduce into the accumulator that lives across blocks.
//
// psa_bond_order (kernel: order.hip) is the same call with the order pass in place of the angle pass: the same checks, work
// buffer, items and reduce; with per-atom output the block's X (8 n_l n_a bytes per origin) lies behind the counts, inside
// the budget, and every block's X and counts are copied to the caller's arrays before the next block overwrites them.
//
// psa_local_order and psa_debug_qlm (kernels: qlm.hip) are the same call again with two passes in place of the angle pass:
// the first leaves the table of the Q_lm (16 sum (l + 1) n_a bytes per origin) behind the counts, the second gathers from
// it; the per-atom rows ((24 n_l + 8) n_a bytes per origin) lie behind the table, all inside the budget.
//
// psa_solid_clusters (kernels: cluster.hip) is that call with the q_lm pass of the one order solid_l and the four cluster
// passes: behind the table the masks, xi, parent / label and size (20 n_a bytes per origin), inside the budget; the size
// histogram, the error word and the per-origin results ride behind the species' rows of the accumulator.
// psa_debug_cluster_labels drives the hook, flatten and stats passes alone on a graph of the caller's.
//
// psa_bond_persistence (kernels: persist.hip) is the call with the tag pass and, per visited frame, a fraction pass and the
// step pass in place of the angle pass; a partial row holds the counters of every listed lag, one behind the other, so the
// one reduce of a block adds them all: behind the counts the tags, the two masks and the lagged fractions (288 n_a bytes per
// origin), inside the budget.
//
// psa_common_neighbours (kernels: cna.hip) is the call with the signature pass and the census pass in place of the angle pass:
// behind the counts the types (8 n_a bytes per origin with their padding) and, where the per-bond output is asked for, the
// signatures (256 n_a), inside the budget; the per-origin type counts ride behind the species' rows of the accumulator.
#include "api_internal.h"

namespace psa {

namespace {

constexpr int64_t ANGLE_ITEM_CENTRES = 64;      // centres of an item of the angle pass: 16 per wavefront and origin
constexpr int64_t ANGLE_PART_BYTES = 64 << 20;  // what the items' partials aim to stay below
// most origins of an item: 64 centres x 8192 origins x 2016 pairs of 64 neighbours stay below 2^32
constexpr int64_t ANGLE_MAX_SLAB = 8192;
static_assert((uint64_t)ANGLE_ITEM_CENTRES * ANGLE_MAX_SLAB * (ANGLE_MAX_NEIGHBOURS * (ANGLE_MAX_NEIGHBOURS - 1) / 2) < (1ull << 32),
              "an item's samples fit 32 bits");
constexpr int64_t ANGLE_ORIGIN_BYTES = 12 + 4 + 16 * ANGLE_MAX_NEIGHBOURS;   // per atom and origin

// the shared checks, the cut-offs, the budget (extra: bytes per atom and origin behind the counts) and origin_step (1 for
// the entries of one frame); fills p and sp.  p->Ab: the origins of a block, as many of the origins 0, origin_step, ... as
// the budget and the fraction pass's grid (65535) hold -- the one place that decides it
int angle_check(psa_ctx* c, const char* entry, const double* box, const double* box_inverse, const int32_t* idx,
                const int64_t* group_start, int32_t n_groups, const double* r_cut, int64_t origin_step, AtomGroups* p, AngleSpecies* sp,
                int64_t extra = 0) {
    PSA_TRY(group_list_check(c, entry, box, box_inverse, idx, group_start, n_groups, p));
    PSA_REQUIRE(r_cut != nullptr, "null r_cut");
    const int    S = p->G;
    *sp = AngleSpecies{};
    sp->S = S;
    for (int a = 0; a < S; ++a)
        for (int b = 0; b < S; ++b) {
            const double r = r_cut[a * S + b];
            PSA_REQUIRE(std::isfinite(r) && r >= 0.0, "r_cut[%d][%d] must be finite and not negative, got %g", a, b, r);
            PSA_REQUIRE(r == r_cut[b * S + a], "r_cut is not symmetric: [%d][%d] = %.17g, [%d][%d] = %.17g", a, b, r, b, a, r_cut[b * S + a]);
            char what[32];
            std::snprintf(what, sizeof what, "r_cut[%d][%d]", a, b);
            PSA_TRY(served_radius_check(box_inverse, what, r));
            const float inv = r > 0.0 ? (float)(1.0 / r) : 0.f;
            PSA_REQUIRE(r == 0.0 || (std::isfinite(inv) && inv > 0.f), "r_cut[%d][%d] = %g has no float32 reciprocal", a, b, r);
            sp->inv_rc[a * S + b] = inv;
        }
    PSA_REQUIRE(p->n_a < (1ll << ANGLE_SPECIES_SHIFT), "at most 2^%d - 1 listed atoms are served, got %lld", ANGLE_SPECIES_SHIFT,
                (long long)p->n_a);
    for (int g = 0; g <= S; ++g) sp->start[g] = (int)p->start[(size_t)g];
    for (int g = 0; g < S; ++g) sp->tile_first[g + 1] = sp->tile_first[g] + (int)((p->size[(size_t)g] + ANGLE_CENTRES - 1) / ANGLE_CENTRES);
    const int64_t W = c->opt_dynamic_work_bytes, per_origin = (ANGLE_ORIGIN_BYTES + extra) * std::max<int64_t>(p->n_a, 1);
    PSA_REQUIRE(W / per_origin >= 1, "the work budget of %lld bytes (PSA_OPT_DYNAMIC_WORK_BYTES) cannot hold the smallest block: the "
                "fractional coordinates, neighbour counts and neighbour lists of %lld atoms at one origin need %lld bytes", (long long)W,
                (long long)p->n_a, (long long)per_origin);
    PSA_REQUIRE(origin_step >= 1, "origin_step must be at least 1, got %lld", (long long)origin_step);
    p->Ab = std::min<int64_t>({(p->T - 1) / origin_step + 1, W / per_origin, 65535});
    return PSA_OK;
}

// the work buffer of a block of B origins: the lists first (16-byte entries), then c, then the counts, then `extra` bytes
// per atom and origin (a multiple of 8: psa_bond_order's X)
struct AngleWork {
    float4*    list;
    float*     c;
    int*       count;
    long long* x;
};
int angle_work(psa_ctx* c, int64_t n_a, int64_t B, AngleWork* w, int64_t extra = 0) {
    const size_t rows = (size_t)B * (size_t)n_a;
    PSA_TRY(c->d_angle_work.reserve(rows * (size_t)(ANGLE_ORIGIN_BYTES + extra)));
    char* base = static_cast<char*>(c->d_angle_work.ptr);
    w->list = reinterpret_cast<float4*>(base);
    w->c = reinterpret_cast<float*>(base + rows * 16 * ANGLE_MAX_NEIGHBOURS);
    w->count = reinterpret_cast<int*>(base + rows * (16 * ANGLE_MAX_NEIGHBOURS + 12));
    w->x = extra ? reinterpret_cast<long long*>(base + rows * (size_t)ANGLE_ORIGIN_BYTES) : nullptr;
    return PSA_OK;
}

// The items of the angle pass over n_ob origins, species by species, ANGLE_ITEM_CENTRES centres each; first (S + 1): where
// each species' items begin.  The partials (items x row words) stay below ANGLE_PART_BYTES where one slab per tile allows
std::vector<AngleItem> angle_items(const AtomGroups& p, int64_t n_ob, int64_t row, int32_t* first) {
    int64_t tiles = 0;
    for (int g = 0; g < p.G; ++g) tiles += (p.size[(size_t)g] + ANGLE_ITEM_CENTRES - 1) / ANGLE_ITEM_CENTRES;
    const int64_t target = std::max<int64_t>(1, std::min(REALSPACE_TARGET_GROUPS, ANGLE_PART_BYTES / (row * (int64_t)sizeof(uint32_t))));
    int64_t       n_os = std::max<int64_t>(1, std::min(n_ob, target / std::max<int64_t>(1, tiles)));
    n_os = std::max(n_os, (n_ob + ANGLE_MAX_SLAB - 1) / ANGLE_MAX_SLAB);
    std::vector<AngleItem> items;
    for (int g = 0; g < p.G; ++g) {
        first[g] = (int32_t)items.size();
        for (int64_t lo = p.start[(size_t)g]; lo < p.start[(size_t)g + 1]; lo += ANGLE_ITEM_CENTRES)
            for (int64_t slab = 0; slab < n_os; ++slab)
                items.push_back(AngleItem{(int)lo, (int)std::min<int64_t>(ANGLE_ITEM_CENTRES, p.start[(size_t)g + 1] - lo), g, (int)slab, (int)n_os});
    }
    first[p.G] = (int32_t)items.size();
    return items;
}

// What a call on the neighbour shells runs after its checks (angle_run, order_run): the item table over the origins of a
// block, the uploads of the atom list and the table, the accumulator (S, row) zeroed; per block the fraction pass, the
// neighbour pass, the caller's `pass` over the items into the partials, the reduce, and `after` where the caller has
// something to take out of the block before the next one overwrites it; at the end the accumulator on the host.
// extra: bytes per atom and origin behind the counts (AngleWork::x); tail: uint64 words of the caller's behind the species'
// rows of the accumulator, zeroed and returned with them
using ShellPass = std::function<int(const AngleWork& w, int64_t n_items, int64_t k0, int64_t nb)>;
int shell_run(psa_ctx* c, AtomGroups& p, const AngleSpecies& sp, const int32_t* idx, const double* box, const double* box_inverse,
              int64_t origin_step, int64_t row, int64_t extra, const ShellPass& pass, const ShellPass& after, std::vector<uint64_t>* acc,
              int64_t tail = 0) {
    const int     S = p.G;
    const int64_t n_o = (p.T - 1) / origin_step + 1, B = p.Ab;
    int32_t                      first[PAIR_MAX_SPECIES + 1];
    const std::vector<AngleItem> items = angle_items(p, B, row, first);
    AngleWork                    w;
    HistRows                     rows;
    PSA_TRY(rows_of_groups(first, S, 1, &rows));
    PSA_TRY(upload_atom_list(c, &p, idx));
    {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_rs_items, items.data(), items.size() * sizeof(AngleItem)));
    }
    PSA_TRY(c->d_rs_part.reserve(items.size() * (size_t)row * sizeof(uint32_t)));
    const size_t acc_words = (size_t)S * (size_t)row + (size_t)tail;
    PSA_TRY(c->d_rs_acc.reserve(acc_words * sizeof(uint64_t)));
    PSA_HIP_CHECK(hipMemsetAsync(c->d_rs_acc.ptr, 0, acc_words * sizeof(uint64_t), c->stream));
    PSA_TRY(angle_work(c, p.n_a, B, &w, extra));
    const float* d_pos = c->slot[PSA_SLOT_POSITIONS].buf.as<float>();
    for (int64_t k0 = 0; k0 < n_o; k0 += B) {
        const int64_t nb = std::min(B, n_o - k0);
        {
            StageTimer st(c, PSA_T_GATHER);
            PSA_TRY(launch_pair_frac(c, d_pos, p.d_idx, p.n_a, box_inverse, w.c, k0 * origin_step, origin_step, nb, p.T, p.N));
        }
        {
            StageTimer st(c, PSA_T_TRANSPOSE);
            PSA_TRY(launch_angle_neighbours(c, w.c, w.count, w.list, sp, box, p.n_a, nb));
        }
        {
            StageTimer st(c, PSA_T_PHASE);
            PSA_TRY(pass(w, (int64_t)items.size(), k0, nb));
        }
        {
            StageTimer st(c, PSA_T_EPILOGUE);
            PSA_TRY(launch_hist_reduce(c, c->d_rs_part.as<unsigned>(), rows, S, 1, row, c->d_rs_acc.as<unsigned long long>()));
        }
        if (after) PSA_TRY(after(w, (int64_t)items.size(), k0, nb));
    }
    acc->resize(acc_words);
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(acc->data(), c->d_rs_acc.ptr, acc->size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// A block's per-atom rows to the caller's arrays: per output the caller's array over all origins (null: not asked for), the
// block's rows on the device and the bytes of a cell, one per (origin, atom)
struct AtomRows { void* host; const void* dev; size_t cell; };
int copy_atom_rows(psa_ctx* c, int64_t n_a, int64_t k0, int64_t nb, std::initializer_list<AtomRows> rows) {
    StageTimer   st(c, PSA_T_D2H);
    const size_t at = (size_t)k0 * (size_t)n_a, cells = (size_t)nb * (size_t)n_a;
    for (const AtomRows& r : rows)
        if (r.host != nullptr)
            PSA_HIP_CHECK(hipMemcpyAsync(static_cast<char*>(r.host) + at * r.cell, r.dev, cells * r.cell, hipMemcpyDeviceToHost, c->stream));
    return PSA_OK;
}

// The orders of a call: 1 to `most` of them, each in [lowest, ORDER_MAX_L] and with `even` not odd, strictly ascending; fills
// o but solid_l (mask: bit l set for every order, columns: the sum of l + 1)
int ascending_orders(const int32_t* ls, int32_t n_ls, int most, int lowest, bool even, LocalLs* o) {
    PSA_REQUIRE(ls != nullptr, "null ls");
    PSA_REQUIRE(n_ls >= 1 && n_ls <= most, "the number of orders is in [1, %d], got %d", most, (int)n_ls);
    *o = LocalLs{(int)n_ls, (int)ls[n_ls - 1], 0, 0, 0u};
    for (int j = 0; j < n_ls; ++j) {
        PSA_REQUIRE(ls[j] >= lowest && ls[j] <= ORDER_MAX_L, "ls[%d] = %d is outside [%d, %d]", j, (int)ls[j], lowest, ORDER_MAX_L);
        PSA_REQUIRE(!even || ls[j] % 2 == 0, "ls[%d] = %d is odd: the 3j symbol (l l l; m1 m2 m3) is antisymmetric under an exchange of two "
                    "columns for odd l, so W_l vanishes identically; only even orders are served", j, (int)ls[j]);
        PSA_REQUIRE(j == 0 || ls[j] > ls[j - 1], "ls must be strictly ascending: ls[%d] = %d after %d", j, (int)ls[j], (int)ls[j ? j - 1 : 0]);
        o->mask |= 1u << ls[j];
        o->columns += ls[j] + 1;
    }
    return PSA_OK;
}

int angle_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
              const double* r_cut, int64_t origin_step, int32_t n_theta, uint64_t* angles, size_t angles_bytes, uint64_t* coord,
              size_t coord_bytes, uint64_t* truncated) {
    PSA_REQUIRE(angles != nullptr && coord != nullptr && truncated != nullptr, "null output");
    AtomGroups   p;
    AngleSpecies sp;
    PSA_TRY(angle_check(c, "psa_angle_histogram", box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, &p, &sp));
    PSA_REQUIRE(n_theta >= 1 && n_theta <= ANGLE_MAX_BINS, "the number of bins is in [1, %d], got %d", ANGLE_MAX_BINS, (int)n_theta);
    const int    S = p.G, P = S * (S + 1) / 2, n1 = n_theta + 1, NC = ANGLE_MAX_NEIGHBOURS + 1;
    const size_t want_a = (size_t)S * (size_t)P * (size_t)n1 * sizeof(uint64_t), want_c = (size_t)S * (size_t)S * (size_t)NC * sizeof(uint64_t);
    PSA_REQUIRE(angles_bytes == want_a, "angles_bytes is %zu, the (%d,%d,%d) uint64 result has %zu", angles_bytes, S, P, n1, want_a);
    PSA_REQUIRE(coord_bytes == want_c, "coord_bytes is %zu, the (%d,%d,%d) uint64 result has %zu", coord_bytes, S, S, NC, want_c);
    std::memset(angles, 0, want_a);
    std::memset(coord, 0, want_c);
    std::memset(truncated, 0, (size_t)S * sizeof(uint64_t));
    if (p.n_a == 0) return PSA_OK;                           // every species empty: zeros
    const int64_t      row = angle_row_words(S, n_theta);
    std::vector<float> edges((size_t)n1);
    for (int i = 0; i < n1; ++i) edges[(size_t)i] = (float)std::cos((double)i * M_PI / (double)n_theta);
    edges[0] = 1.f, edges[(size_t)n_theta] = -1.f;
    {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_angle_edges, edges.data(), edges.size() * sizeof(float)));
    }
    std::vector<uint64_t> acc;
    PSA_TRY(shell_run(c, p, sp, idx, box, box_inverse, origin_step, row, 0, [&](const AngleWork& w, int64_t n_items, int64_t, int64_t nb) -> int {
        return launch_angle_hist(c, w.count, w.list, c->d_rs_items.ptr, n_items, c->d_angle_edges.as<float>(), c->d_rs_part.as<unsigned>(), S,
                                 p.n_a, nb, n_theta);
    }, nullptr, &acc));
    for (int a = 0; a < S; ++a) {
        const uint64_t* r = acc.data() + (size_t)a * (size_t)row;
        std::memcpy(angles + (size_t)a * (size_t)P * (size_t)n1, r, (size_t)P * (size_t)n1 * sizeof(uint64_t));
        std::memcpy(coord + (size_t)a * (size_t)S * (size_t)NC, r + (size_t)P * (size_t)n1, (size_t)S * (size_t)NC * sizeof(uint64_t));
        truncated[a] = r[(size_t)row - 1];
    }
    return PSA_OK;
}

// an item's samples of the order pass, 64 centres x the origins of a block x n_l, fit 32 bits whatever the slabs
static_assert((uint64_t)ANGLE_ITEM_CENTRES * 65535 * ORDER_MAX_LS < (1ull << 32), "an item's samples fit 32 bits");

int order_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
              const double* r_cut, int64_t origin_step, const int32_t* ls, int32_t n_ls, int32_t n_q, uint64_t* hist, size_t hist_bytes,
              uint64_t* truncated, uint64_t* isolated, uint64_t* undefined, int64_t* x, int32_t* n) {
    PSA_REQUIRE(hist != nullptr && truncated != nullptr && isolated != nullptr && undefined != nullptr, "null output");
    LocalLs all;
    PSA_TRY(ascending_orders(ls, n_ls, ORDER_MAX_LS, 1, false, &all));
    const OrderLs o{all.n_l, all.l_max, all.mask};
    const int64_t extra = x != nullptr ? 8 * (int64_t)n_ls : 0;
    AtomGroups    p;
    AngleSpecies  sp;
    PSA_TRY(angle_check(c, "psa_bond_order", box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, &p, &sp, extra));
    PSA_REQUIRE(n_q >= 1 && n_q <= ORDER_MAX_BINS, "the number of bins is in [1, %d], got %d", ORDER_MAX_BINS, (int)n_q);
    const int    S = p.G;
    const size_t bins = (size_t)n_ls * (size_t)n_q, want = (size_t)S * bins * sizeof(uint64_t);
    PSA_REQUIRE(hist_bytes == want, "hist_bytes is %zu, the (%d,%d,%d) uint64 result has %zu", hist_bytes, S, (int)n_ls, (int)n_q, want);
    std::memset(hist, 0, want);
    for (uint64_t* out : {truncated, isolated, undefined}) std::memset(out, 0, (size_t)S * sizeof(uint64_t));
    if (p.n_a == 0) return PSA_OK;                           // every species empty: zeros
    const int64_t         row = order_row_words(n_ls, n_q);
    std::vector<uint64_t> acc;
    const ShellPass       order_pass = [&](const AngleWork& w, int64_t n_items, int64_t, int64_t nb) -> int {
        return launch_order_hist(c, w.count, w.list, c->d_rs_items.ptr, n_items, c->d_rs_part.as<unsigned>(), w.x, o, p.n_a, nb, n_q);
    };
    const ShellPass per_atom = [&](const AngleWork& w, int64_t, int64_t k0, int64_t nb) -> int {
        return copy_atom_rows(c, p.n_a, k0, nb, {{x, w.x, (size_t)n_ls * sizeof(int64_t)}, {n, w.count, sizeof(int32_t)}});
    };
    PSA_TRY(shell_run(c, p, sp, idx, box, box_inverse, origin_step, row, extra, order_pass, x != nullptr || n != nullptr ? per_atom : ShellPass(),
                      &acc));
    for (int a = 0; a < S; ++a) {
        const uint64_t* r = acc.data() + (size_t)a * (size_t)row;
        std::memcpy(hist + (size_t)a * bins, r, bins * sizeof(uint64_t));
        truncated[a] = r[bins], isolated[a] = r[bins + 1], undefined[a] = r[bins + 2];
    }
    return PSA_OK;
}

// an item's samples of the local order pass, 64 centres x the origins of a block, fit 32 bits in every counter
static_assert((uint64_t)ANGLE_ITEM_CENTRES * 65535 < (1ull << 32), "an item's samples fit 32 bits");

// N_lm = (-1)^m sqrt(1 / prod_{k = l-m+1 .. l+m} k), the product in float64 in ascending k, at [l * 13 + m]; behind it the
// caller's 3j blocks, (2 l + 1)^2 each, one per LOCAL_W3J_WORDS
int upload_local_tables(psa_ctx* c, const int32_t* ls, int32_t n_ls, const double* w3j) {
    std::vector<double> tab((size_t)LOCAL_NORM_WORDS + (size_t)n_ls * LOCAL_W3J_WORDS, 0.0);
    for (int l = 0; l <= ORDER_MAX_L; ++l)
        for (int m = 0; m <= l; ++m) {
            double prod = 1.0;
            for (int k = l - m + 1; k <= l + m; ++k) prod *= (double)k;
            tab[(size_t)(l * (ORDER_MAX_L + 1) + m)] = (m & 1 ? -1.0 : 1.0) * std::sqrt(1.0 / prod);
        }
    for (int j = 0; w3j != nullptr && j < n_ls; ++j) {
        const size_t side = 2 * (size_t)ls[j] + 1;
        std::memcpy(&tab[(size_t)LOCAL_NORM_WORDS + (size_t)j * LOCAL_W3J_WORDS], w3j, side * side * sizeof(double));
        w3j += side * side;
    }
    StageTimer st(c, PSA_T_H2D);
    return upload(c, c->d_local_tab, tab.data(), tab.size() * sizeof(double));
}

int local_order_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
                    const double* r_cut, int64_t origin_step, const int32_t* ls, int32_t n_ls, int32_t n_q, int32_t n_w, double w_range,
                    int32_t solid_l, double solid_threshold, const double* w3j, int64_t w3j_count, uint64_t* hist, size_t hist_bytes,
                    double* qbar2, double* w, double* wbar, int32_t* connections, int32_t* n) {
    PSA_REQUIRE(hist != nullptr, "null output");
    LocalLs o;
    PSA_TRY(ascending_orders(ls, n_ls, LOCAL_MAX_LS, 2, true, &o));   // at most four, even, in [2, 12]
    o.solid_l = solid_l;
    PSA_REQUIRE(o.mask >> (solid_l & 31) & 1u && solid_l >= 0 && solid_l < 32, "solid_l = %d is not among ls", (int)solid_l);
    PSA_REQUIRE(solid_threshold > 0.0 && solid_threshold <= 1.0, "the solid-like threshold is in (0, 1], got %g", solid_threshold);
    PSA_REQUIRE(std::isfinite(w_range) && w_range > 0.0, "w_range must be finite and positive, got %g", w_range);
    int64_t want_3j = 0;
    for (int j = 0; j < n_ls; ++j) want_3j += (2ll * ls[j] + 1) * (2ll * ls[j] + 1);
    PSA_REQUIRE(w3j != nullptr && w3j_count == want_3j, "w3j holds %lld values, the blocks (2 l + 1)^2 of the orders have %lld",
                (long long)w3j_count, (long long)want_3j);
    for (int64_t i = 0; i < want_3j; ++i) PSA_REQUIRE(std::isfinite(w3j[i]) && std::fabs(w3j[i]) <= 1.0, "w3j[%lld] = %g is no 3j symbol", (long long)i, w3j[i]);
    const bool    atoms = qbar2 != nullptr || w != nullptr || wbar != nullptr || connections != nullptr;
    const int64_t q_bytes = 16 * (int64_t)o.columns, extra = q_bytes + (atoms ? 24 * (int64_t)n_ls + 8 : 0);
    AtomGroups    p;
    AngleSpecies  sp;
    PSA_TRY(angle_check(c, "psa_local_order", box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, &p, &sp, extra));
    PSA_REQUIRE(n_q >= 1 && n_q <= LOCAL_MAX_BINS, "the number of q bins is in [1, %d], got %d", LOCAL_MAX_BINS, (int)n_q);
    PSA_REQUIRE(n_w >= 1 && n_w <= LOCAL_MAX_BINS, "the number of w bins is in [1, %d], got %d", LOCAL_MAX_BINS, (int)n_w);
    const int     S = p.G;
    const int64_t row = local_row_words(n_ls, n_q, n_w);
    const size_t  want = (size_t)S * (size_t)row * sizeof(uint64_t);
    PSA_REQUIRE(hist_bytes == want, "hist_bytes is %zu, the (%d,%lld) uint64 result has %zu", hist_bytes, S, (long long)row, want);
    std::memset(hist, 0, want);
    if (p.n_a == 0) return PSA_OK;                           // every species empty: zeros
    PSA_TRY(upload_local_tables(c, ls, n_ls, w3j));
    const double*   d_norm = c->d_local_tab.as<double>();
    const LocalBins bins{(int)n_q, (int)n_w, w_range, (double)n_w / (2.0 * w_range), solid_threshold * solid_threshold};
    // behind the table of a block of p.Ab origins: q-bar^2, w, w-bar (nb n_a, n_l) float64 each, one behind the other, of
    // the nb origins a pass runs over; behind the room of 3 p.Ab of them the connections
    const int64_t rows = p.Ab * p.n_a;
    struct Rows {
        double* values;
        int*    xi;
    };
    const auto rows_of = [&](const AngleWork& wk) {
        char* at = reinterpret_cast<char*>(wk.x) + (size_t)rows * (size_t)q_bytes;
        if (!atoms) return Rows{nullptr, nullptr};
        return Rows{reinterpret_cast<double*>(at), reinterpret_cast<int*>(at + 3 * (size_t)rows * (size_t)n_ls * sizeof(double))};
    };
    std::vector<uint64_t> acc;
    const ShellPass       passes = [&](const AngleWork& wk, int64_t n_items, int64_t, int64_t nb) -> int {
        const Rows r = rows_of(wk);
        PSA_TRY(launch_qlm_sum(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, d_norm, wk.x, o, p.n_a, nb));
        StageTimer second(c, PSA_T_PROJECT);                 // (inside the caller's PSA_T_PHASE, which spans both passes)
        return launch_local_order(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, wk.x, d_norm + LOCAL_NORM_WORDS, c->d_rs_part.as<unsigned>(),
                                  r.values, r.xi, o, bins, p.n_a, nb);
    };
    const ShellPass per_atom = [&](const AngleWork& wk, int64_t, int64_t k0, int64_t nb) -> int {
        const Rows   r = rows_of(wk);
        const size_t each = atoms ? (size_t)nb * (size_t)p.n_a * (size_t)n_ls : 0, cell = (size_t)n_ls * sizeof(double);
        return copy_atom_rows(c, p.n_a, k0, nb, {{qbar2, r.values, cell}, {w, r.values + each, cell}, {wbar, r.values + 2 * each, cell},
                                                 {connections, r.xi, sizeof(int32_t)}, {n, wk.count, sizeof(int32_t)}});
    };
    PSA_TRY(shell_run(c, p, sp, idx, box, box_inverse, origin_step, row, extra, passes, atoms || n != nullptr ? per_atom : ShellPass(), &acc));
    std::memcpy(hist, acc.data(), want);
    return PSA_OK;
}

// ---- psa_solid_clusters, psa_debug_cluster_labels (kernels: cluster.hip).  Behind the table of a block of `cap` rows: the
// masks (8 bytes a row), then xi, parent and size (4 each): 20 bytes per atom and origin
constexpr int64_t CLUSTER_ATOM_BYTES = 8 + 4 + 4 + 4;
ClusterWork cluster_work(void* behind, int64_t cap) {
    char* at = static_cast<char*>(behind);
    return ClusterWork{reinterpret_cast<unsigned long long*>(at), reinterpret_cast<int*>(at + 8 * (size_t)cap),
                       reinterpret_cast<int*>(at + 12 * (size_t)cap), reinterpret_cast<int*>(at + 16 * (size_t)cap)};
}

// the accumulator's tail of a call over n_o origins: the stats words, the error word, then (n_o, 4) int32
int64_t cluster_tail_words(int n_sizes, int64_t n_o) { return cluster_stat_words(n_sizes) + 1 + 2 * n_o; }

// The caller's outputs of the two cluster entries, and what both do with a block after its hook pass: the flatten pass, the
// stats pass into the partials, their reduce into the tail at `d_tail`, the per-atom rows to the caller's arrays
struct ClusterOut {
    uint64_t *size_counts, *large_atoms;
    int32_t * n_solid, *n_clusters, *largest, *largest_label, *labels, *size_atoms, *connections, *n;
    uint64_t* bond_masks;
};
int cluster_out_check(const ClusterOut& o, int32_t link, int32_t n_sizes) {
    PSA_REQUIRE(o.size_counts != nullptr && o.large_atoms != nullptr && o.n_solid != nullptr && o.n_clusters != nullptr &&
                    o.largest != nullptr && o.largest_label != nullptr, "null output");
    PSA_REQUIRE(link == 0 || link == 1, "link is 0 (neighbours) or 1 (solid bonds), got %d", (int)link);
    PSA_REQUIRE(n_sizes >= 1 && n_sizes <= CLUSTER_MAX_SIZES, "n_sizes is in [1, %d], got %d", CLUSTER_MAX_SIZES, (int)n_sizes);
    return PSA_OK;
}
// nothing listed: zeros, no cluster
void cluster_out_empty(const ClusterOut& o, int32_t n_sizes, int64_t n_o) {
    std::memset(o.size_counts, 0, ((size_t)n_sizes + 2) * sizeof(uint64_t));
    *o.large_atoms = 0;
    for (int64_t k = 0; k < n_o; ++k) o.n_solid[k] = o.n_clusters[k] = o.largest[k] = 0, o.largest_label[k] = -1;
}
int cluster_block(psa_ctx* c, const ClusterWork& w, const int* d_count, unsigned long long* d_tail, int32_t n_sizes, int64_t n_a, int64_t k0,
                  int64_t nb, const ClusterOut& o) {
    const int64_t words = cluster_stat_words(n_sizes), groups = cluster_stat_groups(nb);
    {
        StageTimer st(c, PSA_T_EPILOGUE);
        PSA_TRY(c->d_rs_part.reserve((size_t)groups * (size_t)words * sizeof(uint32_t)));
        PSA_TRY(launch_cluster_stats(c, w, reinterpret_cast<int*>(d_tail + words + 1) + 4 * k0, c->d_rs_part.as<unsigned>(), n_sizes, n_a, nb));
        HistRows rows{};
        rows.lo[0] = 0, rows.hi[0] = (int)groups, rows.factor[0] = 1;
        PSA_TRY(launch_hist_reduce(c, c->d_rs_part.as<unsigned>(), rows, 1, 1, words, d_tail));
    }
    return copy_atom_rows(c, n_a, k0, nb, {{o.labels, w.parent, sizeof(int32_t)}, {o.size_atoms, w.size, sizeof(int32_t)},
                                           {o.connections, w.xi, sizeof(int32_t)}, {o.n, d_count, sizeof(int32_t)},
                                           {o.bond_masks, w.mask, sizeof(uint64_t)}});
}
// the tail on the host to the caller's arrays; the error word
int cluster_out_tail(const uint64_t* tail, int32_t n_sizes, int64_t n_o, const ClusterOut& o) {
    const int64_t words = cluster_stat_words(n_sizes);
    if (tail[words] != 0) {
        set_error("cluster pass did not converge: a bounded loop of the hook or the flatten pass ran out");
        return PSA_EHIP;
    }
    std::memcpy(o.size_counts, tail, ((size_t)n_sizes + 2) * sizeof(uint64_t));
    *o.large_atoms = tail[n_sizes + 2];
    const int32_t* per = reinterpret_cast<const int32_t*>(tail + words + 1);
    for (int64_t k = 0; k < n_o; ++k)
        o.n_solid[k] = per[4 * k], o.n_clusters[k] = per[4 * k + 1], o.largest[k] = per[4 * k + 2], o.largest_label[k] = per[4 * k + 3];
    return PSA_OK;
}

// an item's samples of the bonds pass, 64 centres x the origins of a block, fit 32 bits in every counter (the stats pass:
// cluster.hip states its own product)
static_assert((uint64_t)ANGLE_ITEM_CENTRES * 65535 < (1ull << 32), "an item's samples fit 32 bits");

int cluster_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
                const double* r_cut, int64_t origin_step, int32_t solid_l, double solid_threshold, int32_t min_connections, int32_t link,
                int32_t n_sizes, uint64_t* species_rows, const ClusterOut& out) {
    PSA_REQUIRE(species_rows != nullptr, "null output");
    PSA_TRY(cluster_out_check(out, link, n_sizes));
    PSA_REQUIRE(solid_l >= 2 && solid_l <= ORDER_MAX_L && solid_l % 2 == 0, "solid_l = %d is not an even order in [2, %d]", (int)solid_l, ORDER_MAX_L);
    PSA_REQUIRE(solid_threshold > 0.0 && solid_threshold <= 1.0, "the solid-like threshold is in (0, 1], got %g", solid_threshold);
    PSA_REQUIRE(min_connections >= 0 && min_connections <= ANGLE_MAX_NEIGHBOURS, "min_connections is in [0, %d], got %d", ANGLE_MAX_NEIGHBOURS,
                (int)min_connections);
    const LocalLs o{1, (int)solid_l, (int)solid_l + 1, (int)solid_l, 1u << solid_l};
    const int64_t q_bytes = 16 * (int64_t)o.columns, extra = q_bytes + CLUSTER_ATOM_BYTES;
    AtomGroups    p;
    AngleSpecies  sp;
    PSA_TRY(angle_check(c, "psa_solid_clusters", box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, &p, &sp, extra));
    const int     S = p.G;
    const int64_t n_o = (p.T - 1) / origin_step + 1, row = CLUSTER_ROW_WORDS;
    const size_t  want = (size_t)S * (size_t)row * sizeof(uint64_t);
    std::memset(species_rows, 0, want);
    if (p.n_a == 0) {                                        // every species empty: zeros, no cluster
        cluster_out_empty(out, n_sizes, n_o);
        return PSA_OK;
    }
    PSA_TRY(upload_local_tables(c, &solid_l, 1, nullptr));
    const double* d_norm = c->d_local_tab.as<double>();
    const double  thr2 = solid_threshold * solid_threshold;
    const int64_t cap = p.Ab * p.n_a, words = cluster_stat_words(n_sizes);
    const auto    tail_of = [&]() { return c->d_rs_acc.as<unsigned long long>() + (size_t)S * (size_t)row; };
    const auto    work_of = [&](const AngleWork& wk) { return cluster_work(reinterpret_cast<char*>(wk.x) + (size_t)cap * (size_t)q_bytes, cap); };
    std::vector<uint64_t> acc;
    const ShellPass       passes = [&](const AngleWork& wk, int64_t n_items, int64_t, int64_t nb) -> int {
        const ClusterWork w = work_of(wk);
        int*              d_err = reinterpret_cast<int*>(tail_of() + words);
        PSA_TRY(launch_qlm_sum(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, d_norm, wk.x, o, p.n_a, nb));
        PSA_TRY(launch_cluster_bonds(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, wk.x, c->d_rs_part.as<unsigned>(), w, o, thr2,
                                     min_connections, p.n_a, nb));
        {
            StageTimer hook(c, PSA_T_PROJECT);               // (inside the caller's PSA_T_PHASE, which spans the four passes)
            PSA_TRY(launch_cluster_hook(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, w, link, false, d_err, p.n_a, nb));
        }
        StageTimer flatten(c, PSA_T_FFT);
        return launch_cluster_flatten(c, w, d_err, p.n_a, nb);
    };
    const ShellPass block = [&](const AngleWork& wk, int64_t, int64_t k0, int64_t nb) -> int {
        return cluster_block(c, work_of(wk), wk.count, tail_of(), n_sizes, p.n_a, k0, nb, out);
    };
    PSA_TRY(shell_run(c, p, sp, idx, box, box_inverse, origin_step, row, extra, passes, block, &acc, cluster_tail_words(n_sizes, n_o)));
    std::memcpy(species_rows, acc.data(), want);
    return cluster_out_tail(acc.data() + (size_t)S * (size_t)row, n_sizes, n_o, out);
}

// ---- psa_bond_persistence (kernels: persist.hip).  Behind the counts of a block of `cap` rows: the tags (256 bytes a row),
// the survivor and the alive masks (8 each), the lagged fractions (12) and 4 bytes of padding: 288 bytes per atom and origin
constexpr int64_t PERSIST_ATOM_BYTES = 4 * ANGLE_MAX_NEIGHBOURS + 8 + 8 + 12 + 4;
static_assert(PERSIST_ATOM_BYTES % 8 == 0, "the work behind the counts is a multiple of 8 bytes per row");
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

int persist_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
                const double* r_cut, const double* r_break, int64_t origin_step, const int64_t* lags, int32_t n_lags, int64_t sample_step,
                int32_t continuous, const PersistOut& out) {
    PSA_REQUIRE(out.bonds != nullptr && out.alive != nullptr && out.unbroken != nullptr && out.lost != nullptr && out.truncated != nullptr,
                "null output");
    PSA_REQUIRE(lags != nullptr && r_break != nullptr, "null lags or r_break");
    PSA_REQUIRE(n_lags >= 1 && n_lags <= PERSIST_MAX_LAGS, "the number of lags is in [1, %d], got %d", PERSIST_MAX_LAGS, (int)n_lags);
    PSA_REQUIRE(sample_step >= 1, "sample_step must be at least 1, got %lld", (long long)sample_step);
    PSA_REQUIRE(continuous == 0 || continuous == 1, "continuous is 0 or 1, got %d", (int)continuous);
    AtomGroups   p;
    AngleSpecies sp;
    PSA_TRY(angle_check(c, "psa_bond_persistence", box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, &p, &sp, PERSIST_ATOM_BYTES));
    const int S = p.G, NC = ANGLE_MAX_NEIGHBOURS + 1;
    for (int j = 0; j < n_lags; ++j) {
        PSA_REQUIRE(lags[j] >= 0 && lags[j] <= p.T - 1, "lag %lld is outside [0, T - 1 = %lld]", (long long)lags[j], (long long)(p.T - 1));
        PSA_REQUIRE(j == 0 || lags[j] > lags[j - 1], "lags must be strictly ascending: lags[%d] = %lld after %lld", j, (long long)lags[j],
                    (long long)lags[j ? j - 1 : 0]);
        PSA_REQUIRE(lags[j] % sample_step == 0, "lag %lld is no multiple of sample_step = %lld", (long long)lags[j], (long long)sample_step);
    }
    AngleSpecies rb = sp;                                    // the species with float32(1 / r_break) in place of 1 / r_cut
    for (int a = 0; a < S; ++a)
        for (int b = 0; b < S; ++b) {
            const double r = r_break[a * S + b], rc = r_cut[a * S + b];
            PSA_REQUIRE(std::isfinite(r) && r >= rc, "r_break[%d][%d] = %g must be finite and at least r_cut[%d][%d] = %g", a, b, r, a, b, rc);
            PSA_REQUIRE(r == r_break[b * S + a], "r_break is not symmetric: [%d][%d] = %.17g, [%d][%d] = %.17g", a, b, r, b, a, r_break[b * S + a]);
            PSA_REQUIRE((r == 0.0) == (rc == 0.0), "r_break[%d][%d] = %g and r_cut[%d][%d] = %g: one is 0 (no bond) and the other is not", a, b,
                        r, a, b, rc);
            char what[32];
            std::snprintf(what, sizeof what, "r_break[%d][%d]", a, b);
            PSA_TRY(served_radius_check(box_inverse, what, r));
            const float inv = r > 0.0 ? (float)(1.0 / r) : 0.f;
            PSA_REQUIRE(r == 0.0 || (std::isfinite(inv) && inv > 0.f), "r_break[%d][%d] = %g has no float32 reciprocal", a, b, r);
            rb.inv_rc[a * S + b] = inv;
        }
    const int64_t n_o0 = (p.T - 1) / origin_step + 1;
    const size_t  pairs = (size_t)n_lags * (size_t)S * (size_t)S, want_p = pairs * sizeof(uint64_t);
    const size_t  want_l = (size_t)n_lags * (size_t)S * (size_t)NC * sizeof(uint64_t), want_t = (size_t)n_lags * (size_t)S * sizeof(uint64_t);
    const size_t  want_m = (size_t)n_lags * (size_t)n_o0 * (size_t)p.n_a * sizeof(uint64_t);
    PSA_REQUIRE(out.pair_bytes == want_p, "pair_bytes is %zu, each (%d,%d,%d) uint64 result has %zu", out.pair_bytes, (int)n_lags, S, S, want_p);
    PSA_REQUIRE(out.lost_bytes == want_l, "lost_bytes is %zu, the (%d,%d,%d) uint64 result has %zu", out.lost_bytes, (int)n_lags, S, NC, want_l);
    PSA_REQUIRE(out.truncated_bytes == want_t, "truncated_bytes is %zu, the (%d,%d) uint64 result has %zu", out.truncated_bytes, (int)n_lags, S,
                want_t);
    const bool masks = out.alive_masks != nullptr || out.unbroken_masks != nullptr;
    PSA_REQUIRE(!masks || out.masks_bytes == want_m, "masks_bytes is %zu, each (%d,%lld,%lld) uint64 per-atom result has %zu", out.masks_bytes,
                (int)n_lags, (long long)n_o0, (long long)p.n_a, want_m);
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
    const int64_t row = persist_row_words(S), cols = (int64_t)n_lags * row, cap = p.Ab * p.n_a, s = origin_step;
    const float*  d_pos = c->slot[PSA_SLOT_POSITIONS].buf.as<float>();
    std::vector<uint64_t> acc;
    const ShellPass       passes = [&](const AngleWork& wk, int64_t n_items, int64_t k0, int64_t nb) -> int {
        char*               at = reinterpret_cast<char*>(wk.x);
        int*                d_tags = reinterpret_cast<int*>(at);
        unsigned long long* d_surv = reinterpret_cast<unsigned long long*>(at + 4 * ANGLE_MAX_NEIGHBOURS * (size_t)cap);
        unsigned long long* d_alive = d_surv + cap;
        float*              d_cl = reinterpret_cast<float*>(d_alive + cap);
        unsigned*           d_part = c->d_rs_part.as<unsigned>();
        // a lag none of whose origins lies in this block is not visited: its counters are zeros
        PSA_HIP_CHECK(hipMemsetAsync(d_part, 0, (size_t)n_items * (size_t)cols * sizeof(uint32_t), c->stream));
        PSA_TRY(launch_persist_tags(c, wk.count, wk.list, d_tags, d_surv, p.n_a, nb));
        for (const Visit& v : visits) {
            // the origins of the block with o + f <= T - 1: a prefix, shorter with every later frame
            const int64_t n_f = std::min(nb, (p.T - 1 - v.f) / s + 1 - k0);
            if (n_f <= 0) break;
            PSA_TRY(launch_pair_frac(c, d_pos, p.d_idx, p.n_a, box_inverse, d_cl, k0 * s + v.f, s, n_f, p.T, p.N));
            PSA_TRY(launch_persist_step(c, wk.count, d_tags, c->d_rs_items.ptr, n_items, d_cl, d_surv, d_alive,
                                        v.j >= 0 ? d_part + (size_t)v.j * (size_t)row : nullptr, cols, rb, box, p.n_a, n_f, continuous != 0));
            if (v.j < 0 || !masks) continue;
            const size_t lag_at = (size_t)v.j * (size_t)n_o0 * (size_t)p.n_a;
            PSA_TRY(copy_atom_rows(c, p.n_a, k0, n_f, {{out.alive_masks ? out.alive_masks + lag_at : nullptr, d_alive, sizeof(uint64_t)},
                                                       {out.unbroken_masks && continuous ? out.unbroken_masks + lag_at : nullptr, d_surv,
                                                        sizeof(uint64_t)}}));
        }
        return PSA_OK;
    };
    PSA_TRY(shell_run(c, p, sp, idx, box, box_inverse, origin_step, cols, PERSIST_ATOM_BYTES, passes, nullptr, &acc));
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

// ---- psa_common_neighbours (kernels: cna.hip).  Behind the counts of a block of `cap` rows: the types (4 bytes a row and 4 of
// padding) and, with the per-bond output, the signatures (256): 8 or 264 bytes per atom and origin
constexpr int64_t CNA_ATOM_BYTES = 8, CNA_BOND_BYTES = 4 * ANGLE_MAX_NEIGHBOURS;
// an item's samples of the signature pass, 64 centres x the origins of its slab x 64 bonds, fit 32 bits in every counter; the
// census pass counts at most 2^28 - 1 atoms of one origin
static_assert((uint64_t)ANGLE_ITEM_CENTRES * ANGLE_MAX_SLAB * ANGLE_MAX_NEIGHBOURS < (1ull << 32), "an item's samples fit 32 bits");

struct CnaOut {
    uint64_t* signature_counts;
    size_t    signature_bytes;
    uint64_t *signature_outside, *type_counts;
    size_t    type_bytes;
    uint64_t* truncated;
    int32_t * types, *n;
    size_t    atom_bytes;
    uint32_t* bond_signatures;
    size_t    bond_bytes;
};

int cna_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
            const double* r_cut, int64_t origin_step, const CnaOut& out) {
    PSA_REQUIRE(out.signature_counts != nullptr && out.signature_outside != nullptr && out.type_counts != nullptr && out.truncated != nullptr,
                "null output");
    const int64_t extra = CNA_ATOM_BYTES + (out.bond_signatures != nullptr ? CNA_BOND_BYTES : 0);
    AtomGroups    p;
    AngleSpecies  sp;
    PSA_TRY(angle_check(c, "psa_common_neighbours", box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, &p, &sp, extra));
    const int     S = p.G;
    const int64_t n_o = (p.T - 1) / origin_step + 1, row = CNA_ROW_WORDS, table = row - 2;
    const size_t  want_s = (size_t)S * (size_t)table * sizeof(uint64_t), want_t = (size_t)n_o * (size_t)S * CNA_TYPES * sizeof(uint64_t);
    const size_t  want_a = (size_t)n_o * (size_t)p.n_a * sizeof(int32_t), want_b = want_a * ANGLE_MAX_NEIGHBOURS;
    PSA_REQUIRE(out.signature_bytes == want_s, "signature_bytes is %zu, the (%d,%d,%d,%d) uint64 result has %zu", out.signature_bytes, S,
                CNA_MAX_J, CNA_MAX_K, CNA_MAX_L, want_s);
    PSA_REQUIRE(out.type_bytes == want_t, "type_bytes is %zu, the (%lld,%d,%d) uint64 result has %zu", out.type_bytes, (long long)n_o, S,
                CNA_TYPES, want_t);
    PSA_REQUIRE((out.types == nullptr && out.n == nullptr) || out.atom_bytes == want_a, "atom_bytes is %zu, each (%lld,%lld) int32 per-atom "
                "result has %zu", out.atom_bytes, (long long)n_o, (long long)p.n_a, want_a);
    PSA_REQUIRE(out.bond_signatures == nullptr || out.bond_bytes == want_b, "bond_bytes is %zu, the (%lld,%lld,%d) uint32 per-bond result has "
                "%zu", out.bond_bytes, (long long)n_o, (long long)p.n_a, ANGLE_MAX_NEIGHBOURS, want_b);
    std::memset(out.signature_counts, 0, want_s);
    std::memset(out.type_counts, 0, want_t);
    for (uint64_t* o : {out.signature_outside, out.truncated}) std::memset(o, 0, (size_t)S * sizeof(uint64_t));
    if (p.n_a == 0) return PSA_OK;                           // every species empty: zeros, nothing per atom
    const int64_t cap = p.Ab * p.n_a, tail = n_o * S * CNA_TYPES;
    // behind the counts of a block: the types, then the signatures
    const auto types_of = [&](const AngleWork& wk) { return reinterpret_cast<int*>(wk.x); };
    const auto sigs_of = [&](const AngleWork& wk) {
        return out.bond_signatures != nullptr ? reinterpret_cast<unsigned*>(reinterpret_cast<char*>(wk.x) + (size_t)cap * CNA_ATOM_BYTES) : nullptr;
    };
    std::vector<uint64_t> acc;
    const ShellPass       passes = [&](const AngleWork& wk, int64_t n_items, int64_t k0, int64_t nb) -> int {
        PSA_TRY(launch_cna_signature(c, wk.c, wk.count, wk.list, c->d_rs_items.ptr, n_items, types_of(wk), sigs_of(wk),
                                     c->d_rs_part.as<unsigned>(), sp, box, p.n_a, nb));
        StageTimer census(c, PSA_T_PROJECT);                 // (inside the caller's PSA_T_PHASE, which spans both passes)
        return launch_cna_census(c, types_of(wk), c->d_rs_acc.as<unsigned long long>() + (size_t)S * (size_t)row + (size_t)k0 * S * CNA_TYPES,
                                 sp, p.n_a, nb);
    };
    const ShellPass per_atom = [&](const AngleWork& wk, int64_t, int64_t k0, int64_t nb) -> int {
        return copy_atom_rows(c, p.n_a, k0, nb, {{out.types, types_of(wk), sizeof(int32_t)}, {out.n, wk.count, sizeof(int32_t)},
                                                 {out.bond_signatures, sigs_of(wk), ANGLE_MAX_NEIGHBOURS * sizeof(uint32_t)}});
    };
    const bool atoms = out.types != nullptr || out.n != nullptr || out.bond_signatures != nullptr;
    PSA_TRY(shell_run(c, p, sp, idx, box, box_inverse, origin_step, row, extra, passes, atoms ? per_atom : ShellPass(), &acc, tail));
    for (int a = 0; a < S; ++a) {
        const uint64_t* r = acc.data() + (size_t)a * (size_t)row;
        std::memcpy(out.signature_counts + (size_t)a * (size_t)table, r, (size_t)table * sizeof(uint64_t));
        out.signature_outside[a] = r[table], out.truncated[a] = r[table + 1];
    }
    std::memcpy(out.type_counts, acc.data() + (size_t)S * (size_t)row, want_t);
    return PSA_OK;
}

// leaves its scope only once the stream has run dry
struct HostSync {
    psa_ctx* c;
    ~HostSync() { (void)hipStreamSynchronize(c->stream); }
};

// the graph passes alone on the caller's graph: one species of n_a columns, all n_o origins in one block
int debug_cluster_run(psa_ctx* c, int64_t n_o, int64_t n_a, const int32_t* count, const int32_t* list, const uint8_t* solid,
                      const uint64_t* bond_masks, int32_t link, int32_t n_sizes, const ClusterOut& out) {
    PSA_TRY(cluster_out_check(out, link, n_sizes));
    PSA_REQUIRE(n_o >= 0 && n_o <= 65535 && n_a >= 0 && n_a < (1ll << ANGLE_SPECIES_SHIFT), "n_o is in [0, 65535] and n_a in [0, 2^%d - 1], got %lld, %lld",
                ANGLE_SPECIES_SHIFT, (long long)n_o, (long long)n_a);
    cluster_out_empty(out, n_sizes, n_o);
    if (n_o == 0 || n_a == 0) return PSA_OK;
    PSA_REQUIRE(count != nullptr && list != nullptr && solid != nullptr, "null input");
    const int64_t cap = n_o * n_a;
    const size_t  bytes = (size_t)cap * (size_t)(ANGLE_ORIGIN_BYTES + CLUSTER_ATOM_BYTES);
    PSA_REQUIRE((int64_t)bytes <= c->opt_dynamic_work_bytes, "the work budget of %lld bytes (PSA_OPT_DYNAMIC_WORK_BYTES) cannot hold the graph: %lld "
                "origins of %lld atoms need %zu bytes", (long long)c->opt_dynamic_work_bytes, (long long)n_o, (long long)n_a, bytes);
    // the list entries as the neighbour pass writes them, as far as the graph passes read them: no leg, the tag = the column
    // (species 0)
    std::vector<float>    entries((size_t)cap * ANGLE_MAX_NEIGHBOURS * 4, 0.f);
    std::vector<uint64_t> masks((size_t)cap);
    std::vector<int32_t>  parent((size_t)cap), zeros((size_t)cap, 0);
    for (int64_t k = 0; k < n_o; ++k)
        for (int64_t a = 0; a < n_a; ++a) {
            const size_t r = (size_t)(k * n_a + a);
            PSA_REQUIRE(count[r] >= 0 && count[r] <= ANGLE_MAX_NEIGHBOURS, "count[%lld][%lld] = %d is outside [0, %d]", (long long)k, (long long)a,
                        (int)count[r], ANGLE_MAX_NEIGHBOURS);
            for (int s = 0; s < count[r]; ++s) {
                const int32_t b = list[r * ANGLE_MAX_NEIGHBOURS + (size_t)s];
                PSA_REQUIRE(b >= 0 && b < n_a, "list[%lld][%lld][%d] = %d is outside [0, n_a = %lld)", (long long)k, (long long)a, s, (int)b, (long long)n_a);
                PSA_REQUIRE(b != a, "list[%lld][%lld][%d] = %d is a self-loop", (long long)k, (long long)a, s, (int)b);
                std::memcpy(&entries[(r * ANGLE_MAX_NEIGHBOURS + (size_t)s) * 4 + 3], &b, sizeof b);
            }
            masks[r] = bond_masks != nullptr ? bond_masks[r] : ~0ull;
            parent[r] = solid[r] ? (int32_t)a : -1;
        }
    AtomGroups p;
    p.n_a = n_a, p.G = 1, p.start = {0, n_a}, p.size = {n_a};
    int32_t                      first[PAIR_MAX_SPECIES + 1];
    const std::vector<AngleItem> items = angle_items(p, n_o, CLUSTER_ROW_WORDS, first);
    AngleWork                    wk;
    PSA_TRY(angle_work(c, n_a, n_o, &wk, CLUSTER_ATOM_BYTES));
    const ClusterWork w = cluster_work(wk.x, cap);
    const int64_t     tail = cluster_tail_words(n_sizes, n_o);
    PSA_TRY(c->d_rs_acc.reserve((size_t)tail * sizeof(uint64_t)));
    std::vector<uint64_t> host((size_t)tail);
    HostSync              wait{c};                           // the copies below read this function's vectors
    PSA_HIP_CHECK(hipMemsetAsync(c->d_rs_acc.ptr, 0, (size_t)tail * sizeof(uint64_t), c->stream));
    PSA_TRY(upload(c, c->d_rs_items, items.data(), items.size() * sizeof(AngleItem)));
    PSA_HIP_CHECK(hipMemcpyAsync(wk.list, entries.data(), entries.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    PSA_HIP_CHECK(hipMemcpyAsync(wk.count, count, (size_t)cap * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    PSA_HIP_CHECK(hipMemcpyAsync(w.mask, masks.data(), (size_t)cap * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    PSA_HIP_CHECK(hipMemcpyAsync(w.parent, parent.data(), (size_t)cap * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    PSA_HIP_CHECK(hipMemcpyAsync(w.size, zeros.data(), (size_t)cap * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    PSA_HIP_CHECK(hipMemcpyAsync(w.xi, zeros.data(), (size_t)cap * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    unsigned long long* d_tail = c->d_rs_acc.as<unsigned long long>();
    int*                d_err = reinterpret_cast<int*>(d_tail + cluster_stat_words(n_sizes));
    PSA_TRY(launch_cluster_hook(c, wk.count, wk.list, c->d_rs_items.ptr, (int64_t)items.size(), w, link, true, d_err, n_a, n_o));
    PSA_TRY(launch_cluster_flatten(c, w, d_err, n_a, n_o));
    ClusterOut per = out;
    per.connections = nullptr, per.n = nullptr, per.bond_masks = nullptr;
    PSA_TRY(cluster_block(c, w, wk.count, d_tail, n_sizes, n_a, 0, n_o, per));
    PSA_HIP_CHECK(hipMemcpyAsync(host.data(), d_tail, host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return cluster_out_tail(host.data(), n_sizes, n_o, out);
}

// What the two entries of one frame start with after angle_check: the frame refused outside [0, T - 1]; then, unless no atom
// is listed (w->list stays null), the atom list uploaded, the work buffer of one origin (extra as for shell_run) and the
// fraction pass and the neighbour pass of that frame into it
int shell_one_frame(psa_ctx* c, AtomGroups& p, const AngleSpecies& sp, const int32_t* idx, const double* box, const double* box_inverse,
                    int64_t frame, int64_t extra, AngleWork* w) {
    PSA_REQUIRE(frame >= 0 && frame <= p.T - 1, "frame %lld is outside [0, T - 1 = %lld]", (long long)frame, (long long)(p.T - 1));
    *w = AngleWork{};
    if (p.n_a == 0) return PSA_OK;
    PSA_TRY(upload_atom_list(c, &p, idx));
    PSA_TRY(angle_work(c, p.n_a, 1, w, extra));
    PSA_TRY(launch_pair_frac(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(), p.d_idx, p.n_a, box_inverse, w->c, frame, 0, 1, p.T, p.N));
    return launch_angle_neighbours(c, w->c, w->count, w->list, sp, box, p.n_a, 1);
}

// the fraction pass, the neighbour pass and the q_lm pass of one frame: Q (n_a, columns, 2) int64
int debug_qlm_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
                  const double* r_cut, int64_t frame, const int32_t* ls, int32_t n_ls, int64_t* q) {
    PSA_REQUIRE(q != nullptr, "null output");
    LocalLs o;
    PSA_TRY(ascending_orders(ls, n_ls, LOCAL_MAX_LS, 2, true, &o));   // at most four, even, in [2, 12]
    o.solid_l = ls[0];
    const int64_t q_bytes = 16 * (int64_t)o.columns;
    AtomGroups    p;
    AngleSpecies  sp;
    AngleWork     w;
    PSA_TRY(angle_check(c, "psa_debug_qlm", box, box_inverse, idx, group_start, n_groups, r_cut, 1, &p, &sp, q_bytes));
    PSA_TRY(shell_one_frame(c, p, sp, idx, box, box_inverse, frame, q_bytes, &w));
    if (p.n_a == 0) return PSA_OK;
    int32_t                      first[PAIR_MAX_SPECIES + 1];
    const std::vector<AngleItem> items = angle_items(p, 1, 1, first);
    PSA_TRY(upload(c, c->d_rs_items, items.data(), items.size() * sizeof(AngleItem)));
    PSA_TRY(upload_local_tables(c, ls, n_ls, nullptr));
    PSA_TRY(launch_qlm_sum(c, w.count, w.list, c->d_rs_items.ptr, (int64_t)items.size(), c->d_local_tab.as<double>(), w.x, o, p.n_a, 1));
    PSA_HIP_CHECK(hipMemcpyAsync(q, w.x, (size_t)p.n_a * (size_t)q_bytes, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the fraction pass and the neighbour pass of one frame: the true counts and the first 64 list positions of every centre
int debug_lists_run(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                    int32_t n_groups, const double* r_cut, int64_t frame, int32_t* count, int32_t* list) {
    PSA_REQUIRE(count != nullptr && list != nullptr, "null output");
    AtomGroups   p;
    AngleSpecies sp;
    AngleWork    w;
    PSA_TRY(angle_check(c, "psa_debug_neighbour_lists", box, box_inverse, idx, group_start, n_groups, r_cut, 1, &p, &sp));
    PSA_TRY(shell_one_frame(c, p, sp, idx, box, box_inverse, frame, 0, &w));
    if (p.n_a == 0) return PSA_OK;
    std::vector<float> h((size_t)p.n_a * ANGLE_MAX_NEIGHBOURS * 4);
    PSA_HIP_CHECK(hipMemcpyAsync(count, w.count, (size_t)p.n_a * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipMemcpyAsync(h.data(), w.list, h.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int64_t a = 0; a < p.n_a; ++a)
        for (int s = 0; s < ANGLE_MAX_NEIGHBOURS; ++s) {
            int32_t tag;
            std::memcpy(&tag, &h[((size_t)a * ANGLE_MAX_NEIGHBOURS + (size_t)s) * 4 + 3], sizeof tag);
            list[(size_t)a * ANGLE_MAX_NEIGHBOURS + (size_t)s] = s < count[a] ? (tag & ((1 << ANGLE_SPECIES_SHIFT) - 1)) : -1;
        }
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_angle_histogram(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                        int32_t n_groups, const double* r_cut, int64_t origin_step, int32_t n_theta, uint64_t* angles, size_t angles_bytes,
                        uint64_t* coord, size_t coord_bytes, uint64_t* truncated) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, angle_run(c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, n_theta, angles, angles_bytes, coord,
                                     coord_bytes, truncated), "psa_angle_histogram");
}

int psa_bond_order(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                   int32_t n_groups, const double* r_cut, int64_t origin_step, const int32_t* ls, int32_t n_ls, int32_t n_q, uint64_t* hist,
                   size_t hist_bytes, uint64_t* truncated, uint64_t* isolated, uint64_t* undefined, int64_t* x, int32_t* n) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, order_run(c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, ls, n_ls, n_q, hist, hist_bytes,
                                     truncated, isolated, undefined, x, n), "psa_bond_order");
}

int psa_local_order(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                    int32_t n_groups, const double* r_cut, int64_t origin_step, const int32_t* ls, int32_t n_ls, int32_t n_q, int32_t n_w,
                    double w_range, int32_t solid_l, double solid_threshold, const double* w3j, int64_t w3j_count, uint64_t* hist,
                    size_t hist_bytes, double* qbar2, double* w, double* wbar, int32_t* connections, int32_t* n) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, local_order_run(c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, ls, n_ls, n_q, n_w, w_range,
                                           solid_l, solid_threshold, w3j, w3j_count, hist, hist_bytes, qbar2, w, wbar, connections, n),
                        "psa_local_order");
}

int psa_solid_clusters(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                       int32_t n_groups, const double* r_cut, int64_t origin_step, int32_t solid_l, double solid_threshold,
                       int32_t min_connections, int32_t link, int32_t n_sizes, uint64_t* species_rows, uint64_t* size_counts,
                       uint64_t* large_atoms, int32_t* n_solid, int32_t* n_clusters, int32_t* largest, int32_t* largest_label, int32_t* labels,
                       int32_t* size_atoms, int32_t* connections, int32_t* n, uint64_t* bond_masks) {
    PSA_TRY(enter(c));
    Guard guard(c);
    const ClusterOut out{size_counts, large_atoms, n_solid, n_clusters, largest, largest_label, labels, size_atoms, connections, n, bond_masks};
    return synchronised(c, cluster_run(c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, solid_l, solid_threshold,
                                       min_connections, link, n_sizes, species_rows, out), "psa_solid_clusters");
}

int psa_bond_persistence(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                         int32_t n_groups, const double* r_cut, const double* r_break, int64_t origin_step, const int64_t* lags,
                         int32_t n_lags, int64_t sample_step, int32_t continuous, uint64_t* bonds, uint64_t* alive, uint64_t* unbroken,
                         size_t pair_bytes, uint64_t* lost, size_t lost_bytes, uint64_t* truncated, size_t truncated_bytes,
                         uint64_t* alive_masks, uint64_t* unbroken_masks, size_t masks_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    const PersistOut out{bonds, alive, unbroken, pair_bytes, lost, lost_bytes, truncated, truncated_bytes, alive_masks, unbroken_masks, masks_bytes};
    return synchronised(c, persist_run(c, box, box_inverse, idx, group_start, n_groups, r_cut, r_break, origin_step, lags, n_lags, sample_step,
                                       continuous, out), "psa_bond_persistence");
}

int psa_common_neighbours(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                          int32_t n_groups, const double* r_cut, int64_t origin_step, uint64_t* signature_counts, size_t signature_bytes,
                          uint64_t* signature_outside, uint64_t* type_counts, size_t type_bytes, uint64_t* truncated, int32_t* types,
                          int32_t* n, size_t atom_bytes, uint32_t* bond_signatures, size_t bond_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    const CnaOut out{signature_counts, signature_bytes, signature_outside, type_counts, type_bytes, truncated, types, n, atom_bytes,
                     bond_signatures, bond_bytes};
    return synchronised(c, cna_run(c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step, out), "psa_common_neighbours");
}

int psa_debug_cluster_labels(psa_ctx* c, int64_t n_o, int64_t n_a, const int32_t* count, const int32_t* list, const uint8_t* solid,
                             const uint64_t* bond_masks, int32_t link, int32_t n_sizes, uint64_t* size_counts, uint64_t* large_atoms,
                             int32_t* n_solid, int32_t* n_clusters, int32_t* largest, int32_t* largest_label, int32_t* labels,
                             int32_t* size_atoms) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_REQUIRE(c->comm == nullptr && c->nranks == 1, "psa_debug_cluster_labels is not available on a sharded context (%d ranks)", c->nranks);
    const ClusterOut out{size_counts, large_atoms, n_solid, n_clusters, largest, largest_label, labels, size_atoms, nullptr, nullptr, nullptr};
    return synchronised(c, debug_cluster_run(c, n_o, n_a, count, list, solid, bond_masks, link, n_sizes, out), "psa_debug_cluster_labels");
}

int psa_debug_qlm(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
                  const double* r_cut, int64_t frame, const int32_t* ls, int32_t n_ls, int64_t* q) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, debug_qlm_run(c, box, box_inverse, idx, group_start, n_groups, r_cut, frame, ls, n_ls, q), "psa_debug_qlm");
}

int psa_debug_neighbour_lists(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                              int32_t n_groups, const double* r_cut, int64_t frame, int32_t* count, int32_t* list) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, debug_lists_run(c, box, box_inverse, idx, group_start, n_groups, r_cut, frame, count, list),
                        "psa_debug_neighbour_lists");
}

}  // extern "C"
