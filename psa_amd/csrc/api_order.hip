// psa_bond_order, psa_local_order, psa_debug_qlm: the Steinhardt order parameters q_l and the local order parameters
// (q-bar_l, w_l, solid-like bonds) of the neighbour shells over time origins (definition: include/psa_hip.h; host core:
// api_shell.h).
//
// psa_bond_order (kernel: order.hip) is psa_angle_histogram's call with the order pass in place of the angle pass: the same
// checks, work buffer, items and reduce; with per-atom output the block's X (8 n_l n_a bytes per origin) lies behind the
// counts, inside the budget, and every block's X and counts are copied to the caller's arrays before the next block
// overwrites them.
//
// psa_local_order and psa_debug_qlm (kernels: qlm.hip) are the same call again with two passes in place of the angle pass:
// the first leaves the table of the Q_lm (16 sum (l + 1) n_a bytes per origin) behind the counts, the second gathers from
// it; the per-atom rows ((24 n_l + 8) n_a bytes per origin) lie behind the table, all inside the budget.
#include "api_shell.h"

namespace psa {

namespace {

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

// behind the counts of psa_bond_order, with per-atom output: X (n_l) int64
constexpr ShellLayout order_layout(int n_l) { return ShellLayout{8 * (int64_t)n_l}; }
static_assert(order_layout(ORDER_MAX_LS).bytes() == 8 * ORDER_MAX_LS, "8 n_l bytes per atom and origin");
// an item's samples of the order pass, 64 centres x the origins of a block x n_l, fit 32 bits whatever the slabs
static_assert((uint64_t)ANGLE_ITEM_CENTRES * 65535 * ORDER_MAX_LS < (1ull << 32), "an item's samples fit 32 bits");

int order_run(ShellCall& s, const int32_t* ls, int32_t n_ls, int32_t n_q, uint64_t* hist, size_t hist_bytes, uint64_t* truncated,
              uint64_t* isolated, uint64_t* undefined, int64_t* x, int32_t* n) {
    PSA_REQUIRE(hist != nullptr && truncated != nullptr && isolated != nullptr && undefined != nullptr, "null output");
    LocalLs all;
    PSA_TRY(ascending_orders(ls, n_ls, ORDER_MAX_LS, 1, false, &all));
    const OrderLs     o{all.n_l, all.l_max, all.mask};
    const ShellLayout layout = order_layout(n_ls).first(x != nullptr ? 1 : 0);
    PSA_TRY(shell_check(&s, "psa_bond_order", layout));
    psa_ctx*          c = s.c;
    const AtomGroups& p = s.p;
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
        return launch_order_hist(c, w.count, w.list, c->d_rs_items.ptr, n_items, c->d_rs_part.as<unsigned>(), w.carve().take<long long>(), o,
                                 p.n_a, nb, n_q);
    };
    const ShellPass per_atom = [&](const AngleWork& w, int64_t, int64_t k0, int64_t nb) -> int {
        return copy_atom_rows(c, p.n_a, k0, nb, {{x, w.carve().take<long long>(), (size_t)n_ls * sizeof(int64_t)}, {n, w.count, sizeof(int32_t)}});
    };
    PSA_TRY(shell_run(s, row, layout, order_pass, x != nullptr || n != nullptr ? per_atom : ShellPass(), &acc));
    for (int a = 0; a < S; ++a) {
        const uint64_t* r = acc.data() + (size_t)a * (size_t)row;
        std::memcpy(hist + (size_t)a * bins, r, bins * sizeof(uint64_t));
        truncated[a] = r[bins], isolated[a] = r[bins + 1], undefined[a] = r[bins + 2];
    }
    return PSA_OK;
}

// behind the counts of psa_local_order: the table of the Q_lm (columns, 2) int64; with per-atom output q-bar^2, w, w-bar
// (n_l) float64 each -- the three of the nb origins a pass runs over one behind the other, in the room of a whole block's --,
// the connections and 4 bytes of padding
constexpr ShellLayout local_layout(int columns, int n_l) { return ShellLayout{16 * (int64_t)columns, 24 * (int64_t)n_l, 4, 4}; }
static_assert(local_layout(7, 1).first(1).bytes() == 16 * 7 && local_layout(7, 1).bytes() == 16 * 7 + 24 * 1 + 8,
              "16 columns bytes per atom and origin, 24 n_l + 8 more with the per-atom output");
// an item's samples of the local order pass, 64 centres x the origins of a block, fit 32 bits in every counter
static_assert((uint64_t)ANGLE_ITEM_CENTRES * 65535 < (1ull << 32), "an item's samples fit 32 bits");

int local_order_run(ShellCall& s, const int32_t* ls, int32_t n_ls, int32_t n_q, int32_t n_w, double w_range, int32_t solid_l,
                    double solid_threshold, const double* w3j, int64_t w3j_count, uint64_t* hist, size_t hist_bytes, double* qbar2, double* w,
                    double* wbar, int32_t* connections, int32_t* n) {
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
    const bool        atoms = qbar2 != nullptr || w != nullptr || wbar != nullptr || connections != nullptr;
    const ShellLayout layout = local_layout(o.columns, n_ls).first(atoms ? 4 : 1);
    PSA_TRY(shell_check(&s, "psa_local_order", layout));
    psa_ctx*          c = s.c;
    const AtomGroups& p = s.p;
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
    struct Rows {
        long long* q;
        double*    values;
        int*       xi;
    };
    const auto rows_of = [](const AngleWork& wk) {
        ShellCarve cv = wk.carve();
        return Rows{cv.take<long long>(), cv.take<double>(), cv.take<int>()};
    };
    std::vector<uint64_t> acc;
    const ShellPass       passes = [&](const AngleWork& wk, int64_t n_items, int64_t, int64_t nb) -> int {
        const Rows r = rows_of(wk);
        PSA_TRY(launch_qlm_sum(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, d_norm, r.q, o, p.n_a, nb));
        StageTimer second(c, PSA_T_PROJECT);                 // (inside the caller's PSA_T_PHASE, which spans both passes)
        return launch_local_order(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, r.q, d_norm + LOCAL_NORM_WORDS, c->d_rs_part.as<unsigned>(),
                                  r.values, r.xi, o, bins, p.n_a, nb);
    };
    const ShellPass per_atom = [&](const AngleWork& wk, int64_t, int64_t k0, int64_t nb) -> int {
        const Rows   r = rows_of(wk);
        const size_t each = atoms ? (size_t)nb * (size_t)p.n_a * (size_t)n_ls : 0, cell = (size_t)n_ls * sizeof(double);
        return copy_atom_rows(c, p.n_a, k0, nb, {{qbar2, r.values, cell}, {w, r.values + each, cell}, {wbar, r.values + 2 * each, cell},
                                                 {connections, r.xi, sizeof(int32_t)}, {n, wk.count, sizeof(int32_t)}});
    };
    PSA_TRY(shell_run(s, row, layout, passes, atoms || n != nullptr ? per_atom : ShellPass(), &acc));
    std::memcpy(hist, acc.data(), want);
    return PSA_OK;
}

// the fraction pass, the neighbour pass and the q_lm pass of one frame: Q (n_a, columns, 2) int64
int debug_qlm_run(ShellCall& s, int64_t frame, const int32_t* ls, int32_t n_ls, int64_t* q) {
    PSA_REQUIRE(q != nullptr, "null output");
    LocalLs o;
    PSA_TRY(ascending_orders(ls, n_ls, LOCAL_MAX_LS, 2, true, &o));   // at most four, even, in [2, 12]
    o.solid_l = ls[0];
    const ShellLayout layout = local_layout(o.columns, n_ls).first(1);
    AngleWork         w;
    PSA_TRY(shell_check(&s, "psa_debug_qlm", layout));
    PSA_TRY(shell_one_frame(s, frame, layout, &w));
    psa_ctx*          c = s.c;
    const AtomGroups& p = s.p;
    if (p.n_a == 0) return PSA_OK;
    int32_t                      first[PAIR_MAX_SPECIES + 1];
    const std::vector<AngleItem> items = angle_items(p, 1, 1, first);
    long long*                   d_q = w.carve().take<long long>();
    PSA_TRY(upload(c, c->d_rs_items, items.data(), items.size() * sizeof(AngleItem)));
    PSA_TRY(upload_local_tables(c, ls, n_ls, nullptr));
    PSA_TRY(launch_qlm_sum(c, w.count, w.list, c->d_rs_items.ptr, (int64_t)items.size(), c->d_local_tab.as<double>(), d_q, o, p.n_a, 1));
    PSA_HIP_CHECK(hipMemcpyAsync(q, d_q, (size_t)p.n_a * (size_t)layout.bytes(), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_bond_order(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                   int32_t n_groups, const double* r_cut, int64_t origin_step, const int32_t* ls, int32_t n_ls, int32_t n_q, uint64_t* hist,
                   size_t hist_bytes, uint64_t* truncated, uint64_t* isolated, uint64_t* undefined, int64_t* x, int32_t* n) {
    PSA_TRY(enter(c));
    Guard     guard(c);
    ShellCall s{c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step};
    return synchronised(c, order_run(s, ls, n_ls, n_q, hist, hist_bytes, truncated, isolated, undefined, x, n), "psa_bond_order");
}

int psa_local_order(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                    int32_t n_groups, const double* r_cut, int64_t origin_step, const int32_t* ls, int32_t n_ls, int32_t n_q, int32_t n_w,
                    double w_range, int32_t solid_l, double solid_threshold, const double* w3j, int64_t w3j_count, uint64_t* hist,
                    size_t hist_bytes, double* qbar2, double* w, double* wbar, int32_t* connections, int32_t* n) {
    PSA_TRY(enter(c));
    Guard     guard(c);
    ShellCall s{c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step};
    return synchronised(c, local_order_run(s, ls, n_ls, n_q, n_w, w_range, solid_l, solid_threshold, w3j, w3j_count, hist, hist_bytes, qbar2, w,
                                           wbar, connections, n), "psa_local_order");
}

int psa_debug_qlm(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start, int32_t n_groups,
                  const double* r_cut, int64_t frame, const int32_t* ls, int32_t n_ls, int64_t* q) {
    PSA_TRY(enter(c));
    Guard     guard(c);
    ShellCall s{c, box, box_inverse, idx, group_start, n_groups, r_cut, 1};
    return synchronised(c, debug_qlm_run(s, frame, ls, n_ls, q), "psa_debug_qlm");
}

}  // extern "C"
