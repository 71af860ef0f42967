// psa_solid_clusters, psa_debug_cluster_labels: the connected components of the solid atoms of the neighbour shells over time
// origins (definition: include/psa_hip.h; kernels: cluster.hip, qlm.hip's q_lm pass; host core: api_shell.h).
//
// psa_solid_clusters is psa_local_order's call with the q_lm pass of the one order solid_l and the four cluster passes:
// behind the table the masks, xi, parent / label and size (20 n_a bytes per origin), inside the budget; the size histogram,
// the error word and the per-origin results ride behind the species' rows of the accumulator.
// psa_debug_cluster_labels drives the hook, flatten and stats passes alone on a graph of the caller's.
#include "api_shell.h"

namespace psa {

namespace {

// behind the table of a block (psa_debug_cluster_labels: behind the counts): the masks, then xi, parent and size
constexpr ShellLayout CLUSTER_LAYOUT{8, 4, 4, 4};
static_assert(CLUSTER_LAYOUT.bytes() == 20, "20 bytes per atom and origin");
static_assert(CLUSTER_LAYOUT.behind(16 * (6 + 1)).bytes() == 16 * (6 + 1) + 20, "behind the 16 (solid_l + 1) bytes of the table");
ClusterWork cluster_work(ShellCarve cv) { return ClusterWork{cv.take<unsigned long long>(), cv.take<int>(), cv.take<int>(), cv.take<int>()}; }

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

int cluster_run(ShellCall& s, int32_t solid_l, double solid_threshold, int32_t min_connections, int32_t link, int32_t n_sizes,
                uint64_t* species_rows, const ClusterOut& out) {
    PSA_REQUIRE(species_rows != nullptr, "null output");
    PSA_TRY(cluster_out_check(out, link, n_sizes));
    PSA_REQUIRE(solid_l >= 2 && solid_l <= ORDER_MAX_L && solid_l % 2 == 0, "solid_l = %d is not an even order in [2, %d]", (int)solid_l, ORDER_MAX_L);
    PSA_REQUIRE(solid_threshold > 0.0 && solid_threshold <= 1.0, "the solid-like threshold is in (0, 1], got %g", solid_threshold);
    PSA_REQUIRE(min_connections >= 0 && min_connections <= ANGLE_MAX_NEIGHBOURS, "min_connections is in [0, %d], got %d", ANGLE_MAX_NEIGHBOURS,
                (int)min_connections);
    const LocalLs     o{1, (int)solid_l, (int)solid_l + 1, (int)solid_l, 1u << solid_l};
    const ShellLayout layout = CLUSTER_LAYOUT.behind(16 * (int64_t)o.columns);   // the table of the Q_lm in front
    PSA_TRY(shell_check(&s, "psa_solid_clusters", layout));
    psa_ctx*          c = s.c;
    const AtomGroups& p = s.p;
    const int         S = p.G;
    const int64_t     n_o = s.n_o, row = CLUSTER_ROW_WORDS;
    const size_t      want = (size_t)S * (size_t)row * sizeof(uint64_t);
    std::memset(species_rows, 0, want);
    if (p.n_a == 0) {                                        // every species empty: zeros, no cluster
        cluster_out_empty(out, n_sizes, n_o);
        return PSA_OK;
    }
    PSA_TRY(upload_local_tables(c, &solid_l, 1, nullptr));
    const double* d_norm = c->d_local_tab.as<double>();
    const double  thr2 = solid_threshold * solid_threshold;
    const int64_t words = cluster_stat_words(n_sizes);
    const auto    tail_of = [&]() { return c->d_rs_acc.as<unsigned long long>() + (size_t)S * (size_t)row; };
    struct Block {
        long long*  q;
        ClusterWork w;
    };
    const auto block_of = [](const AngleWork& wk) {
        ShellCarve cv = wk.carve();
        return Block{cv.take<long long>(), cluster_work(cv)};
    };
    std::vector<uint64_t> acc;
    const ShellPass       passes = [&](const AngleWork& wk, int64_t n_items, int64_t, int64_t nb) -> int {
        const auto [d_q, w] = block_of(wk);
        int*       d_err = reinterpret_cast<int*>(tail_of() + words);
        PSA_TRY(launch_qlm_sum(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, d_norm, d_q, o, p.n_a, nb));
        PSA_TRY(launch_cluster_bonds(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, d_q, c->d_rs_part.as<unsigned>(), w, o, thr2,
                                     min_connections, p.n_a, nb));
        {
            StageTimer hook(c, PSA_T_PROJECT);               // (inside the caller's PSA_T_PHASE, which spans the four passes)
            PSA_TRY(launch_cluster_hook(c, wk.count, wk.list, c->d_rs_items.ptr, n_items, w, link, false, d_err, p.n_a, nb));
        }
        StageTimer flatten(c, PSA_T_FFT);
        return launch_cluster_flatten(c, w, d_err, p.n_a, nb);
    };
    const ShellPass block = [&](const AngleWork& wk, int64_t, int64_t k0, int64_t nb) -> int {
        return cluster_block(c, block_of(wk).w, wk.count, tail_of(), n_sizes, p.n_a, k0, nb, out);
    };
    PSA_TRY(shell_run(s, row, layout, passes, block, &acc, cluster_tail_words(n_sizes, n_o)));
    std::memcpy(species_rows, acc.data(), want);
    return cluster_out_tail(acc.data() + (size_t)S * (size_t)row, n_sizes, n_o, out);
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
    const size_t  bytes = (size_t)cap * (size_t)(ANGLE_ORIGIN_BYTES + CLUSTER_LAYOUT.bytes());
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
    PSA_TRY(angle_work(c, n_a, n_o, CLUSTER_LAYOUT, &wk));
    const ClusterWork w = cluster_work(wk.carve());
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

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_solid_clusters(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                       int32_t n_groups, const double* r_cut, int64_t origin_step, int32_t solid_l, double solid_threshold,
                       int32_t min_connections, int32_t link, int32_t n_sizes, uint64_t* species_rows, uint64_t* size_counts,
                       uint64_t* large_atoms, int32_t* n_solid, int32_t* n_clusters, int32_t* largest, int32_t* largest_label, int32_t* labels,
                       int32_t* size_atoms, int32_t* connections, int32_t* n, uint64_t* bond_masks) {
    PSA_TRY(enter(c));
    Guard            guard(c);
    ShellCall        s{c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step};
    const ClusterOut out{size_counts, large_atoms, n_solid, n_clusters, largest, largest_label, labels, size_atoms, connections, n, bond_masks};
    return synchronised(c, cluster_run(s, solid_l, solid_threshold, min_connections, link, n_sizes, species_rows, out), "psa_solid_clusters");
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

}  // extern "C"
