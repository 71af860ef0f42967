// psa_adaptive_common_neighbours: the common-neighbour analysis with a cut-off per centre, derived from its nearest
// candidates, over time origins (definition: include/psa_hip.h; kernel: acna.hip; host core: api_shell.h).  It is
// psa_common_neighbours' call with the adaptive signature pass in place of the signature pass and the same census pass:
// behind the counts the types (8 n_a bytes per origin with their padding), the cut-offs (4 n_a) and, where the per-bond
// output is asked for, the members' columns and their bonds' words by rank (56 n_a each), inside the budget; the per-origin
// type counts ride behind the species' rows of the accumulator.
#include "api_shell.h"

namespace psa {

namespace {

// behind the counts of a block: the types (int32 and 4 bytes of padding), the cut-offs float32 and, with the per-bond output,
// the members' columns (14) int32 and their bonds' words (14) uint32
constexpr ShellLayout ACNA_LAYOUT{8, 4, 4 * ACNA_MEMBERS, 4 * ACNA_MEMBERS};
static_assert(ACNA_LAYOUT.first(2).bytes() == 12 && ACNA_LAYOUT.bytes() == 124, "12 bytes per atom and origin, 124 with the per-bond output");
// an item's samples, 64 centres x the origins of its slab x 14 bonds, fit 32 bits in every counter
static_assert((uint64_t)ANGLE_ITEM_CENTRES * ANGLE_MAX_SLAB * ACNA_MEMBERS < (1ull << 32), "an item's samples fit 32 bits");

struct AcnaOut {
    uint64_t* signature_counts;
    size_t    signature_bytes;
    uint64_t *signature_outside, *type_counts;
    size_t    type_bytes;
    uint64_t *truncated, *short_centres;
    int32_t * types, *n;
    float*    cutoffs;
    size_t    atom_bytes;
    int32_t*  nearest;
    uint32_t* bond_signatures;
    size_t    bond_bytes;
};

int acna_run(ShellCall& s, const AcnaOut& out) {
    PSA_REQUIRE(out.signature_counts != nullptr && out.signature_outside != nullptr && out.type_counts != nullptr && out.truncated != nullptr &&
                    out.short_centres != nullptr, "null output");
    const bool        bonds = out.nearest != nullptr || out.bond_signatures != nullptr;
    const ShellLayout layout = ACNA_LAYOUT.first(bonds ? 4 : 2);
    PSA_TRY(shell_check(&s, "psa_adaptive_common_neighbours", layout));
    psa_ctx*          c = s.c;
    const AtomGroups& p = s.p;
    const int         S = p.G;
    const int64_t     n_o = s.n_o, row = ACNA_ROW_WORDS, table = row - 3;
    const size_t      want_s = (size_t)S * (size_t)table * sizeof(uint64_t), want_t = (size_t)n_o * (size_t)S * CNA_TYPES * sizeof(uint64_t);
    const size_t      want_a = (size_t)n_o * (size_t)p.n_a * sizeof(int32_t), want_b = want_a * ACNA_MEMBERS;
    PSA_REQUIRE(out.signature_bytes == want_s, "signature_bytes is %zu, the (%d,%d,%d,%d) uint64 result has %zu", out.signature_bytes, S,
                CNA_MAX_J, CNA_MAX_K, CNA_MAX_L, want_s);
    PSA_REQUIRE(out.type_bytes == want_t, "type_bytes is %zu, the (%lld,%d,%d) uint64 result has %zu", out.type_bytes, (long long)n_o, S,
                CNA_TYPES, want_t);
    PSA_REQUIRE((out.types == nullptr && out.n == nullptr && out.cutoffs == nullptr) || out.atom_bytes == want_a, "atom_bytes is %zu, each "
                "(%lld,%lld) 32-bit per-atom result has %zu", out.atom_bytes, (long long)n_o, (long long)p.n_a, want_a);
    PSA_REQUIRE(!bonds || out.bond_bytes == want_b, "bond_bytes is %zu, each (%lld,%lld,%d) 32-bit per-bond result has %zu", out.bond_bytes,
                (long long)n_o, (long long)p.n_a, ACNA_MEMBERS, want_b);
    std::memset(out.signature_counts, 0, want_s);
    std::memset(out.type_counts, 0, want_t);
    for (uint64_t* o : {out.signature_outside, out.truncated, out.short_centres}) std::memset(o, 0, (size_t)S * sizeof(uint64_t));
    if (p.n_a == 0) return PSA_OK;                           // every species empty: zeros, nothing per atom
    const int64_t tail = n_o * S * CNA_TYPES;
    struct Rows {
        int*      types;
        float*    cut;
        int*      near;                                      // null without the per-bond output, and so is sigs
        unsigned* sigs;
    };
    const auto rows_of = [](const AngleWork& wk) {
        ShellCarve cv = wk.carve();
        Rows       r;
        r.types = cv.take<int>(), r.cut = cv.take<float>(), r.near = cv.take<int>(), r.sigs = cv.take<unsigned>();
        return r;
    };
    std::vector<uint64_t> acc;
    const ShellPass       passes = [&](const AngleWork& wk, int64_t n_items, int64_t k0, int64_t nb) -> int {
        const Rows r = rows_of(wk);
        PSA_TRY(launch_acna_signature(c, wk.c, wk.count, wk.list, c->d_rs_items.ptr, n_items, r.types, r.cut, r.near, r.sigs,
                                      c->d_rs_part.as<unsigned>(), s.box, p.n_a, nb));
        StageTimer census(c, PSA_T_PROJECT);                 // (inside the caller's PSA_T_PHASE, which spans both passes)
        return launch_cna_census(c, r.types, c->d_rs_acc.as<unsigned long long>() + (size_t)S * (size_t)row + (size_t)k0 * S * CNA_TYPES, s.sp,
                                 p.n_a, nb);
    };
    const ShellPass per_atom = [&](const AngleWork& wk, int64_t, int64_t k0, int64_t nb) -> int {
        const Rows r = rows_of(wk);
        return copy_atom_rows(c, p.n_a, k0, nb, {{out.types, r.types, sizeof(int32_t)}, {out.n, wk.count, sizeof(int32_t)},
                                                 {out.cutoffs, r.cut, sizeof(float)}, {out.nearest, r.near, ACNA_MEMBERS * sizeof(int32_t)},
                                                 {out.bond_signatures, r.sigs, ACNA_MEMBERS * sizeof(uint32_t)}});
    };
    const bool atoms = out.types != nullptr || out.n != nullptr || out.cutoffs != nullptr || bonds;
    PSA_TRY(shell_run(s, row, layout, passes, atoms ? per_atom : ShellPass(), &acc, tail));
    for (int a = 0; a < S; ++a) {
        const uint64_t* r = acc.data() + (size_t)a * (size_t)row;
        std::memcpy(out.signature_counts + (size_t)a * (size_t)table, r, (size_t)table * sizeof(uint64_t));
        out.signature_outside[a] = r[table], out.truncated[a] = r[table + 1], out.short_centres[a] = r[table + 2];
    }
    std::memcpy(out.type_counts, acc.data() + (size_t)S * (size_t)row, want_t);
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_adaptive_common_neighbours(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                                   int32_t n_groups, const double* r_cut, int64_t origin_step, uint64_t* signature_counts,
                                   size_t signature_bytes, uint64_t* signature_outside, uint64_t* type_counts, size_t type_bytes,
                                   uint64_t* truncated, uint64_t* short_centres, int32_t* types, int32_t* n, float* cutoffs, size_t atom_bytes,
                                   int32_t* nearest, uint32_t* bond_signatures, size_t bond_bytes) {
    PSA_TRY(enter(c));
    Guard         guard(c);
    ShellCall     s{c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step};
    const AcnaOut out{signature_counts, signature_bytes, signature_outside, type_counts, type_bytes, truncated, short_centres, types, n,
                      cutoffs, atom_bytes, nearest, bond_signatures, bond_bytes};
    return synchronised(c, acna_run(s, out), "psa_adaptive_common_neighbours");
}

}  // extern "C"
