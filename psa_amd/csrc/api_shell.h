// What the entries on the neighbour shells share on the host (api_shell.hip): api_angle.hip (bond angles, coordination),
// api_order.hip (q_l, the local order), api_cluster.hip (solid clusters), api_persist.hip (bond persistence), api_cna.hip
// (common neighbours) and api_acna.hip (adaptive common neighbours).  Each of them is one call description (ShellCall), one
// layout of what it keeps behind the counts (ShellLayout), a pass over the items and, where it has something to take out of
// a block, an `after`, run by shell_run.
//
// Budget (PSA_OPT_DYNAMIC_WORK_BYTES = W): per origin of a block the centred fractional coordinates of the listed atoms
// (12 n_a bytes), their neighbour counts (4 n_a), their neighbour lists (64 x 16 n_a) and what the entry's layout adds per
// atom: (1040 + layout) n_a bytes; a block is a whole number of origins, W / ((1040 + layout) n_a) of them, and a budget
// below one origin is refused.  The item table, the bin edges, the partials, the accumulator and the result lie outside it.
// Per block: the fraction pass, the neighbour pass, the entry's pass over the items, the reduce into the accumulator that
// lives across blocks.
#pragma once
#include "api_internal.h"

namespace psa {

constexpr int64_t ANGLE_ITEM_CENTRES = 64;      // centres of an item of the angle pass: 16 per wavefront and origin
// most origins of an item: 64 centres x 8192 origins x 2016 pairs of 64 neighbours stay below 2^32
constexpr int64_t ANGLE_MAX_SLAB = 8192;
static_assert((uint64_t)ANGLE_ITEM_CENTRES * ANGLE_MAX_SLAB * (ANGLE_MAX_NEIGHBOURS * (ANGLE_MAX_NEIGHBOURS - 1) / 2) < (1ull << 32),
              "an item's samples fit 32 bits");
constexpr int64_t ANGLE_ORIGIN_BYTES = 12 + 4 + 16 * ANGLE_MAX_NEIGHBOURS;   // per atom and origin

// What an entry keeps behind the counts of a block, stated once: the bytes of a row (an atom at an origin) of each array, in
// order.  bytes(): of a row of them all -- what the budget and the work buffer add per atom and origin; ShellCarve: the arrays
// of a block of `cap` rows, one behind the other.  first(k): the first k arrays alone; behind(front): behind an array more
struct ShellLayout {
    int64_t size[6] = {};
    int     n = 0;
    constexpr ShellLayout() = default;
    constexpr ShellLayout(std::initializer_list<int64_t> sizes) {
        for (int64_t s : sizes) size[n++] = s;
    }
    constexpr int64_t bytes() const {
        int64_t b = 0;
        for (int i = 0; i < n; ++i) b += size[i];
        return b;
    }
    constexpr ShellLayout first(int k) const {
        ShellLayout l = *this;
        l.n = k;
        return l;
    }
    constexpr ShellLayout behind(int64_t front) const {
        ShellLayout l{front};
        for (int i = 0; i < n; ++i) l.size[l.n++] = size[i];
        return l;
    }
};
struct ShellCarve {
    ShellLayout layout;
    char*       at;
    size_t      cap;
    int         i = 0;
    // the next array of the layout; null once the layout holds no more
    template <class T> T* take() {
        if (i >= layout.n) return nullptr;
        T* p = reinterpret_cast<T*>(at);
        at += cap * (size_t)layout.size[i++];
        return p;
    }
};

// A call on the neighbour shells.  The C entry fills the caller's arguments (origin_step: 1 for the entries of one frame);
// shell_check fills p, sp and n_o, the origins 0, origin_step, ... of the call
struct ShellCall {
    psa_ctx*       c;
    const double * box, *box_inverse;
    const int32_t* idx;
    const int64_t* group_start;
    int32_t        n_groups;
    const double*  r_cut;
    int64_t        origin_step;
    AtomGroups     p;
    AngleSpecies   sp;
    int64_t        n_o = 0;
};

// What r_cut and psa_bond_persistence's r_break share per entry (a, b) of an S x S cut-off matrix `name`: the symmetry; the
// served radius of `name`[a][b] = r and its float32 reciprocal (0 for r = 0: no bond).  Two halves, since r_break has a
// condition of its own between them
int cutoff_symmetric(const char* name, const double* m, int S, int a, int b);
int cutoff_reciprocal(const double* box_inverse, const char* name, int a, int b, double r, float* inv);

// the shared checks, the cut-offs, the budget (layout: what the entry keeps behind the counts) and origin_step; fills s->p,
// s->sp and s->n_o.  p.Ab: the origins of a block, as many of the n_o as the budget and the fraction pass's grid (65535)
// hold -- the one place that decides it
int shell_check(ShellCall* s, const char* entry, const ShellLayout& layout = {});

// the work buffer of a block of B origins: the lists first (16-byte entries), then c, then the counts, then at x the arrays
// of `behind` (a multiple of 8 bytes per atom and origin: psa_bond_order's X), `cap` = B n_a rows each
struct AngleWork {
    float4*     list;
    float*      c;
    int*        count;
    long long*  x;
    ShellLayout behind;
    size_t      cap;
    ShellCarve  carve() const { return ShellCarve{behind, reinterpret_cast<char*>(x), cap}; }
};
int angle_work(psa_ctx* c, int64_t n_a, int64_t B, const ShellLayout& behind, AngleWork* w);

// The items of the angle pass over n_ob origins, species by species, ANGLE_ITEM_CENTRES centres each; first (S + 1): where
// each species' items begin.  The partials (items x row words) stay below 64 MiB where one slab per tile allows
std::vector<AngleItem> angle_items(const AtomGroups& p, int64_t n_ob, int64_t row, int32_t* first);

// What a call on the neighbour shells runs after its checks: the item table over the origins of a block, the uploads of the
// atom list and the table, the accumulator (S, row) zeroed; per block the fraction pass, the neighbour pass, the caller's
// `pass` over the items into the partials, the reduce, and `after` where the caller has something to take out of the block
// before the next one overwrites it; at the end the accumulator on the host.
// layout: as for shell_check; tail: uint64 words of the caller's behind the species' rows of the accumulator, zeroed and
// returned with them
using ShellPass = std::function<int(const AngleWork& w, int64_t n_items, int64_t k0, int64_t nb)>;
int shell_run(ShellCall& s, int64_t row, const ShellLayout& layout, const ShellPass& pass, const ShellPass& after, std::vector<uint64_t>* acc,
              int64_t tail = 0);

// A block's per-atom rows to the caller's arrays: per output the caller's array over all origins (null: not asked for), the
// block's rows on the device and the bytes of a cell, one per (origin, atom)
struct AtomRows { void* host; const void* dev; size_t cell; };
int copy_atom_rows(psa_ctx* c, int64_t n_a, int64_t k0, int64_t nb, std::initializer_list<AtomRows> rows);

// What the two entries of one frame start with after shell_check: the frame refused outside [0, T - 1]; then, unless no atom
// is listed (w->list stays null), the atom list uploaded, the work buffer of one origin and the fraction pass and the
// neighbour pass of that frame into it
int shell_one_frame(ShellCall& s, int64_t frame, const ShellLayout& layout, AngleWork* w);

// N_lm = (-1)^m sqrt(1 / prod_{k = l-m+1 .. l+m} k), the product in float64 in ascending k, at [l * 13 + m]; behind it the
// caller's 3j blocks, (2 l + 1)^2 each, one per LOCAL_W3J_WORDS
int upload_local_tables(psa_ctx* c, const int32_t* ls, int32_t n_ls, const double* w3j);

}  // namespace psa
