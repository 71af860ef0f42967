// The folded D image of the low-rank route's 48-node pair launch (k1_lowrank_n48.hip): one 512-row block of D'
// (k1_planes_diff.hip, diff_n48_table_kernel) cut for its two roles.  Rows 0..159 go to role A, which projects them beside
// the 96 node rows; rows 160..511 to role B.  Each role's part is what its LDS-DMA streams, stage after stage:
//     role A part: [atom stage][unit x = 0..9 ][16 rows][32 atoms]   unit x = 2 mt + h holds row tile 5 h + mt
//     role B part: [atom stage][unit x = 0..21][16 rows][32 atoms]   unit x = 2 mt + h holds row tile 10 + 11 h + mt
// (h: the row half a wavefront owns, mt: its row tile, as in k1_lowrank_fold.h).  The 16-byte slots of a row are
// swizzled as in pd16_index.  Each part ends with 4 stages of padding: a role fetches up to three stages past the end
// and never reads them.
#pragma once
#include "k1_tile.h"

namespace psa {

constexpr int LOWRANK_NODES_48 = 48;                     // the route's smaller node count (psa_set_k1_lowrank_nodes)
constexpr int LRN_ROWS = 512;                            // rows of the block (one D block: 2K <= 512)
constexpr int LRN_NODE_MT = 3;                           // node row tiles per row half: 96 node rows
constexpr int LRN_A_ROWS = 160, LRN_A_MT = 5, LRN_A_UNITS = 2 * LRN_A_MT;   // D' rows, row tiles per row half, D' units per stage of role A
constexpr int LRN_B_MT = 11, LRN_B_UNITS = 2 * LRN_B_MT; // row tiles per row half and D' units per stage of role B
constexpr int LRN_PAD_STAGES = 4;
static_assert(2 * 16 * LRN_NODE_MT == 2 * LOWRANK_NODES_48, "six row tiles hold the 48 nodes' cos and sin rows");
static_assert(LRN_A_ROWS == 16 * LRN_A_UNITS && LRN_A_ROWS + 16 * LRN_B_UNITS == LRN_ROWS, "the two roles share the block's rows");
static_assert(2 * LRN_NODE_MT + LRN_A_MT == LRN_B_MT, "both roles multiply the same per stage");

// first unit of role B's part
__host__ __device__ inline size_t lrn_b_first_unit(int n_stage) { return (size_t)(n_stage + LRN_PAD_STAGES) * LRN_A_UNITS; }
// element (row m < 512, atom a) of the image (float16 elements; one unit = 16 x K1_BA of them)
__host__ __device__ inline size_t pd16_n48_index(int m, int a, int n_stage) {
    const int rt = m >> 4, r = m & 15, al = a % K1_BA, st = a / K1_BA;
    size_t    unit;
    if (rt < LRN_A_UNITS) {
        unit = (size_t)st * LRN_A_UNITS + (size_t)(2 * (rt % LRN_A_MT) + rt / LRN_A_MT);
    } else {
        const int rb = rt - LRN_A_UNITS, h = rb / LRN_B_MT, mt = rb % LRN_B_MT;
        unit = lrn_b_first_unit(n_stage) + (size_t)st * LRN_B_UNITS + (size_t)(2 * mt + h);
    }
    return unit * (16 * K1_BA) + (size_t)r * K1_BA + (size_t)((((al >> 3) ^ pl_swizzle(r)) << 3) + (al & 7));
}
// bytes of the image, padding included (the same as the two-pass image of one block: pd16_table_bytes)
__host__ __device__ inline size_t pd16_n48_table_bytes(int n_stage) {
    return (size_t)(n_stage + LRN_PAD_STAGES) * (LRN_A_UNITS + LRN_B_UNITS) * 1024;
}

}  // namespace psa
