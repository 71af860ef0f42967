// The folded D image of the low-rank route's folded pair launch (k1_lowrank_fold.hip): one 512-row block of D' = D + E
// (k1_planes_diff.hip, diff_fold_table_kernel) cut for its two roles.  Rows 0..127 go to role A, which projects them
// beside the 128 node rows; rows 128..511 to role B.  Each role's part is what its LDS-DMA streams, stage after stage:
//     role A part: [atom stage][unit x = 0..7 ][16 rows][32 atoms]   unit x = 2 mt + h holds row tile 4 h + mt
//     role B part: [atom stage][unit x = 0..23][16 rows][32 atoms]   unit x = 2 mt + h holds row tile 8 + 12 h + mt
// (h: the row half a wavefront owns, mt: its row tile, as in k1_lowrank_pair.h).  The 16-byte slots of a row are
// swizzled as in pd16_index.  Each part ends with 4 stages of padding: a role fetches up to three stages past the end
// and never reads them.
#pragma once
#include "k1_tile.h"

namespace psa {

constexpr int LRF_ROWS = 512;                            // rows of the block (one D block: 2K <= 512)
constexpr int LRF_A_ROWS = 128, LRF_A_MT = 4, LRF_A_UNITS = 2 * LRF_A_MT;   // D' rows, row tiles per row half, D' units per stage of role A
constexpr int LRF_B_MT = 12, LRF_B_UNITS = 2 * LRF_B_MT; // row tiles per row half and D' units per stage of role B
constexpr int LRF_PAD_STAGES = 4;
static_assert(LRF_A_ROWS == 16 * LRF_A_UNITS && LRF_A_ROWS + 16 * LRF_B_UNITS == LRF_ROWS, "the two roles share the block's rows");

// first unit of role B's part
__host__ __device__ inline size_t lrf_b_first_unit(int n_stage) { return (size_t)(n_stage + LRF_PAD_STAGES) * LRF_A_UNITS; }
// element (row m < 512, atom a) of the image (float16 elements; one unit = 16 x K1_BA of them)
__host__ __device__ inline size_t pd16_fold_index(int m, int a, int n_stage) {
    const int rt = m >> 4, r = m & 15, al = a % K1_BA, st = a / K1_BA;
    size_t    unit;
    if (rt < LRF_A_UNITS) {
        unit = (size_t)st * LRF_A_UNITS + (size_t)(2 * (rt % LRF_A_MT) + rt / LRF_A_MT);
    } else {
        const int rb = rt - LRF_A_UNITS, h = rb / LRF_B_MT, mt = rb % LRF_B_MT;
        unit = lrf_b_first_unit(n_stage) + (size_t)st * LRF_B_UNITS + (size_t)(2 * mt + h);
    }
    return unit * (16 * K1_BA) + (size_t)r * K1_BA + (size_t)((((al >> 3) ^ pl_swizzle(r)) << 3) + (al & 7));
}
// bytes of the image, padding included (the same as the two-pass image of one block: pd16_table_bytes)
__host__ __device__ inline size_t pd16_fold_table_bytes(int n_stage) {
    return (size_t)(n_stage + LRF_PAD_STAGES) * (LRF_A_UNITS + LRF_B_UNITS) * 1024;
}

}  // namespace psa
