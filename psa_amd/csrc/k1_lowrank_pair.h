// The D image of the low-rank route's pair launch (k1_lowrank_pair.hip): one 512-row block cut for its two roles.
// Rows 0..63 go to role A, which projects them beside the 128 node rows; rows 64..511 to role B.  Each role's part is
// what its LDS-DMA streams, stage after stage:
//     role A part: [atom stage][unit x = 0..3 ][16 rows][32 atoms]   unit x = 2 mt + h holds row tile 2 h + mt
//     role B part: [atom stage][unit x = 0..27][16 rows][32 atoms]   unit x = 2 mt + h holds row tile 4 + 14 h + mt
// (h: the row half a wavefront owns, mt: its row tile; the halves alternate so that a wavefront's lane base carries h and
// the unit offset stays even: unit_off, k1_f16.h).  The 16-byte slots of a row are swizzled as in pd16_index.  Each part
// ends with 4 stages of padding: a role fetches up to three stages past the end and never reads them.
#pragma once
#include "k1_tile.h"

namespace psa {

constexpr int LRP_ROWS = 512;                            // rows of the block (one D block: 2K <= 512)
constexpr int LRP_A_ROWS = 64, LRP_A_UNITS = 4;          // D rows and D units per stage of role A
constexpr int LRP_B_MT = 14, LRP_B_UNITS = 2 * LRP_B_MT; // row tiles per row half and D units per stage of role B
constexpr int LRP_PAD_STAGES = 4;
static_assert(LRP_A_ROWS + 16 * LRP_B_UNITS == LRP_ROWS, "the two roles share the block's rows");

// first unit of role B's part
__host__ __device__ inline size_t lrp_b_first_unit(int n_stage) { return (size_t)(n_stage + LRP_PAD_STAGES) * LRP_A_UNITS; }
// element (row m < 512, atom a) of the image (float16 elements; one unit = 16 x K1_BA of them)
__host__ __device__ inline size_t pd16_pair_index(int m, int a, int n_stage) {
    const int rt = m >> 4, r = m & 15, al = a % K1_BA, st = a / K1_BA;
    size_t    unit;
    if (rt < LRP_A_UNITS) {
        unit = (size_t)st * LRP_A_UNITS + (size_t)(2 * (rt & 1) + (rt >> 1));
    } else {
        const int rb = rt - LRP_A_UNITS, h = rb / LRP_B_MT, mt = rb % LRP_B_MT;
        unit = lrp_b_first_unit(n_stage) + (size_t)st * LRP_B_UNITS + (size_t)(2 * mt + h);
    }
    return unit * (16 * K1_BA) + (size_t)r * K1_BA + (size_t)((((al >> 3) ^ pl_swizzle(r)) << 3) + (al & 7));
}
// bytes of the image, padding included (the same as the two-pass image of one block: pd16_table_bytes)
__host__ __device__ inline size_t pd16_pair_table_bytes(int n_stage) {
    return (size_t)(n_stage + LRP_PAD_STAGES) * (LRP_A_UNITS + LRP_B_UNITS) * 1024;
}

}  // namespace psa
