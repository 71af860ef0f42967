// What every K1 projection kernel shares whatever its arithmetic (k1_mfma.hip, k1_split.hip and, through
// k1_f16.h, the "2 x f16" kernels): the XCD-aware block map with the grid that goes with it, and the slot
// swizzles of the LDS images.  One definition each -- a new kernel uses these, it does not copy them.
#pragma once
#include "psa_ctx.h"

namespace psa {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// XCD-aware block map.  The hardware deals consecutive workgroups round-robin to the eight XCDs, so blocks b and
// b + 8 share an XCD and its L2: they get the M blocks of ONE frame tile, the tile's data (V rows or planes) comes
// from HBM once and the second read is an L2 hit.  The grid (k1_grid below) rounds the frame tiles up to eight;
// false for the blocks past the last tile, which return at once.
__device__ __forceinline__ bool k1_block_map(int n_mblk, int n_tblk, int& mb, int& tb) {
    const int b = blockIdx.x;
    const int r8 = b >> 3;
    mb = r8 % n_mblk;
    tb = (r8 / n_mblk) * 8 + (b & 7);
    return tb < n_tblk;
}

// the launch side of k1_block_map: M blocks of m_blk rows x frame tiles of t_blk frames
struct K1Grid {
    int      n_mblk, n_tblk;
    unsigned blocks;
};
inline int k1_grid(const ProjGeom& g, int m_blk, int t_blk, K1Grid& o) {
    const int     n_mblk = g.M_pad / m_blk;
    const int64_t n_tblk = (g.T + t_blk - 1) / t_blk;
    const int64_t grid = ((n_tblk + 7) / 8) * 8 * n_mblk;
    PSA_REQUIRE(grid < (1ll << 31) && n_tblk < (1ll << 31), "projection grid too large");
    o = K1Grid{n_mblk, (int)n_tblk, (unsigned)grid};
    return PSA_OK;
}

// float32 V rows (96 floats = 24 slots of 16 bytes per frame): slot s of row `row` is stored at this physical
// slot.  LDS-DMA writes 1 KiB linearly per instruction, so rows cannot be padded; the swizzle goes on the per-lane
// source address and on the read (an involution).
__device__ __forceinline__ int vs_phys_slot(int s, int row) { return (s & ~7) | ((s & 7) ^ (row & 7)); }

// 16-bit tile images (32 atoms = four 16-byte slots per row): slot q of row r is stored at q ^ g((r >> 2) & 3),
// g = {0, 2, 3, 1} packed two bits each as 0x78, which makes the four 16-lane groups of a fragment's
// ds_read_b128 conflict-free
__host__ __device__ __forceinline__ int pl_swizzle(int r) { return (0x78 >> (2 * ((r >> 2) & 3))) & 3; }

}  // namespace psa
