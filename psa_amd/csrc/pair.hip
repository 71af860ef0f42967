// Kernels of the pair distributions (psa_pair_histogram, psa_debug_pair_fractions; definition: include/psa_hip.h, host
// side: api_pair.hip): the histogram of the minimum-image distance |mi(r_b(o + tau) - r_a(o))| over the ordered pairs of
// two species and the time origins o -- g(r) at tau = 0, the distinct van Hove function G_d(r,t) at tau > 0.
//
//   pair_frac          positions -> c (frames of a block, 3, n_a) float32, the centred fractional coordinates
//   pair_hist          c of the origin frames and of their partner frames -> per-workgroup 32-bit histograms in LDS -> partials
//   hist_reduce (hist_reduce.hip)  the partials summed in 64-bit integers into the accumulator (n_vh, S, S, n_r + 1)
//
// Arithmetic (the pair chain is min_image.h's min_image and radial_bin, which angle.hip and msd.hip share: this is its one
// statement).  Per (frame, atom), float64 from the float32 position r:
//     sigma_j = fma(r_z, Hinv[2][j], fma(r_y, Hinv[1][j], r_x Hinv[0][j]))
//     c_j     = float32(sigma_j - floor(sigma_j) - 0.5)                          in [-0.5, 0.5]
// (the prepass; a fractional coordinate formed in float32 would carry 2^-24 |sigma|, a bin's width at |r| of 10^3 boxes).
// Per pair, float32, every operation rounded once:
//     e_j = __fsub_rn(c_j(b), c_j(a));   e_j = e_j - rintf(e_j)                  (the second line is exact)
//     d_c = fma(e_2, h[2][c], fma(e_1, h[1][c], e_0 h[0][c]))                    h = H rounded to float32
//     r2  = fma(d_z, d_z, fma(d_y, d_y, d_x d_x));   x = __fmul_rn(__fsqrt_rn(r2), inv_dr)     inv_dr = float32(1 / dr)
//     bin = x < n_r ? (int)floorf(x) : n_r                                       (n_r: the overflow counter)
// Errors: c carries 2^-26 (half an ulp below 0.5), so e carries 2^-24 (two stagings, one subtraction of a value below 1);
// d_c carries sum_j (2^-24 + 3 2^-24 |e_j|) |H_jc| (e's error, and three roundings of values below sum |e_j| |H_jc|);
// x carries (|delta d|_2 + 4.5 2^-24 |d|) / dr: the sum's three roundings halve under the root, the root, inv_dr and the
// product one each.  The rounding e - rint(e) picks the true minimum image of every pair closer than half the smallest
// perpendicular width of the box; the host serves r_max up to (1/2 - 2^-12) of it, so a pair whose fractional difference
// lies within rounding of 1/2 is longer than r_max in either image and is counted in the overflow either way.
//
// Tiling.  A workgroup of PAIR_TILE = 256 lanes takes one item of the host's table: a tile of PAIR_TILE alpha-atoms, one
// per lane with c in registers, a run of beta-tiles and a slab of the block's origins.  Per origin it loads its alpha
// atom at the origin frame, then stages each beta-tile of the partner frame in LDS as three rows (x, y, z) and walks it
// four beta-atoms at a time: every lane reads the same 16 bytes of a row (a broadcast), so the inner loop loads nothing
// from global memory.  Each pair ends in a 32-bit integer add into the workgroup's histogram in LDS (n_r + 1 counters):
// integer adds commute, so the counts are the same bits whatever the order, the blocking and the order of the atoms
// inside a species.  One histogram per workgroup: one per wavefront was measured and was 3-4 % slower (DESIGN section 7
// has both timings).  The host keeps an item's samples below 2^32; the histogram goes to partials with plain
// stores; the reduce kernel sums a species pair's items in uint64.  No global atomics, no float atomics.
//
// tau = 0: every unordered pair is evaluated once.  alpha = beta: the items cover the upper triangle of tiles, the
// diagonal tile counts list position a < b only, and the reduce doubles the sum (each unordered pair is two ordered
// ones); alpha < beta: the items exist for that order alone and the reduce adds the sum to (beta, alpha) as well --
// e and d change sign exactly, r2 is the same bits.  tau > 0: all ordered pairs, the diagonal tile of alpha = beta
// leaves out b = a (the self part).
#include <algorithm>

#include "min_image.h"
#include "psa_ctx.h"

namespace psa {

namespace {

struct PairInv {
    double inv[9];
};

// Grid (atom tiles, frames of the block).  Frame k of the block is f0 + k df.  out[(k 3 + j) n_a + i], i the list position
__global__ void __launch_bounds__(256)
pair_frac_kernel(const float* __restrict__ pos, const int* __restrict__ idx, int n_a, const PairInv box, float* __restrict__ out,
                 int64_t f0, int64_t df, int64_t N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_a) return;
    const int64_t a = idx ? idx[i] : i, f = f0 + (int64_t)blockIdx.y * df;
    const float*  r = pos + (f * N + a) * 3;
    const double  x = (double)r[0], y = (double)r[1], z = (double)r[2];
    for (int j = 0; j < 3; ++j) {
        const double s = __fma_rn(z, box.inv[6 + j], __fma_rn(y, box.inv[3 + j], __dmul_rn(x, box.inv[j])));
        out[((int64_t)blockIdx.y * 3 + j) * n_a + i] = (float)(s - floor(s) - 0.5);
    }
}

// One pair: the bin of |mi(b - a)|
__device__ inline int pair_bin(float ax, float ay, float az, float bx, float by, float bz, const Box32& B, float inv_dr, float edge,
                               int n_r) {
    return radial_bin(min_image(ax, ay, az, bx, by, bz, B).r2, inv_dr, edge, n_r);
}

// Grid (items).  cA, cB: (origins of the block, 3, n_a) float32 at the origin frames and at their partners (tau = 0: the
// same buffer).  part[item][n_r + 1] uint32
__global__ void __launch_bounds__(PAIR_TILE)
pair_hist_kernel(const float* __restrict__ cA, const float* __restrict__ cB, const PairItem* __restrict__ items,
                 unsigned* __restrict__ part, const Box32 B, int n_a, int n_ob, float inv_dr, int n_r) {
    __shared__ unsigned hist[PAIR_MAX_BINS + 1];
    __shared__ __attribute__((aligned(16))) float sb[3][PAIR_TILE];
    const PairItem it = items[blockIdx.x];
    const int      lane = threadIdx.x;
    for (int i = lane; i <= n_r; i += PAIR_TILE) hist[i] = 0u;
    const bool  active = lane < it.a_n;
    const float edge = (float)n_r;
    for (int k = it.slab; k < n_ob; k += it.n_os) {
        const float* a = cA + (int64_t)k * 3 * n_a + it.a_lo + lane;
        const float* b = cB + (int64_t)k * 3 * n_a;
        float        ax = 0.f, ay = 0.f, az = 0.f;
        if (active) ax = a[0], ay = a[n_a], az = a[2 * (int64_t)n_a];
        for (int bt = it.b_lo; bt < it.b_hi; bt += PAIR_TILE) {
            const int nb = min(PAIR_TILE, it.b_hi - bt);
            __syncthreads();                                               // the last tile's reads (and the zeroing) have ended
            for (int c = 0; c < 3; ++c) sb[c][lane] = lane < nb ? b[(int64_t)c * n_a + bt + lane] : 0.f;
            __syncthreads();
            if (!active) continue;
            const int mode = bt == it.a_lo ? it.diag : 0;                  // the diagonal tile of alpha = beta
            if (mode) {
                for (int i = 0; i < nb; ++i) {
                    if (mode == 1 ? lane >= i : lane == i) continue;       // 1: list position a < b only; 2: b != a
                    atomicAdd(&hist[pair_bin(ax, ay, az, sb[0][i], sb[1][i], sb[2][i], B, inv_dr, edge, n_r)], 1u);
                }
                continue;
            }
            int i = 0;
            for (; i + 4 <= nb; i += 4) {                                  // the inner loop: four beta-atoms per row read
                const float4 bx = *reinterpret_cast<const float4*>(&sb[0][i]);
                const float4 by = *reinterpret_cast<const float4*>(&sb[1][i]);
                const float4 bz = *reinterpret_cast<const float4*>(&sb[2][i]);
                atomicAdd(&hist[pair_bin(ax, ay, az, bx.x, by.x, bz.x, B, inv_dr, edge, n_r)], 1u);
                atomicAdd(&hist[pair_bin(ax, ay, az, bx.y, by.y, bz.y, B, inv_dr, edge, n_r)], 1u);
                atomicAdd(&hist[pair_bin(ax, ay, az, bx.z, by.z, bz.z, B, inv_dr, edge, n_r)], 1u);
                atomicAdd(&hist[pair_bin(ax, ay, az, bx.w, by.w, bz.w, B, inv_dr, edge, n_r)], 1u);
            }
            for (; i < nb; ++i) atomicAdd(&hist[pair_bin(ax, ay, az, sb[0][i], sb[1][i], sb[2][i], B, inv_dr, edge, n_r)], 1u);
        }
    }
    __syncthreads();
    unsigned* dst = part + (int64_t)blockIdx.x * (n_r + 1);
    for (int i = lane; i <= n_r; i += PAIR_TILE) dst[i] = hist[i];
}

}  // namespace

int launch_pair_frac(psa_ctx* c, const float* d_pos, const int* d_idx, int64_t n_a, const double* box_inverse, float* d_out, int64_t f0,
                     int64_t df, int64_t n_frames, int64_t T, int64_t N) {
    if (n_a == 0 || n_frames == 0) return PSA_OK;
    PSA_REQUIRE(n_a < (1ll << 31) && N < (1ll << 31) && n_frames >= 1 && n_frames <= 65535 && f0 >= 0 && df >= 0 &&
                    f0 + (n_frames - 1) * df <= T - 1,
                "fraction pass outside its grid");
    PairInv b;
    for (int i = 0; i < 9; ++i) b.inv[i] = box_inverse[i];
    hipLaunchKernelGGL(pair_frac_kernel, dim3((unsigned)((n_a + 255) / 256), (unsigned)n_frames), dim3(256), 0, c->stream, d_pos, d_idx,
                       (int)n_a, b, d_out, f0, df, N);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_pair_hist(psa_ctx* c, const float* d_cA, const float* d_cB, const void* d_items, int64_t n_items, unsigned* d_part,
                     const double* box, int64_t n_a, int64_t n_ob, float inv_dr, int32_t n_r) {
    if (n_items == 0) return PSA_OK;
    PSA_REQUIRE(n_items < (1ll << 31) && n_a < (1ll << 31) && n_ob >= 1 && n_ob < (1ll << 31) && n_r >= 1 && n_r <= PAIR_MAX_BINS,
                "pair pass outside its grid");
    hipLaunchKernelGGL(pair_hist_kernel, dim3((unsigned)n_items), dim3(PAIR_TILE), 0, c->stream, d_cA, d_cB,
                       static_cast<const PairItem*>(d_items), d_part, Box32(box), (int)n_a, (int)n_ob, inv_dr, (int)n_r);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
