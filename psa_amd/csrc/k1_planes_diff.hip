// K1 low-rank route for k-paths (planned on the host in api_lowrank.hip): the device half.
//
// A k-path lies on one line, k_j = k0 + kappa_j u, so its phase matrix is, to fp64 rounding, 64 node rows
// combined per k-vector: exp(i k_j.r) = sum_l C[j,l] W[l,.] (Chebyshev interpolation in kappa).  The reference
// rounds the phase argument in float32, which the node rows do not; the difference D = P_ref - P_line is
// small (|D| <= 2^-13, checked by the plan) and goes through ONE float16 product with the hi plane.  So
//     q = C (W v) + D v_hi
// = a 128-row "2 x f16" launch of the existing planes kernel (node_table_kernel -> k1_planes_lw.hip), the D pass
// below (one MFMA per row tile and component instead of three, hi plane only), and the combine (lowrank_combine.hip).
//
// D pass: 512-ROW x 64-frame workgroup tile.  Eight wavefronts, two per SIMD; wavefront w = 4 h + f owns rows
// [256 h, +256) x frames [16 f, +16) x 3 components = 48 accumulator tiles (192 registers), the stage's three B
// fragments (12) and a four-deep ring of A fragments read two row tiles ahead (16).  No float32 fold sums: the D
// part is ~1e-5 of the signal, so the float16-MFMA chain's truncation over all stages (<= n_stage * 2^-24 of it)
// stays far below float32 rounding of the total.
// A stage is 44 one-KiB units: 12 plane units (unit 4 c + j = hi piece of component c, frame group j) and 32 D
// units (unit 12 + 2 mt + h = row tile mt of row half h).  The units live in a ring of 160 units of LDS: stage s,
// unit u at (44 s + u) mod 160; positions repeat every 40 stages, so the main loop is unrolled 40 times and every
// LDS address is a constant.  Entering stage s (stage s-1's units are free) waves 0-3 issue the units 28..43 of
// stage s+2 and 0..27 of stage s+3 (the 160 - 3 x 44 = 28 spare units) -- eleven LDS-DMA instructions each,
// their SIMD partners none (the issuing wavefront is held per instruction, its partner multiplies meanwhile:
// the scheme of k1_planes_wide.hip).  The barrier that ends stage s is preceded by vmcnt(7): all of stages s+1
// and s+2 have landed, so a stage reads the next one's fragments while it multiplies.
// Per stage and CU: 44 KiB of LDS-DMA (11 per 128 rows; the 256-row kernel needs 28), 384 MFMAs.
#include <utility>

#include "k1_f16.h"
#include "k1_lowrank_fold.h"
#include "k1_lowrank_n48.h"
#include "k1_lowrank_pair.h"

namespace psa {

namespace {
constexpr int D_M_BLK = 512, D_T_BLK = 64, D_MT = 16, D_PERIOD = 40;
constexpr int D_STAGE_UNITS = 44, D_RING_UNITS = 160, D_EARLY = D_RING_UNITS - 3 * D_STAGE_UNITS;   // 28
constexpr int D_STAGE_BYTES = D_M_BLK * K1_BA * 2;                                               // 32 KiB of D per stage
static_assert(D_EARLY == 28 && D_RING_UNITS % 4 == 0 && D_STAGE_UNITS % 4 == 0, "ring arithmetic");
constexpr auto d_unit_off = unit_off<D_STAGE_UNITS, D_RING_UNITS, D_PERIOD>;
}  // namespace

// element (row m, atom a) of the D image: [M block of 512][atom stage][unit 2 mt + h][16 rows][32 atoms] (float16), the
// 16-byte slots of a row swizzled as in the phase-table image (pf16_tile_index)
__host__ __device__ inline size_t pd16_index(int m, int a, int n_stage) {
    const int row = m % D_M_BLK, rt = row >> 4, v = 2 * (rt & 15) + (rt >> 4), r = row & 15, al = a % K1_BA;
    return (((size_t)(m / D_M_BLK) * n_stage + a / K1_BA) * 32 + v) * (16 * K1_BA) + (size_t)r * K1_BA +
           (size_t)((((al >> 3) ^ pl_swizzle(r)) << 3) + (al & 7));
}
// (+ 4 stages of padding: the D pass fetches up to three stages past an M block's end and never reads them)
size_t pd16_table_bytes(int M_pad, int A_pad) { return ((size_t)M_pad * A_pad + 4 * (size_t)D_M_BLK * K1_BA) * 2; }

template <bool NT_V>
__global__ void __launch_bounds__(512, 2)
k1_planes_diff_kernel(const _Float16* __restrict__ planes, const _Float16* __restrict__ Db, float2* __restrict__ Q, int64_t T,
                      int64_t q_stride, int n_fg, int n_stage, int K, int n_mblk, int n_tblk, float qscale) {
    using PR = F16x2;
    using E8 = PR::v8;
    __shared__ __attribute__((aligned(16))) unsigned char smem[D_RING_UNITS * 1024];
    const unsigned lds0 = (unsigned)(size_t)(lds_u8*)smem;

    int mb, tb;                                        // M block, 64-frame tile (k1_block_map: XCD-aware)
    if (!k1_block_map(n_mblk, n_tblk, mb, tb)) return;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wh = w >> 2, wf = w & 3;
    const int r16 = lane & 15, q = lane >> 4;

    // ---- waves 0-3: eleven source streams, instruction i = unit w + 4 i of every stage ----------------------
    // i = 0..2: hi piece of component i of frame group w; i = 3..10: D unit w + 4 (i - 3)
    const unsigned char* src[11];
    {
        int fg = tb * 4 + (w & 3);                                      // frame group (past the end: the last one, never stored)
        if (fg >= n_fg) fg = n_fg - 1;
        const unsigned char* pl0 = reinterpret_cast<const unsigned char*>(planes) + (size_t)fg * n_stage * PL_STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < 3; ++i) src[i] = pl0 + 1024 * (2 * i);      // (component i, piece 0) = block 2 i of the 6
        const unsigned char* d0 = reinterpret_cast<const unsigned char*>(Db) + (size_t)mb * n_stage * D_STAGE_BYTES;
#pragma unroll
        for (int i = 3; i < 11; ++i) src[i] = d0 + 1024 * ((w & 3) + 4 * (i - 3));
    }
    const unsigned dma_voff = 16 * lane;
    const unsigned wbase = lds0 + 1024 * (w & 3);                       // unit 4 i + w: 1024 w past unit 4 i (no wrap: 44 s + 4 i is a multiple of 4)
    using std::integral_constant;
    auto dma = [&](auto s40_c, auto i_c) __attribute__((always_inline)) {
        constexpr int      S40 = decltype(s40_c)::value, I = decltype(i_c)::value;
        constexpr unsigned OFF = d_unit_off(S40, 4 * I);
        if constexpr (I < 3) {
            lds_dma16_at<OFF, NT_V>(src[I], dma_voff, wbase);
            src[I] += PL_STAGE_BYTES;
        } else {
            lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);
            src[I] += D_STAGE_BYTES;
        }
    };
    auto dma_range = [&]<int S40, int... Is>(integral_constant<int, S40>, std::integer_sequence<int, Is...>) __attribute__((always_inline)) {
        (dma(integral_constant<int, S40>{}, integral_constant<int, Is>{}), ...);
    };
    // units 0..27 of a stage are instructions 0..6, units 28..43 instructions 7..10
    auto dma_late = [&](auto s40_c) __attribute__((always_inline)) {
        dma_range(s40_c, std::integer_sequence<int, 7, 8, 9, 10>{});
    };
    auto dma_early = [&](auto s40_c) __attribute__((always_inline)) {
        dma_range(s40_c, std::make_integer_sequence<int, 7>{});
    };

    // ---- fragment reads: every unit is 16 rows (frames) x 64 bytes, lane (r16, q) takes 16 bytes ----------
    const unsigned lane_off = lds0 + r16 * (K1_BA * 2) + ((q ^ pl_swizzle(r16)) << 4);
    unsigned       lane_a[3], lane_b[3];
    // D unit 12 + 2 mt + h: 1024 h past unit 12 + 2 mt (even); plane unit 4 c + f
    unit_ring_windows(lane_off + 1024 * wh, lane_off + 1024 * wf, lane_a, lane_b);
    E8    a[4];                                    // A fragments of row tiles mt .. mt+3 (mod 4), read two ahead
    E8    bf[3];                                   // hi B fragments of the stage in work
    f32x4 acc[D_MT][3];
    auto  read_a = [&](auto s40_c, auto mt_c) __attribute__((always_inline)) {
        constexpr int S40 = decltype(s40_c)::value, MTI = decltype(mt_c)::value;
        a[MTI & 3] = lds_frag(lane_a, d_unit_off(S40, 12 + 2 * MTI));
    };
    auto read_b = [&](auto s40_c, auto c_c) __attribute__((always_inline)) {
        constexpr int S40 = decltype(s40_c)::value, CC = decltype(c_c)::value;
        bf[CC] = lds_frag(lane_b, d_unit_off(S40, 4 * CC));
    };
    // (zeroed in place: through a shared helper the compiler orders this kernel's instructions differently)
#pragma unroll
    for (int mt = 0; mt < D_MT; ++mt)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- prologue: stages 0 and 1 whole, units 0..27 of stage 2 ------------------------------------------
    using I0 = integral_constant<int, 0>;
    using I1 = integral_constant<int, 1>;
    using I2 = integral_constant<int, 2>;
    if (wh == 0) {
        dma_early(I0{});
        dma_late(I0{});
        dma_early(I1{});
        dma_late(I1{});
        dma_early(I2{});
    }
    asm volatile("s_waitcnt vmcnt(7)\n\ts_barrier" ::: "memory");      // stages 0 and 1 landed
    read_b(I0{}, I0{});
    read_b(I0{}, I1{});
    read_b(I0{}, I2{});
    read_a(I0{}, I0{});
    read_a(I0{}, I1{});

    int  left = n_stage;                                               // stages to go when the period began
    auto stage = [&](auto s40_c) __attribute__((always_inline)) {
        constexpr int S40 = decltype(s40_c)::value;
        if (left <= S40) return;                                       // past the group's last stage
        using SN = integral_constant<int, (S40 + 1) % D_PERIOD>;
        using SNN = integral_constant<int, (S40 + 2) % D_PERIOD>;
        using S3 = integral_constant<int, (S40 + 3) % D_PERIOD>;
        if (wh == 0) {                                                 // stage s-1's units are free
            dma_late(SNN{});
            dma_early(S3{});
        }
        auto tile = [&](auto mt_c) __attribute__((always_inline)) {
            constexpr int MTI = decltype(mt_c)::value;
            if constexpr (MTI + 2 < D_MT)
                read_a(s40_c, integral_constant<int, MTI + 2>{});
            else
                read_a(SN{}, integral_constant<int, MTI + 2 - D_MT>{});
            auto comp = [&](auto c_c) __attribute__((always_inline)) {
                constexpr int CC = decltype(c_c)::value;
                acc[MTI][CC] = PR::mma(a[MTI & 3], bf[CC], acc[MTI][CC]);
                if constexpr (MTI == D_MT - 1) read_b(SN{}, c_c);      // behind the component's last use in this stage
            };
            comp(I0{});
            comp(I1{});
            comp(I2{});
            __builtin_amdgcn_sched_barrier(0);
        };
        [&]<int... Ms>(std::integer_sequence<int, Ms...>) __attribute__((always_inline)) { (tile(integral_constant<int, Ms>{}), ...); }(
            std::make_integer_sequence<int, D_MT>{});
        // what this stage read from its own units has been consumed above; reads in flight come from stage s+1
        asm volatile("s_waitcnt vmcnt(7)\n\ts_barrier" ::: "memory");     // stages s+1 and s+2 landed
    };
    for (; left > 0; left -= D_PERIOD)
        [&]<int... Ss>(std::integer_sequence<int, Ss...>) __attribute__((always_inline)) { (stage(integral_constant<int, Ss>{}), ...); }(
            std::make_integer_sequence<int, D_PERIOD>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // nothing in flight when LDS is handed on

    // ---- epilogue: the lane's coordinates are taken afresh (not carried through the loop: k1_planes_wide.hip)
    const int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int r16_e = lane_e & 15, q_e = lane_e >> 4;
    k1_store_q(Q, acc, wh * (D_M_BLK / 2) + mb * D_M_BLK, q_e, (int64_t)tb * D_T_BLK + wf * 16 + r16_e, T, K, q_stride, qscale);
}

// d_planes: the group's planes from its first frame group on; d_diff: the D image (pd16_index), g.M_pad rows; dscale: the
// power of two the image was multiplied by
int launch_k1_planes_diff(psa_ctx* c, const void* d_planes, const void* d_diff, float2* d_q, const ProjGeom& g, int64_t n_fg, float dscale) {
    PSA_REQUIRE(g.M_pad % D_M_BLK == 0 && g.M_pad >= 2 * g.K && g.M_pad > 0, "D pass: 512-row M blocks only");
    PSA_REQUIRE(dscale > 0.f, "planes do not cover the launch");
    return launch_planes_family(c, k1_planes_diff_kernel<true>, k1_planes_diff_kernel<false>, D_M_BLK, 512, "D pass", K1_BA, dscale,
                                d_planes, d_diff, d_q, g, n_fg);
}

// ---------------------------------------------------------------------------------------------
// Tables
// ---------------------------------------------------------------------------------------------
// The parts of D[k, a] for group atom a: cs = P_ref (cos, sin), ce / se = P_line in fp64, wa = the atom's weight (1 without)
__device__ __forceinline__ void diff_parts(const float* __restrict__ kvec, const double* __restrict__ kline,
                                           const float* __restrict__ mean_all, const int* __restrict__ idx,
                                           const float* __restrict__ w, float wnorm, int k, int a, float (&cs)[2], double& ce,
                                           double& se, double& wa) {
    const int   src = idx ? idx[a] : a;
    const float rx = mean_all[3 * (size_t)src + 0], ry = mean_all[3 * (size_t)src + 1], rz = mean_all[3 * (size_t)src + 2];
    const float kx = kvec[3 * k + 0], ky = kvec[3 * k + 1], kz = kvec[3 * k + 2];
    const float arg = __fmaf_rn(kz, rz, __fmaf_rn(ky, ry, __fmul_rn(kx, rx)));
    sincosf(arg, &cs[1], &cs[0]);
    const double th = kline[3 * k + 0] * (double)rx + kline[3 * k + 1] * (double)ry + kline[3 * k + 2] * (double)rz;
    sincos(th, &se, &ce);
    wa = w ? (double)(w[src] * wnorm) : 1.0;
}

// D[j, a] = (P_ref - P_line) * dscale, one float16 piece.  P_ref exactly as phase_table_f16_kernel (k1_pair.hip)
// computes it -- the same float32 FMA chain and sincosf, under the same compiler flags --, P_line from the k-vector
// projected on the plan's line, kline[3 j..], in fp64.  Rows past 2K and atoms past n_g are zero.
// Per-atom weights w (may be null): the route is linear per atom column, so D and the node rows both carry the same
// w * wnorm (phase_table_f16_kernel, k1_pair.hip): |w wnorm| <= 1 keeps |D| under the plan's bound and dscale valid.
// PAIR: the image of the pair launch (pd16_pair_index, k1_lowrank_pair.h; one 512-row block) instead of the D pass's.
template <bool PAIR>
__global__ void __launch_bounds__(256)
diff_table_kernel(const float* __restrict__ kvec, const double* __restrict__ kline, const float* __restrict__ mean_all,
                  const int* __restrict__ idx, const float* __restrict__ w, float wnorm, _Float16* __restrict__ Db, int K,
                  int n_g, int A_pad, float dscale) {
    const int a = blockIdx.y * 256 + threadIdx.x;
    const int k = blockIdx.x;
    if (a >= A_pad) return;
    float d[2] = {0.f, 0.f};
    if (k < K && a < n_g) {      // (diff_parts, written out: through the helper the compiler orders this kernel's instructions differently)
        const int   src = idx ? idx[a] : a;
        const float rx = mean_all[3 * (size_t)src + 0], ry = mean_all[3 * (size_t)src + 1], rz = mean_all[3 * (size_t)src + 2];
        const float kx = kvec[3 * k + 0], ky = kvec[3 * k + 1], kz = kvec[3 * k + 2];
        const float arg = __fmaf_rn(kz, rz, __fmaf_rn(ky, ry, __fmul_rn(kx, rx)));
        float       cs[2];
        sincosf(arg, &cs[1], &cs[0]);
        const double th = kline[3 * k + 0] * (double)rx + kline[3 * k + 1] * (double)ry + kline[3 * k + 2] * (double)rz;
        double       se, ce;
        sincos(th, &se, &ce);
        const double wa = w ? (double)(w[src] * wnorm) : 1.0;
        d[0] = (float)(((double)cs[0] - ce) * (double)dscale * wa);
        d[1] = (float)(((double)cs[1] - se) * (double)dscale * wa);
    }
    const int n_stage = A_pad / K1_BA;
    Db[PAIR ? pd16_pair_index(2 * k, a, n_stage) : pd16_index(2 * k, a, n_stage)] = (_Float16)d[0];
    Db[PAIR ? pd16_pair_index(2 * k + 1, a, n_stage) : pd16_index(2 * k + 1, a, n_stage)] = (_Float16)d[1];
}

// Node rows W[l, a] = exp(i k0.r_a) exp(i kappa_l (u.r_a - x_c)), fp64 argument and sincos, in the two-piece phase-table
// image of one 128-row M block (pf16_tile_index): what k1_planes_lw.hip projects as 64 k-vectors.
// geo = {k0 (3), u (3), x_c}; kappa: the 64 nodes
__global__ void __launch_bounds__(256)
node_table_kernel(const double* __restrict__ geo, const double* __restrict__ kappa, const float* __restrict__ mean_all,
                  const int* __restrict__ idx, const float* __restrict__ w, float wnorm, _Float16* __restrict__ Pb, int n_g,
                  int A_pad) {
    const int a = blockIdx.y * 256 + threadIdx.x;
    const int l = blockIdx.x;
    if (a >= A_pad) return;
    double cs[2] = {0.0, 0.0};
    if (a < n_g) {
        const int    src = idx ? idx[a] : a;
        const double rx = mean_all[3 * (size_t)src + 0], ry = mean_all[3 * (size_t)src + 1], rz = mean_all[3 * (size_t)src + 2];
        const double th = (geo[0] * rx + geo[1] * ry + geo[2] * rz) + kappa[l] * ((geo[3] * rx + geo[4] * ry + geo[5] * rz) - geo[6]);
        sincos(th, &cs[1], &cs[0]);
        if (w) {
            const double wa = (double)(w[src] * wnorm);
            cs[0] *= wa;
            cs[1] *= wa;
        }
    }
    const int n_stage = A_pad / K1_BA;
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
        const double   x = cs[ri] * (double)F16x2::P_SCALE;
        const _Float16 lead = (_Float16)(float)x;
        Pb[pf16_tile_index(0, 2 * l + ri, a, 128, n_stage)] = lead;
        Pb[pf16_tile_index(1, 2 * l + ri, a, 128, n_stage)] = (_Float16)(float)(x - (double)lead);
    }
}

// The FOLDED D image (psa_set_k1_lowrank_fold): D'[j, a] = (D[j, a] + E[j, a]) dscale, rounded once to float32 and then to
// one float16 piece like D.  D as above, in fp64.  E[j, a] = phi_j sum_l L[j, l] W_lo[l, a] / 2^14 is what the combine
// makes of the node rows' product W_lo v_hi, which the folded node rows leave out (k1_lowrank_fold.hip): W_lo are the
// float16 lo pieces AS THEY STAND in the node table image Pn (node_table_kernel, which therefore runs first; they carry
// the weights already), L and phi the plan's float32 tables that the combine reads.  One fixed order per element: float32
// FMAs over l = 0..63, real and imaginary sums on their own, then phase_add's two operations per part
// (lowrank_combine.hip) -- a row's bits depend on k_j, the node interval and the group alone, however rows and atoms are
// tiled.  |E| <= rot_j Lam_j 2^-12 (the plan's e_bound), so dscale is the plan's dscale_fold.
// A thread holds one atom's 128 lo pieces and walks FOLD_JB rows; L and phi are uniform reads.  (32 rows per thread, and the
// two sums as one packed FMA, measured no faster: 0.12 and 0.11 ms against 0.11 at configuration 3.)
// FOLD: the folded pair launch's image (pd16_fold_index, k1_lowrank_fold.h) instead of the D pass's.
constexpr int FOLD_JB = 16;
template <bool FOLD>
__global__ void __launch_bounds__(256)
diff_fold_table_kernel(const float* __restrict__ kvec, const double* __restrict__ kline, const float* __restrict__ mean_all,
                       const int* __restrict__ idx, const float* __restrict__ w, float wnorm, const _Float16* __restrict__ Pn,
                       const float* __restrict__ L, const float2* __restrict__ phi, _Float16* __restrict__ Db, int K, int n_g,
                       int A_pad, float dscale) {
    const int a = blockIdx.y * 256 + threadIdx.x;
    const int k0 = blockIdx.x * FOLD_JB;
    if (a >= A_pad) return;
    const int n_stage = A_pad / K1_BA;
    _Float16  wl[2 * LOWRANK_NODES];
#pragma unroll
    for (int m = 0; m < 2 * LOWRANK_NODES; ++m) wl[m] = Pn[pf16_tile_index(1, m, a, 2 * LOWRANK_NODES, n_stage)];
    for (int k = k0; k < k0 + FOLD_JB; ++k) {
        float d[2] = {0.f, 0.f};
        if (k < K && a < n_g) {
            const float* Lk = L + (size_t)k * LOWRANK_NODES;
            float        sr = 0.f, si = 0.f;
#pragma unroll
            for (int l = 0; l < LOWRANK_NODES; ++l) {
                sr = __fmaf_rn(Lk[l], (float)wl[2 * l], sr);
                si = __fmaf_rn(Lk[l], (float)wl[2 * l + 1], si);
            }
            const float2 ph = phi[k];
            const float  er = __fmaf_rn(-ph.y, si, __fmul_rn(ph.x, sr)), ei = __fmaf_rn(ph.y, sr, __fmul_rn(ph.x, si));
            float        cs[2];
            double       se, ce, wa;
            diff_parts(kvec, kline, mean_all, idx, w, wnorm, k, a, cs, ce, se, wa);
            constexpr double inv_p = 1.0 / (double)F16x2::P_SCALE;
            d[0] = (float)((((double)cs[0] - ce) * wa + (double)er * inv_p) * (double)dscale);
            d[1] = (float)((((double)cs[1] - se) * wa + (double)ei * inv_p) * (double)dscale);
        }
        Db[FOLD ? pd16_fold_index(2 * k, a, n_stage) : pd16_index(2 * k, a, n_stage)] = (_Float16)d[0];
        Db[FOLD ? pd16_fold_index(2 * k + 1, a, n_stage) : pd16_index(2 * k + 1, a, n_stage)] = (_Float16)d[1];
    }
}

// the same tables for the folded route: the node table first, then the folded D image from it (d_L, d_phi: the plan's)
int launch_lowrank_tables_fold(psa_ctx* c, const float* d_kvec, const double* d_kline, const double* d_geo, const double* d_kappa,
                               const float* d_mean_all, const int* d_idx, const float* d_L, const float2* d_phi, void* d_diff,
                               void* d_nodes, const ProjGeom& g, int M_pad_d, float dscale, bool pair) {
    PSA_REQUIRE(M_pad_d % D_M_BLK == 0 && M_pad_d >= 2 * g.K && g.A_pad % K1_BA == 0, "bad low-rank table geometry");
    PSA_REQUIRE(!pair || M_pad_d == LRF_ROWS, "the folded pair launch's image is one 512-row block");
    static_assert((D_M_BLK / 2) % FOLD_JB == 0, "whole blocks of rows");
    hipLaunchKernelGGL(node_table_kernel, dim3(LOWRANK_NODES, (g.A_pad + 255) / 256), dim3(256), 0, c->stream, d_geo, d_kappa, d_mean_all,
                       d_idx, g.weights, 1.f / g.wscale, (_Float16*)d_nodes, g.n_g, g.A_pad);
    PSA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pair ? diff_fold_table_kernel<true> : diff_fold_table_kernel<false>,
                       dim3(M_pad_d / 2 / FOLD_JB, (g.A_pad + 255) / 256), dim3(256), 0, c->stream, d_kvec, d_kline, d_mean_all, d_idx,
                       g.weights, 1.f / g.wscale, (const _Float16*)d_nodes, d_L, d_phi, (_Float16*)d_diff, g.K, g.n_g, g.A_pad, dscale);
    PSA_HIP_CHECK(hipGetLastError());
    if (pair) {      // each role's part ends with its own padding stages
        const size_t n_stage = (size_t)g.A_pad / K1_BA, a_pad = LRF_PAD_STAGES * LRF_A_UNITS * 1024, b_pad = LRF_PAD_STAGES * LRF_B_UNITS * 1024;
        static_assert(LRF_ROWS == D_M_BLK, "the fold image has the size of one D block");
        PSA_HIP_CHECK(hipMemsetAsync((char*)d_diff + n_stage * LRF_A_UNITS * 1024, 0, a_pad, c->stream));
        PSA_HIP_CHECK(hipMemsetAsync((char*)d_diff + pd16_fold_table_bytes((int)n_stage) - b_pad, 0, b_pad, c->stream));
    } else {
        PSA_HIP_CHECK(hipMemsetAsync((char*)d_diff + (size_t)M_pad_d * g.A_pad * 2, 0,
                                     pd16_table_bytes(M_pad_d, g.A_pad) - (size_t)M_pad_d * g.A_pad * 2, c->stream));
    }
    return PSA_OK;
}

int launch_lowrank_tables(psa_ctx* c, const float* d_kvec, const double* d_kline, const double* d_geo, const double* d_kappa,
                          const float* d_mean_all, const int* d_idx, void* d_diff, void* d_nodes, const ProjGeom& g, int M_pad_d,
                          float dscale, bool pair) {
    PSA_REQUIRE(M_pad_d % D_M_BLK == 0 && M_pad_d >= 2 * g.K && g.A_pad % K1_BA == 0, "bad low-rank table geometry");
    PSA_REQUIRE(!pair || M_pad_d == LRP_ROWS, "the pair launch's image is one 512-row block");
    hipLaunchKernelGGL(pair ? diff_table_kernel<true> : diff_table_kernel<false>, dim3(M_pad_d / 2, (g.A_pad + 255) / 256), dim3(256), 0,
                       c->stream, d_kvec, d_kline, d_mean_all, d_idx, g.weights, 1.f / g.wscale, (_Float16*)d_diff, g.K, g.n_g, g.A_pad,
                       dscale);
    PSA_HIP_CHECK(hipGetLastError());
    if (pair) {      // each role's part ends with its own padding stages
        const size_t n_stage = (size_t)g.A_pad / K1_BA, a_pad = LRP_PAD_STAGES * LRP_A_UNITS * 1024, b_pad = LRP_PAD_STAGES * LRP_B_UNITS * 1024;
        static_assert(LRP_ROWS == D_M_BLK, "the pair image has the size of one D block");
        PSA_HIP_CHECK(hipMemsetAsync((char*)d_diff + n_stage * LRP_A_UNITS * 1024, 0, a_pad, c->stream));
        PSA_HIP_CHECK(hipMemsetAsync((char*)d_diff + pd16_pair_table_bytes((int)n_stage) - b_pad, 0, b_pad, c->stream));
    } else {
        PSA_HIP_CHECK(hipMemsetAsync((char*)d_diff + (size_t)M_pad_d * g.A_pad * 2, 0,
                                     pd16_table_bytes(M_pad_d, g.A_pad) - (size_t)M_pad_d * g.A_pad * 2, c->stream));
    }
    hipLaunchKernelGGL(node_table_kernel, dim3(LOWRANK_NODES, (g.A_pad + 255) / 256), dim3(256), 0, c->stream, d_geo, d_kappa, d_mean_all,
                       d_idx, g.weights, 1.f / g.wscale, (_Float16*)d_nodes, g.n_g, g.A_pad);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

// ---------------------------------------------------------------------------------------------
// Tables of the 48-node route (psa_set_k1_lowrank_nodes, k1_lowrank_n48.hip)
// ---------------------------------------------------------------------------------------------
// node_table_kernel for 48 nodes in the same 128-row block: rows 2 l, 2 l + 1 of node l < 48 with node_table_kernel's
// arithmetic, rows 96..127 zero in both pieces (the two-product node pass multiplies them and stores nothing of them)
__global__ void __launch_bounds__(256)
node_table_n48_kernel(const double* __restrict__ geo, const double* __restrict__ kappa, const float* __restrict__ mean_all,
                      const int* __restrict__ idx, const float* __restrict__ w, float wnorm, _Float16* __restrict__ Pb, int n_g,
                      int A_pad) {
    const int a = blockIdx.y * 256 + threadIdx.x;
    const int l = blockIdx.x;
    if (a >= A_pad) return;
    double cs[2] = {0.0, 0.0};
    if (a < n_g && l < LOWRANK_NODES_48) {
        const int    src = idx ? idx[a] : a;
        const double rx = mean_all[3 * (size_t)src + 0], ry = mean_all[3 * (size_t)src + 1], rz = mean_all[3 * (size_t)src + 2];
        const double th = (geo[0] * rx + geo[1] * ry + geo[2] * rz) + kappa[l] * ((geo[3] * rx + geo[4] * ry + geo[5] * rz) - geo[6]);
        sincos(th, &cs[1], &cs[0]);
        if (w) {
            const double wa = (double)(w[src] * wnorm);
            cs[0] *= wa;
            cs[1] *= wa;
        }
    }
    const int n_stage = A_pad / K1_BA;
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
        const double   x = cs[ri] * (double)F16x2::P_SCALE;
        const _Float16 lead = (_Float16)(float)x;
        Pb[pf16_tile_index(0, 2 * l + ri, a, 128, n_stage)] = lead;
        Pb[pf16_tile_index(1, 2 * l + ri, a, 128, n_stage)] = (_Float16)(float)(x - (double)lead);
    }
}

// fp64 to float16 with ONE rounding: to float32 rounded to odd (an inexact result takes the neighbour whose last bit is
// set), which float16's rounding to nearest even then sees as it would see x itself (24 bits >= 11 + 2)
__device__ __forceinline__ _Float16 f64_to_f16(double x) {
    float        f = (float)x;
    const double e = x - (double)f;                                       // exact
    if (e != 0.0 && f != 0.f) {
        unsigned b = __float_as_uint(f);
        if (!(b & 1u)) {
            const bool grow = (e > 0.0) == !(b >> 31);                    // x lies past f in magnitude
            f = __uint_as_float(grow ? b + 1u : b - 1u);
        }
    }
    return (_Float16)f;
}

// The D image of the 48-node route: what the node rows' hi piece does not carry,
//     D'[j, a] = (P_ref[j, a] w_a - phi_j sum_l L[j, l] W_hi[l, a] / 2^14) dscale,
// taken in fp64 and rounded ONCE to float16.  P_ref and w_a as in diff_table_kernel; W_hi the float16 hi pieces AS THEY
// STAND in the node table image Pn (node_table_n48_kernel, which therefore runs first; they carry the weights), exact in
// fp64; L and phi the plan's float32 tables that the combine reads.  The one expression holds D = (P_ref - P_line) w,
// E = phi L W_lo, the residual of 48-node interpolation (<= 4.6e-7) and the float32 rounding of phi and L on the v_hi
// term.  One fixed order per element: fp64 FMAs over l = 0..47 from zero, real and imaginary sums on their own, then
// phi_r s_r, fma(-phi_i, s_i, .) and phi_r s_i, fma(phi_i, s_r, .) -- a row's bits depend on k_j, the node interval and
// the group alone, however rows and atoms are tiled.  |D'| <= d_bound + e_bound + r_bound: dscale is the 48-node plan's
// dscale_fold.  A thread holds one atom's 96 hi pieces as doubles and walks FOLD_JB rows; L and phi are uniform reads.
// N48: the 48-node pair launch's image (pd16_n48_index, k1_lowrank_n48.h) instead of the D pass's.
template <bool N48>
__global__ void __launch_bounds__(256)
diff_n48_table_kernel(const float* __restrict__ kvec, const float* __restrict__ mean_all, const int* __restrict__ idx,
                      const float* __restrict__ w, float wnorm, const _Float16* __restrict__ Pn, const float* __restrict__ L,
                      const float2* __restrict__ phi, _Float16* __restrict__ Db, int K, int n_g, int A_pad, float dscale) {
    constexpr int NN = LOWRANK_NODES_48;
    const int     a = blockIdx.y * 256 + threadIdx.x;
    const int     k0 = blockIdx.x * FOLD_JB;
    if (a >= A_pad) return;
    const int n_stage = A_pad / K1_BA;
    double    wh[2 * NN];
#pragma unroll
    for (int m = 0; m < 2 * NN; ++m) wh[m] = (double)(float)Pn[pf16_tile_index(0, m, a, 128, n_stage)];
    float  rx = 0.f, ry = 0.f, rz = 0.f;
    double wa = 0.0;
    if (a < n_g) {
        const int src = idx ? idx[a] : a;
        rx = mean_all[3 * (size_t)src + 0], ry = mean_all[3 * (size_t)src + 1], rz = mean_all[3 * (size_t)src + 2];
        wa = w ? (double)(w[src] * wnorm) : 1.0;
    }
    for (int k = k0; k < k0 + FOLD_JB; ++k) {
        double d[2] = {0.0, 0.0};
        if (k < K && a < n_g) {
            const float* Lk = L + (size_t)k * NN;
            double       sr = 0.0, si = 0.0;
#pragma unroll
            for (int l = 0; l < NN; ++l) {
                const double ll = (double)Lk[l];
                sr = fma(ll, wh[2 * l], sr);
                si = fma(ll, wh[2 * l + 1], si);
            }
            const float2 ph = phi[k];
            const double pr = (double)ph.x, pi = (double)ph.y;
            const double er = fma(-pi, si, pr * sr), ei = fma(pi, sr, pr * si);
            const float  kx = kvec[3 * k + 0], ky = kvec[3 * k + 1], kz = kvec[3 * k + 2];
            const float  arg = __fmaf_rn(kz, rz, __fmaf_rn(ky, ry, __fmul_rn(kx, rx)));
            float        cs[2];
            sincosf(arg, &cs[1], &cs[0]);
            constexpr double inv_p = 1.0 / (double)F16x2::P_SCALE;
            d[0] = ((double)cs[0] * wa - er * inv_p) * (double)dscale;
            d[1] = ((double)cs[1] * wa - ei * inv_p) * (double)dscale;
        }
        Db[N48 ? pd16_n48_index(2 * k, a, n_stage) : pd16_index(2 * k, a, n_stage)] = f64_to_f16(d[0]);
        Db[N48 ? pd16_n48_index(2 * k + 1, a, n_stage) : pd16_index(2 * k + 1, a, n_stage)] = f64_to_f16(d[1]);
    }
}

// the tables of the 48-node route: the node table first, then the D image from its hi pieces (d_L, d_phi: the 48-node plan's)
int launch_lowrank_tables_n48(psa_ctx* c, const float* d_kvec, const double* d_geo, const double* d_kappa, const float* d_mean_all,
                              const int* d_idx, const float* d_L, const float2* d_phi, void* d_diff, void* d_nodes, const ProjGeom& g,
                              int M_pad_d, float dscale, bool pair) {
    PSA_REQUIRE(M_pad_d % D_M_BLK == 0 && M_pad_d >= 2 * g.K && g.A_pad % K1_BA == 0, "bad low-rank table geometry");
    PSA_REQUIRE(!pair || M_pad_d == LRN_ROWS, "the 48-node pair launch's image is one 512-row block");
    hipLaunchKernelGGL(node_table_n48_kernel, dim3(64, (g.A_pad + 255) / 256), dim3(256), 0, c->stream, d_geo, d_kappa, d_mean_all,
                       d_idx, g.weights, 1.f / g.wscale, (_Float16*)d_nodes, g.n_g, g.A_pad);
    PSA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pair ? diff_n48_table_kernel<true> : diff_n48_table_kernel<false>,
                       dim3(M_pad_d / 2 / FOLD_JB, (g.A_pad + 255) / 256), dim3(256), 0, c->stream, d_kvec, d_mean_all, d_idx, g.weights,
                       1.f / g.wscale, (const _Float16*)d_nodes, d_L, d_phi, (_Float16*)d_diff, g.K, g.n_g, g.A_pad, dscale);
    PSA_HIP_CHECK(hipGetLastError());
    if (pair) {      // each role's part ends with its own padding stages
        const size_t n_stage = (size_t)g.A_pad / K1_BA, a_pad = LRN_PAD_STAGES * LRN_A_UNITS * 1024, b_pad = LRN_PAD_STAGES * LRN_B_UNITS * 1024;
        static_assert(LRN_ROWS == D_M_BLK, "the 48-node image has the size of one D block");
        PSA_HIP_CHECK(hipMemsetAsync((char*)d_diff + n_stage * LRN_A_UNITS * 1024, 0, a_pad, c->stream));
        PSA_HIP_CHECK(hipMemsetAsync((char*)d_diff + pd16_n48_table_bytes((int)n_stage) - b_pad, 0, b_pad, c->stream));
    } else {
        PSA_HIP_CHECK(hipMemsetAsync((char*)d_diff + (size_t)M_pad_d * g.A_pad * 2, 0,
                                     pd16_table_bytes(M_pad_d, g.A_pad) - (size_t)M_pad_d * g.A_pad * 2, c->stream));
    }
    return PSA_OK;
}

}  // namespace psa
