// K1 low-rank route for k-paths, the FOLDED pair launch (psa_set_k1_lowrank_fold): k1_lowrank_pair.hip's launch with one
// product fewer per node row.
//
// The route computes q = phi L (W_hi v_hi + W_hi v_lo + W_lo v_hi) + D v_hi.  Two of these terms meet v_hi, and the
// combine is linear: phi L (W_lo v_hi) = (phi L W_lo) v_hi = E v_hi, with E[j, a] = phi_j sum_l L[j, l] W_lo[l, a] a
// K x atoms table that, like D, depends on the plan and the node table alone and is as small as D.  The folded D image
// holds D' = D + E (diff_fold_table_kernel, k1_planes_diff.hip), so the node rows keep two products, read the node
// table's hi piece only, and a stage is 768 row-products instead of 896.
//
// The launch has k1_lowrank_pair.hip's shape -- k1_grid with two "M blocks" per 64-frame tile, so k1_block_map puts the
// tile's two workgroups on one XCD; eight wavefronts, two per SIMD, wavefront w = 4 h + f owns row half h x frames
// [16 f, +16) x 3 components; rings of one-KiB units filled by wavefronts 0-3, unit 4 i + w by instruction i of
// wavefront w, three stages ahead; one barrier per stage behind a counted vmcnt; nothing couples the roles -- and the
// balanced split is 24 row-tile products per role and stage, 36 MFMAs per wavefront:
//
//   role A (mb = 0): the 128 node rows, two products per row tile and component, and D' rows 0..127, one product
//                    (8 x 2 + 8 = 24 row-tile products x 12 column tiles);
//   role B (mb = 1): D' rows 128..511, one product (24 row tiles x 12 column tiles).
//
// Role A: a stage is 40 units -- 24 plane units (unit 4 (2 c + p) + j: component c, piece p, frame group j), 8 node
// units (unit 24 + 2 mt + h: the hi piece of the node table's rows [64 h + 16 mt, +16); the hi piece is the first 8 KiB
// of each 16-KiB stage of the node table image, whose lo piece is never fetched) and 8 D' units (unit 32 + 2 mt + h:
// D' rows [64 h + 16 mt, +16)) --, the ring four whole stages, the loop unrolled over the 8 stages of a fold.  Node rows
// keep the arithmetic of k1_planes_lw.hip's two-product instantiation bit for bit: per row tile and component the chain
// mma(a, b[1]), mma(a, b[0]), restarted from zero and folded into float32 sums every 8 stages (k1_fold).  The D' chain
// of a row tile runs between the two, so that eight independent MFMAs separate a chain's dependent pair.  36
// accumulator tiles per wavefront: 4 x 3 chains, their 4 x 3 sums, 4 x 3 of D'; two sets of A fragments, so that the
// next stage's are read while this one multiplies.  The lo plane is read by role A alone: non-temporal.
// Role B: the D pass's body with 12 row tiles per row half; a stage is 36 units -- 12 hi-plane units (unit 4 c + j) and
// 24 D' units (unit 12 + 2 mt + h) --, the ring four whole stages in 144 of the 160 KiB.  36 accumulator tiles.
// D' rows: one unfolded chain over all stages in both roles, as in the D pass.  q before the combine is bit-identical
// to that of the folded two passes (k1_planes_lw2_kernel, k1_planes_diff_kernel on the folded image).
#include <utility>

#include "k1_f16.h"
#include "k1_lowrank_fold.h"

namespace psa {

namespace {
constexpr int LF_T_BLK = 64, LF_PERIOD = 4;
constexpr int LFA_STAGE_UNITS = 24 + 8 + LRF_A_UNITS, LFA_RING_UNITS = LF_PERIOD * LFA_STAGE_UNITS, LFA_FOLD = 8, LFA_MT = LRF_A_MT;
constexpr int LFA_NODE_U0 = 24, LFA_D_U0 = 32, LFA_DMA = LFA_STAGE_UNITS / 4;
constexpr int LFB_STAGE_UNITS = 12 + LRF_B_UNITS, LFB_RING_UNITS = LF_PERIOD * LFB_STAGE_UNITS, LFB_D_U0 = 12, LFB_DMA = LFB_STAGE_UNITS / 4;
constexpr int LF_NODE_STAGE_BYTES = pf16_stage_bytes(2 * LOWRANK_NODES);                         // 16 KiB, the hi piece its first 8
static_assert(LFA_STAGE_UNITS == 40 && LFA_RING_UNITS == 160 && LFA_FOLD % LF_PERIOD == 0 && LFA_DMA == 10, "role A's ring is four whole stages");
static_assert(LFB_STAGE_UNITS == 36 && LFB_RING_UNITS == 144 && LFB_DMA == 9, "role B's ring is four whole stages");
static_assert(3 * 2 * LFA_MT + 3 * LFA_MT == 3 * LRF_B_MT, "both roles multiply the same per stage: 36 MFMAs per wavefront");
constexpr auto a_unit_off = unit_off<LFA_STAGE_UNITS, LFA_RING_UNITS, LF_PERIOD>;
constexpr auto b_unit_off = unit_off<LFB_STAGE_UNITS, LFB_RING_UNITS, LF_PERIOD>;
}  // namespace

__global__ void __launch_bounds__(512, 2)
k1_lowrank_fold_kernel(const _Float16* __restrict__ planes, const _Float16* __restrict__ Pn, const _Float16* __restrict__ Dp,
                       float2* __restrict__ Qn, float2* __restrict__ Q, int64_t T, int64_t q_stride, int n_fg, int n_stage, int K,
                       int n_tblk, float qscale_n, float qscale_d) {
    using PR = F16x2;
    using E8 = PR::v8;
    using std::integral_constant;
    __shared__ __attribute__((aligned(16))) unsigned char smem[LFA_RING_UNITS * 1024];
    const unsigned lds0 = (unsigned)(size_t)(lds_u8*)smem;

    int mb, tb;                                        // role, 64-frame tile (k1_block_map: the roles of a tile share an XCD)
    if (!k1_block_map(2, n_tblk, mb, tb)) return;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wh = w >> 2, wf = w & 3;
    const int r16 = lane & 15, q = lane >> 4;

    int fg = tb * 4 + wf;                                               // frame group (past the end: the last one, never stored)
    if (fg >= n_fg) fg = n_fg - 1;
    const unsigned char* pl0 = reinterpret_cast<const unsigned char*>(planes) + (size_t)fg * n_stage * PL_STAGE_BYTES;
    const unsigned dma_voff = 16 * lane;
    const unsigned wbase = lds0 + 1024 * wf;                            // unit 4 i + w: 1024 w past unit 4 i (no wrap: stages and rings are multiples of 4)
    // fragment reads: every unit is 16 rows (frames) x 64 bytes, lane (r16, q) takes 16 bytes; A units come in pairs
    // 2 mt + h, B units in fours 4 x + f
    const unsigned lane_off = lds0 + r16 * (K1_BA * 2) + ((q ^ pl_swizzle(r16)) << 4);
    unsigned       lane_a[3], lane_b[3];
    unit_ring_windows(lane_off + 1024 * wh, lane_off + 1024 * wf, lane_a, lane_b);
    using I0 = integral_constant<int, 0>;
    using I1 = integral_constant<int, 1>;
    using I2 = integral_constant<int, 2>;
    using I3 = integral_constant<int, 3>;

    if (mb == 0) {
        // =============================== role A: node rows + D' rows 0..127 ===============================
        // waves 0-3: ten source streams, instruction i = unit 4 i + w of every stage.  i = 0..5: block i = 2 c + p of
        // frame group w; i = 6, 7: the node table's KiB 4 h + mt (hi piece) for unit x = 4 (i - 6) + w = 2 mt + h;
        // i = 8, 9: D' unit 4 (i - 8) + w
        const unsigned char* src[LFA_DMA];
#pragma unroll
        for (int i = 0; i < 6; ++i) src[i] = pl0 + 1024 * i;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int x = 4 * j + wf;
            src[6 + j] = reinterpret_cast<const unsigned char*>(Pn) + 1024 * (4 * (x & 1) + (x >> 1));
            src[8 + j] = reinterpret_cast<const unsigned char*>(Dp) + 1024 * x;
        }
        auto dma = [&](auto s4_c, auto i_c) __attribute__((always_inline)) {
            constexpr int      S4 = decltype(s4_c)::value, I = decltype(i_c)::value;
            constexpr unsigned OFF = a_unit_off(S4, 4 * I);
            if constexpr (I < 6) {
                lds_dma16_at<OFF, (I & 1) != 0>(src[I], dma_voff, wbase);     // the lo piece is this role's alone: non-temporal
                src[I] += PL_STAGE_BYTES;
            } else if constexpr (I < 8) {
                lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);
                src[I] += LF_NODE_STAGE_BYTES;
            } else {
                lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);
                src[I] += LRF_A_UNITS * 1024;
            }
        };
        auto dma_stage = [&](auto s4_c) __attribute__((always_inline)) {
            [&]<int... Is>(std::integer_sequence<int, Is...>) __attribute__((always_inline)) { (dma(s4_c, integral_constant<int, Is>{}), ...); }(
                std::make_integer_sequence<int, LFA_DMA>{});
        };

        // A fragments in two sets, [stage parity]: a stage reads the next one's into the other set while it multiplies
        // (k1_lowrank_pair.hip).  B fragments are read again in place.
        E8    a[2][LFA_MT];                            // node A fragments (hi piece) [parity][row tile]
        E8    ad[2][LFA_MT];                           // D' A fragments [parity][row tile]
        E8    bb[3][2];                                // B fragments [component][piece]
        f32x4 hi[LFA_MT][3], lo[LFA_MT][3], accd[LFA_MT][3];
        auto  read_a = [&](auto s_c, auto mt_c) __attribute__((always_inline)) {
            constexpr int S = decltype(s_c)::value, MTI = decltype(mt_c)::value;
            a[S & 1][MTI] = lds_frag(lane_a, a_unit_off(S, LFA_NODE_U0 + 2 * MTI));
        };
        auto read_ad = [&](auto s_c, auto mt_c) __attribute__((always_inline)) {
            constexpr int S = decltype(s_c)::value, MTI = decltype(mt_c)::value;
            ad[S & 1][MTI] = lds_frag(lane_a, a_unit_off(S, LFA_D_U0 + 2 * MTI));
        };
        auto read_b = [&](auto s_c, auto c_c, auto p_c) __attribute__((always_inline)) {
            constexpr int S = decltype(s_c)::value, CC = decltype(c_c)::value, P = decltype(p_c)::value;
            bb[CC][P] = lds_frag(lane_b, a_unit_off(S, 4 * (2 * CC + P)));
        };
        auto each_mt = [&](auto&& f) __attribute__((always_inline)) {
            f(I0{});
            f(I1{});
            f(I2{});
            f(I3{});
        };
        static_assert(LFA_MT == 4 && LFA_FOLD % 2 == 0, "four row tiles; the fragment sets alternate with the stage");
#pragma unroll
        for (int mt = 0; mt < LFA_MT; ++mt)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                hi[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
                lo[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
                accd[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }

        // ---- prologue: stages 0, 1 and 2; every fragment of stage 0 --------------------------------------------
        if (wh == 0) {
            dma_stage(I0{});
            dma_stage(I1{});
            dma_stage(I2{});
        }
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(LFA_DMA) : "memory");      // stages 0 and 1 landed
        each_mt([&](auto mt_c) __attribute__((always_inline)) { read_a(I0{}, mt_c); });
        read_b(I0{}, I0{}, I1{});
        read_b(I0{}, I0{}, I0{});
        each_mt([&](auto mt_c) __attribute__((always_inline)) { read_ad(I0{}, mt_c); });
        read_b(I0{}, I1{}, I1{});
        read_b(I0{}, I1{}, I0{});
        read_b(I0{}, I2{}, I1{});
        read_b(I0{}, I2{}, I0{});

        int  left = n_stage;                                               // stages to go when the fold began
        // One stage: every fragment of stage s is in registers.  Stage s + 1's A fragments are read into the other set
        // during components 0 and 1, its B fragments in place behind their last use.  Nothing is read from the stage's
        // own units; stage s - 1's are overwritten right away.
        auto stage = [&](auto s_c) __attribute__((always_inline)) {
            constexpr int S = decltype(s_c)::value, PAR = S & 1;
            if (left <= S) return;                                         // past the group's last stage
            constexpr bool restart = S == 0;                               // a chain's first stage: from zero
            using SN = integral_constant<int, (S + 1) % LFA_FOLD>;
            using S3 = integral_constant<int, (S + 3) % LFA_FOLD>;
            if (wh == 0) dma_stage(S3{});                                  // into stage s-1's units, which are free
            auto comp = [&](auto c_c) __attribute__((always_inline)) {
                constexpr int CC = decltype(c_c)::value;
                f32x4         ch[LFA_MT];
                each_mt([&](auto mt_c) __attribute__((always_inline)) {
                    constexpr int MTI = decltype(mt_c)::value;
                    ch[MTI] = PR::mma(a[PAR][MTI], bb[CC][1], restart ? f32x4{0.f, 0.f, 0.f, 0.f} : hi[MTI][CC]);
                });
                read_b(SN{}, c_c, I1{});
                if constexpr (CC == 0) each_mt([&](auto mt_c) __attribute__((always_inline)) { read_a(SN{}, mt_c); });
                if constexpr (CC == 1) each_mt([&](auto mt_c) __attribute__((always_inline)) { read_ad(SN{}, mt_c); });
                __builtin_amdgcn_sched_barrier(0);
                each_mt([&](auto mt_c) __attribute__((always_inline)) {
                    constexpr int MTI = decltype(mt_c)::value;
                    accd[MTI][CC] = PR::mma(ad[PAR][MTI], bb[CC][0], accd[MTI][CC]);
                });
                each_mt([&](auto mt_c) __attribute__((always_inline)) {
                    constexpr int MTI = decltype(mt_c)::value;
                    hi[MTI][CC] = PR::mma(a[PAR][MTI], bb[CC][0], ch[MTI]);
                });
                read_b(SN{}, c_c, I0{});
                __builtin_amdgcn_sched_barrier(0);
            };
            comp(I0{});
            comp(I1{});
            comp(I2{});
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(LFA_DMA) : "memory");     // stages s+1 and s+2 landed
        };
        // k1_chain_loop's chains: up to LFA_FOLD stages from zero, folded into lo
        for (; left > 0; left -= LFA_FOLD) {
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) __attribute__((always_inline)) { (stage(integral_constant<int, Ss>{}), ...); }(
                std::make_integer_sequence<int, LFA_FOLD>{});
            k1_fold(lo, hi);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // nothing in flight when LDS is handed on

        // ---- epilogue: the lane's coordinates are taken afresh (k1_planes_diff.hip)
        const int     lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int     r16_e = lane_e & 15, q_e = lane_e >> 4;
        const int64_t t = (int64_t)tb * LF_T_BLK + wf * 16 + r16_e;
        k1_store_q(Qn, lo, wh * LOWRANK_NODES, q_e, t, T, LOWRANK_NODES, T, qscale_n);
        k1_store_q(Q, accd, wh * (LRF_A_ROWS / 2), q_e, t, T, K, q_stride, qscale_d);
    } else {
        // =============================== role B: D' rows 128..511 ===============================
        // waves 0-3: nine source streams.  i = 0..2: hi piece of component i of frame group w; i = 3..8: D' unit w + 4 (i - 3)
        const unsigned char* src[LFB_DMA];
#pragma unroll
        for (int i = 0; i < 3; ++i) src[i] = pl0 + 1024 * (2 * i);
        const unsigned char* d0 = reinterpret_cast<const unsigned char*>(Dp) + lrf_b_first_unit(n_stage) * 1024;
#pragma unroll
        for (int i = 3; i < LFB_DMA; ++i) src[i] = d0 + 1024 * (wf + 4 * (i - 3));
        auto dma = [&](auto s4_c, auto i_c) __attribute__((always_inline)) {
            constexpr int      S4 = decltype(s4_c)::value, I = decltype(i_c)::value;
            constexpr unsigned OFF = b_unit_off(S4, 4 * I);
            lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);          // the hi plane with the default policy: the sibling's hit
            src[I] += I < 3 ? PL_STAGE_BYTES : LRF_B_UNITS * 1024;
        };
        auto dma_stage = [&](auto s4_c) __attribute__((always_inline)) {
            [&]<int... Is>(std::integer_sequence<int, Is...>) __attribute__((always_inline)) { (dma(s4_c, integral_constant<int, Is>{}), ...); }(
                std::make_integer_sequence<int, LFB_DMA>{});
        };

        E8    a[4];                                    // A fragments of four consecutive row tiles, read two ahead
        E8    bf[3];                                   // hi B fragments of the stage in work
        f32x4 acc[LRF_B_MT][3];
        static_assert(LRF_B_MT % 4 == 0, "row tile mt of every stage sits at mt mod 4 of the ring of four");
        auto read_a = [&](auto s4_c, auto mt_c) __attribute__((always_inline)) {
            constexpr int S4 = decltype(s4_c)::value, MTI = decltype(mt_c)::value;
            a[MTI & 3] = lds_frag(lane_a, b_unit_off(S4, LFB_D_U0 + 2 * MTI));
        };
        auto read_b = [&](auto s4_c, auto c_c) __attribute__((always_inline)) {
            constexpr int S4 = decltype(s4_c)::value, CC = decltype(c_c)::value;
            bf[CC] = lds_frag(lane_b, b_unit_off(S4, 4 * CC));
        };
#pragma unroll
        for (int mt = 0; mt < LRF_B_MT; ++mt)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};

        // ---- prologue: stages 0, 1 and 2 ------------------------------------------------------------------------
        if (wh == 0) {
            dma_stage(I0{});
            dma_stage(I1{});
            dma_stage(I2{});
        }
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(LFB_DMA) : "memory");      // stages 0 and 1 landed
        read_b(I0{}, I0{});
        read_b(I0{}, I1{});
        read_b(I0{}, I2{});
        read_a(I0{}, I0{});
        read_a(I0{}, I1{});

        int  left = n_stage;
        auto stage = [&](auto s4_c) __attribute__((always_inline)) {
            constexpr int S4 = decltype(s4_c)::value;
            if (left <= S4) return;                                        // past the group's last stage
            using SN = integral_constant<int, (S4 + 1) % LF_PERIOD>;
            using S3 = integral_constant<int, (S4 + 3) % LF_PERIOD>;
            if (wh == 0) dma_stage(S3{});                                  // into stage s-1's units, which are free
            auto tile = [&](auto mt_c) __attribute__((always_inline)) {
                constexpr int MTI = decltype(mt_c)::value;
                if constexpr (MTI + 2 < LRF_B_MT)
                    read_a(s4_c, integral_constant<int, MTI + 2>{});
                else
                    read_a(SN{}, integral_constant<int, MTI + 2 - LRF_B_MT>{});
                auto comp = [&](auto c_c) __attribute__((always_inline)) {
                    constexpr int CC = decltype(c_c)::value;
                    acc[MTI][CC] = PR::mma(a[MTI & 3], bf[CC], acc[MTI][CC]);
                    if constexpr (MTI == LRF_B_MT - 1) read_b(SN{}, c_c);  // behind the component's last use in this stage
                };
                comp(I0{});
                comp(I1{});
                comp(I2{});
                __builtin_amdgcn_sched_barrier(0);
            };
            [&]<int... Ms>(std::integer_sequence<int, Ms...>) __attribute__((always_inline)) { (tile(integral_constant<int, Ms>{}), ...); }(
                std::make_integer_sequence<int, LRF_B_MT>{});
            // what this stage read from its own units has been consumed above; reads in flight come from stage s+1
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(LFB_DMA) : "memory");    // stages s+1 and s+2 landed
        };
        for (; left > 0; left -= LF_PERIOD)
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) __attribute__((always_inline)) { (stage(integral_constant<int, Ss>{}), ...); }(
                std::make_integer_sequence<int, LF_PERIOD>{});
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

        const int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int r16_e = lane_e & 15, q_e = lane_e >> 4;
        k1_store_q(Q, acc, wh * (16 * LRF_B_MT) + LRF_A_ROWS, q_e, (int64_t)tb * LF_T_BLK + wf * 16 + r16_e, T, K, q_stride, qscale_d);
    }
}

// d_planes: the group's planes from its first frame group on; d_nodes: the node table (one 128-row block of the phase-table
// image; its hi piece alone is read); d_diff: the folded D image in the fold layout (pd16_fold_index), one 512-row block;
// d_qn: (64, 3, g.T) node projections; dscale: the power of two the image was multiplied by (the plan's dscale_fold)
int launch_k1_lowrank_fold(psa_ctx* c, const void* d_planes, const void* d_nodes, const void* d_diff, float2* d_qn, float2* d_q,
                           const ProjGeom& g, int64_t n_fg, float dscale) {
    PSA_REQUIRE(g.M_pad_d == LRF_ROWS && 2 * g.K <= LRF_ROWS && g.K > 0, "folded pair launch: one 512-row D block only");
    PSA_REQUIRE(g.A_pad % (2 * K1_BA) == 0 && g.A_pad > 0, "folded pair launch needs the atom axis padded to %d", 2 * K1_BA);
    PSA_REQUIRE(g.vscale > 0.f && dscale > 0.f && n_fg * 16 >= g.T, "planes do not cover the launch");
    ProjGeom g2 = g;
    g2.M_pad = 2 * LRF_ROWS;                                             // two roles per frame tile
    K1Grid gr;
    PSA_TRY(k1_grid(g2, LRF_ROWS, LF_T_BLK, gr));
    PSA_REQUIRE(gr.n_mblk == 2 && gr.n_tblk < (1 << 29) && n_fg < (1ll << 31), "projection grid too large");
    const float qscale_n = 1.f / (g.vscale * F16x2::P_SCALE) * g.wscale;      // powers of two: exact (launch_planes_family)
    const float qscale_d = 1.f / (g.vscale * dscale) * g.wscale;
    hipLaunchKernelGGL(k1_lowrank_fold_kernel, dim3(gr.blocks), dim3(512), 0, c->stream, (const _Float16*)d_planes,
                       (const _Float16*)d_nodes, (const _Float16*)d_diff, d_qn, d_q, g.T, g.q_stride, (int)n_fg, g.A_pad / K1_BA, g.K,
                       gr.n_tblk, qscale_n, qscale_d);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
