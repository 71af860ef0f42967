// K1 low-rank route for k-paths, ONE launch of balanced row pairs: the node rows (k1_planes_lw.hip on the node table)
// and the D pass (k1_planes_diff.hip) of a list with a single 512-row D block, run by two sibling workgroups per
// 64-frame tile that multiply the same amount per 32-atom stage.
//
// The two-pass route reads the hi plane twice from HBM (node pass: both planes; D pass: the hi plane again).  Here
// the grid is k1_grid with two "M blocks" per frame tile, so k1_block_map puts the tile's two workgroups (blocks b and
// b + 8) on one XCD; both stream the tile's hi plane with the default cache policy, so that whichever comes second can
// find it in that XCD's L2.  Nothing couples them -- no flag, no atomic, no wait: one that falls behind only pays an
// HBM read.  Measured (profiles/lowrank_pair_*): a stage costs both the same 336 MFMAs but role A
// 5.8 % more time, role B runs some 50 stages ahead by the end of a tile and the launch still fetches what the two
// passes fetched; it is 0.2 ms per step faster than they are at configuration 3 all the same.
//
//   role A (mb = 0): the 128 node rows, three products per row tile and component, and D rows 0..63, one product
//                    (8 x 3 + 4 = 28 row-tile products x 12 column tiles);
//   role B (mb = 1): D rows 64..511, one product (28 row tiles x 12 column tiles).
//
// Both roles have the D pass's shape: eight wavefronts, two per SIMD, wavefront w = 4 h + f owns row half h x frames
// [16 f, +16) x 3 components; a ring of 160 one-KiB units of LDS (unit_off, k1_f16.h) filled by wavefronts 0-3, unit
// 4 i + w by instruction i of wavefront w, two to three stages ahead; one barrier per stage behind a counted vmcnt.
//
// Role A: a stage is 44 units -- 24 plane units (unit 4 (2 c + p) + j: component c, piece p, frame group j), 16 node
// units (unit 24 + 8 p + 2 mt + h: piece p of the node table's rows [64 h + 16 mt, +16)) and 4 D units (unit
// 40 + 2 mt + h: D rows [32 h + 16 mt, +16)) -- in the D pass's ring: positions repeat every 40 stages, the loop is
// unrolled 40 times.  Node rows keep k1_planes_lw.hip's arithmetic bit for bit: per row tile and component the chain
// mma(a[1], b[0]), mma(a[0], b[1]), mma(a[0], b[0]), restarted from zero and folded into float32 sums every 8 stages
// (k1_fold; k1_chain_loop's chains, written out because its ring slot is a run-time number and this ring's addresses
// are constants).  The four row tiles' chains are interleaved, which changes no chain.  30 accumulator tiles per
// wavefront: 4 x 3 chains, their 4 x 3 sums, 2 x 3 of D; two sets of A fragments, so that the next stage's are read
// while this one multiplies.  The lo plane is read by role A alone: non-temporal.
// Role B: the D pass's body with 14 row tiles per row half; a stage is 40 units -- 12 hi-plane units (unit 4 c + j)
// and 28 D units (unit 12 + 2 mt + h) --, the ring four whole stages.  42 accumulator tiles.
// D rows: one unfolded chain over all stages in both roles, as in the D pass.  q before the combine is bit-identical
// to the two-pass route's.
#include <utility>

#include "k1_f16.h"
#include "k1_lowrank_pair.h"

namespace psa {

namespace {
constexpr int LP_T_BLK = 64, LP_RING_UNITS = 160;
constexpr int LPA_STAGE_UNITS = 44, LPA_PERIOD = 40, LPA_FOLD = 8, LPA_MT = 4, LPA_DT = LRP_A_UNITS / 2;
constexpr int LPA_NODE_U0 = 24, LPA_D_U0 = 40;
constexpr int LPA_EARLY = LP_RING_UNITS - 3 * LPA_STAGE_UNITS;                                   // 28
constexpr int LPB_STAGE_UNITS = 12 + LRP_B_UNITS, LPB_PERIOD = LP_RING_UNITS / LPB_STAGE_UNITS, LPB_D_U0 = 12;
constexpr int LP_NODE_STAGE_BYTES = pf16_stage_bytes(2 * LOWRANK_NODES);                         // 16 KiB
static_assert(LPA_EARLY == 28 && LPA_PERIOD % LPA_FOLD == 0 && LPA_D_U0 + LRP_A_UNITS == LPA_STAGE_UNITS, "role A's ring");
static_assert(LPB_STAGE_UNITS == 40 && LPB_PERIOD == 4, "role B's ring is four whole stages");
static_assert(3 * 3 * LPA_MT + 3 * LPA_DT == 3 * LRP_B_MT, "both roles multiply the same per stage: 42 MFMAs per wavefront");
constexpr auto a_unit_off = unit_off<LPA_STAGE_UNITS, LP_RING_UNITS, LPA_PERIOD>;
constexpr auto b_unit_off = unit_off<LPB_STAGE_UNITS, LP_RING_UNITS, LPB_PERIOD>;
}  // namespace

__global__ void __launch_bounds__(512, 2)
k1_lowrank_pair_kernel(const _Float16* __restrict__ planes, const _Float16* __restrict__ Pn, const _Float16* __restrict__ Dp,
                       float2* __restrict__ Qn, float2* __restrict__ Q, int64_t T, int64_t q_stride, int n_fg, int n_stage, int K,
                       int n_tblk, float qscale_n, float qscale_d) {
    using PR = F16x2;
    using E8 = PR::v8;
    using std::integral_constant;
    __shared__ __attribute__((aligned(16))) unsigned char smem[LP_RING_UNITS * 1024];
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
    const unsigned wbase = lds0 + 1024 * wf;                            // unit 4 i + w: 1024 w past unit 4 i (no wrap: both stages are multiples of 4)
    // fragment reads: every unit is 16 rows (frames) x 64 bytes, lane (r16, q) takes 16 bytes; A units come in pairs
    // 2 mt + h, B units in fours 4 x + f
    const unsigned lane_off = lds0 + r16 * (K1_BA * 2) + ((q ^ pl_swizzle(r16)) << 4);
    unsigned       lane_a[3], lane_b[3];
    unit_ring_windows(lane_off + 1024 * wh, lane_off + 1024 * wf, lane_a, lane_b);
    using I0 = integral_constant<int, 0>;
    using I1 = integral_constant<int, 1>;
    using I2 = integral_constant<int, 2>;

    if (mb == 0) {
        // =============================== role A: node rows + D rows 0..63 ===============================
        // waves 0-3: eleven source streams, instruction i = unit 4 i + w of every stage.  i = 0..5: block i = 2 c + p of
        // frame group w; i = 6..9: the node table's KiB 8 p + 4 h + mt for unit x = 4 (i - 6) + w = 8 p + 2 mt + h;
        // i = 10: D unit w
        const unsigned char* src[11];
#pragma unroll
        for (int i = 0; i < 6; ++i) src[i] = pl0 + 1024 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = 4 * j + wf;
            src[6 + j] = reinterpret_cast<const unsigned char*>(Pn) + 1024 * (8 * (x >> 3) + 4 * (x & 1) + ((x >> 1) & 3));
        }
        src[10] = reinterpret_cast<const unsigned char*>(Dp) + 1024 * wf;
        auto dma = [&](auto s40_c, auto i_c) __attribute__((always_inline)) {
            constexpr int      S40 = decltype(s40_c)::value, I = decltype(i_c)::value;
            constexpr unsigned OFF = a_unit_off(S40, 4 * I);
            if constexpr (I < 6) {
                lds_dma16_at<OFF, (I & 1) != 0>(src[I], dma_voff, wbase);     // the lo piece is this role's alone: non-temporal
                src[I] += PL_STAGE_BYTES;
            } else if constexpr (I < 10) {
                lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);
                src[I] += LP_NODE_STAGE_BYTES;
            } else {
                lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);
                src[I] += LRP_A_UNITS * 1024;
            }
        };
        auto dma_range = [&]<int S40, int... Is>(integral_constant<int, S40>, std::integer_sequence<int, Is...>) __attribute__((always_inline)) {
            (dma(integral_constant<int, S40>{}, integral_constant<int, Is>{}), ...);
        };
        // units 0..27 of a stage are instructions 0..6, units 28..43 instructions 7..10
        auto dma_late = [&](auto s40_c) __attribute__((always_inline)) { dma_range(s40_c, std::integer_sequence<int, 7, 8, 9, 10>{}); };
        auto dma_early = [&](auto s40_c) __attribute__((always_inline)) { dma_range(s40_c, std::make_integer_sequence<int, 7>{}); };

        // A fragments in two sets, [stage parity]: a stage reads the next one's into the other set while it multiplies
        // (read behind their last use instead, they come back only at the stage's end, and after the barrier both
        // wavefronts of a SIMD wait for LDS at once: 13 % longer stages, measured).  B fragments are read again in place.
        E8    a[2][2][LPA_MT];                         // node A fragments [parity][piece][row tile]
        E8    ad[2][LPA_DT];                           // D A fragments [parity][row tile]
        E8    bb[3][2];                                // B fragments [component][piece]
        f32x4 hi[LPA_MT][3], lo[LPA_MT][3], accd[LPA_DT][3];
        auto  read_a = [&](auto s40_c, auto p_c, auto mt_c) __attribute__((always_inline)) {
            constexpr int S40 = decltype(s40_c)::value, P = decltype(p_c)::value, MTI = decltype(mt_c)::value;
            a[S40 & 1][P][MTI] = lds_frag(lane_a, a_unit_off(S40, LPA_NODE_U0 + 8 * P + 2 * MTI));
        };
        auto read_ad = [&](auto s40_c, auto mt_c) __attribute__((always_inline)) {
            constexpr int S40 = decltype(s40_c)::value, MTI = decltype(mt_c)::value;
            ad[S40 & 1][MTI] = lds_frag(lane_a, a_unit_off(S40, LPA_D_U0 + 2 * MTI));
        };
        auto read_b = [&](auto s40_c, auto c_c, auto p_c) __attribute__((always_inline)) {
            constexpr int S40 = decltype(s40_c)::value, CC = decltype(c_c)::value, P = decltype(p_c)::value;
            bb[CC][P] = lds_frag(lane_b, a_unit_off(S40, 4 * (2 * CC + P)));
        };
        auto each_mt = [&](auto&& f) __attribute__((always_inline)) {
            f(I0{});
            f(I1{});
            f(I2{});
            f(integral_constant<int, 3>{});
        };
        static_assert(LPA_PERIOD % 2 == 0, "the fragment sets alternate with the stage");
#pragma unroll
        for (int mt = 0; mt < LPA_MT; ++mt)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                hi[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
                lo[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
        for (int mt = 0; mt < LPA_DT; ++mt)
#pragma unroll
            for (int c = 0; c < 3; ++c) accd[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};

        // ---- prologue: stages 0 and 1 whole, units 0..27 of stage 2; every fragment of stage 0 --------------------
        if (wh == 0) {
            dma_early(I0{});
            dma_late(I0{});
            dma_early(I1{});
            dma_late(I1{});
            dma_early(I2{});
        }
        asm volatile("s_waitcnt vmcnt(7)\n\ts_barrier" ::: "memory");      // stages 0 and 1 landed
        each_mt([&](auto mt_c) __attribute__((always_inline)) {
            read_a(I0{}, I1{}, mt_c);
            read_a(I0{}, I0{}, mt_c);
        });
        read_b(I0{}, I0{}, I0{});
        read_b(I0{}, I0{}, I1{});
        read_ad(I0{}, I0{});
        read_ad(I0{}, I1{});
        read_b(I0{}, I1{}, I0{});
        read_b(I0{}, I1{}, I1{});
        read_b(I0{}, I2{}, I0{});
        read_b(I0{}, I2{}, I1{});

        int  left = n_stage;                                               // stages to go when the period began
        // One stage: every fragment of stage s is in registers.  Stage s + 1's A fragments are read into the other set
        // during component 0 and 1, its B fragments in place behind their component.  Nothing is read from the stage's
        // own units, which are overwritten right after the barrier.
        auto stage = [&](auto s40_c) __attribute__((always_inline)) {
            constexpr int S40 = decltype(s40_c)::value, PAR = S40 & 1;
            if (left <= S40) return;                                       // past the group's last stage
            constexpr bool restart = S40 % LPA_FOLD == 0;                  // a chain's first stage: from zero
            using SN = integral_constant<int, (S40 + 1) % LPA_PERIOD>;
            using SNN = integral_constant<int, (S40 + 2) % LPA_PERIOD>;
            using S3 = integral_constant<int, (S40 + 3) % LPA_PERIOD>;
            if (wh == 0) {                                                 // stage s-1's units are free
                dma_late(SNN{});
                dma_early(S3{});
            }
            auto comp = [&](auto c_c) __attribute__((always_inline)) {
                constexpr int CC = decltype(c_c)::value;
                f32x4         ch[LPA_MT];
                each_mt([&](auto mt_c) __attribute__((always_inline)) {
                    constexpr int MTI = decltype(mt_c)::value;
                    ch[MTI] = PR::mma(a[PAR][1][MTI], bb[CC][0], restart ? f32x4{0.f, 0.f, 0.f, 0.f} : hi[MTI][CC]);
                });
                if constexpr (CC == 0) each_mt([&](auto mt_c) __attribute__((always_inline)) { read_a(SN{}, I1{}, mt_c); });
                if constexpr (CC == 1) {
                    read_ad(SN{}, I0{});
                    read_ad(SN{}, I1{});
                }
                __builtin_amdgcn_sched_barrier(0);
                each_mt([&](auto mt_c) __attribute__((always_inline)) {
                    constexpr int MTI = decltype(mt_c)::value;
                    ch[MTI] = PR::mma(a[PAR][0][MTI], bb[CC][1], ch[MTI]);
                });
                read_b(SN{}, c_c, I1{});
                if constexpr (CC == 0) each_mt([&](auto mt_c) __attribute__((always_inline)) { read_a(SN{}, I0{}, mt_c); });
                __builtin_amdgcn_sched_barrier(0);
                accd[0][CC] = PR::mma(ad[PAR][0], bb[CC][0], accd[0][CC]);
                accd[1][CC] = PR::mma(ad[PAR][1], bb[CC][0], accd[1][CC]);
                each_mt([&](auto mt_c) __attribute__((always_inline)) {
                    constexpr int MTI = decltype(mt_c)::value;
                    hi[MTI][CC] = PR::mma(a[PAR][0][MTI], bb[CC][0], ch[MTI]);
                });
                read_b(SN{}, c_c, I0{});
                __builtin_amdgcn_sched_barrier(0);
            };
            comp(I0{});
            comp(I1{});
            comp(I2{});
            asm volatile("s_waitcnt vmcnt(7)\n\ts_barrier" ::: "memory");     // stages s+1 and s+2 landed
        };
        // k1_chain_loop's chains: up to LPA_FOLD stages from zero, folded into lo
        auto chain = [&](auto c_c) __attribute__((always_inline)) {
            constexpr int C0 = decltype(c_c)::value * LPA_FOLD;
            if (left <= C0) return;
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) __attribute__((always_inline)) { (stage(integral_constant<int, C0 + Ss>{}), ...); }(
                std::make_integer_sequence<int, LPA_FOLD>{});
            k1_fold(lo, hi);
        };
        for (; left > 0; left -= LPA_PERIOD)
            [&]<int... Cs>(std::integer_sequence<int, Cs...>) __attribute__((always_inline)) { (chain(integral_constant<int, Cs>{}), ...); }(
                std::make_integer_sequence<int, LPA_PERIOD / LPA_FOLD>{});
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // nothing in flight when LDS is handed on

        // ---- epilogue: the lane's coordinates are taken afresh (k1_planes_diff.hip)
        const int     lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int     r16_e = lane_e & 15, q_e = lane_e >> 4;
        const int64_t t = (int64_t)tb * LP_T_BLK + wf * 16 + r16_e;
        k1_store_q(Qn, lo, wh * LOWRANK_NODES, q_e, t, T, LOWRANK_NODES, T, qscale_n);
        k1_store_q(Q, accd, wh * (LRP_A_ROWS / 2), q_e, t, T, K, q_stride, qscale_d);
    } else {
        // =============================== role B: D rows 64..511 ===============================
        // waves 0-3: ten source streams.  i = 0..2: hi piece of component i of frame group w; i = 3..9: D unit w + 4 (i - 3)
        const unsigned char* src[10];
#pragma unroll
        for (int i = 0; i < 3; ++i) src[i] = pl0 + 1024 * (2 * i);
        const unsigned char* d0 = reinterpret_cast<const unsigned char*>(Dp) + lrp_b_first_unit(n_stage) * 1024;
#pragma unroll
        for (int i = 3; i < 10; ++i) src[i] = d0 + 1024 * (wf + 4 * (i - 3));
        auto dma = [&](auto s4_c, auto i_c) __attribute__((always_inline)) {
            constexpr int      S4 = decltype(s4_c)::value, I = decltype(i_c)::value;
            constexpr unsigned OFF = b_unit_off(S4, 4 * I);
            lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);          // the hi plane with the default policy: the sibling's hit
            src[I] += I < 3 ? PL_STAGE_BYTES : LRP_B_UNITS * 1024;
        };
        auto dma_stage = [&](auto s4_c) __attribute__((always_inline)) {
            [&]<int... Is>(std::integer_sequence<int, Is...>) __attribute__((always_inline)) { (dma(s4_c, integral_constant<int, Is>{}), ...); }(
                std::make_integer_sequence<int, 10>{});
        };

        E8    a[4];                                    // A fragments of four consecutive row tiles, read two ahead
        E8    bf[3];                                   // hi B fragments of the stage in work
        f32x4 acc[LRP_B_MT][3];
        // row tile mt of stage s is the (14 s + mt)-th of the launch: its place in the ring of four
        auto read_a = [&](auto s4_c, auto mt_c) __attribute__((always_inline)) {
            constexpr int S4 = decltype(s4_c)::value, MTI = decltype(mt_c)::value;
            a[(LRP_B_MT * S4 + MTI) & 3] = lds_frag(lane_a, b_unit_off(S4, LPB_D_U0 + 2 * MTI));
        };
        auto read_b = [&](auto s4_c, auto c_c) __attribute__((always_inline)) {
            constexpr int S4 = decltype(s4_c)::value, CC = decltype(c_c)::value;
            bf[CC] = lds_frag(lane_b, b_unit_off(S4, 4 * CC));
        };
#pragma unroll
        for (int mt = 0; mt < LRP_B_MT; ++mt)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};

        // ---- prologue: stages 0, 1 and 2 ------------------------------------------------------------------------
        if (wh == 0) {
            dma_stage(I0{});
            dma_stage(I1{});
            dma_stage(I2{});
        }
        asm volatile("s_waitcnt vmcnt(10)\n\ts_barrier" ::: "memory");     // stages 0 and 1 landed
        read_b(I0{}, I0{});
        read_b(I0{}, I1{});
        read_b(I0{}, I2{});
        read_a(I0{}, I0{});
        read_a(I0{}, I1{});

        int  left = n_stage;
        auto stage = [&](auto s4_c) __attribute__((always_inline)) {
            constexpr int S4 = decltype(s4_c)::value;
            if (left <= S4) return;                                        // past the group's last stage
            using SN = integral_constant<int, (S4 + 1) % LPB_PERIOD>;
            using S3 = integral_constant<int, (S4 + 3) % LPB_PERIOD>;
            if (wh == 0) dma_stage(S3{});                                  // into stage s-1's units, which are free
            auto tile = [&](auto mt_c) __attribute__((always_inline)) {
                constexpr int MTI = decltype(mt_c)::value;
                if constexpr (MTI + 2 < LRP_B_MT)
                    read_a(s4_c, integral_constant<int, MTI + 2>{});
                else
                    read_a(SN{}, integral_constant<int, MTI + 2 - LRP_B_MT>{});
                auto comp = [&](auto c_c) __attribute__((always_inline)) {
                    constexpr int CC = decltype(c_c)::value;
                    acc[MTI][CC] = PR::mma(a[(LRP_B_MT * S4 + MTI) & 3], bf[CC], acc[MTI][CC]);
                    if constexpr (MTI == LRP_B_MT - 1) read_b(SN{}, c_c);  // behind the component's last use in this stage
                };
                comp(I0{});
                comp(I1{});
                comp(I2{});
                __builtin_amdgcn_sched_barrier(0);
            };
            [&]<int... Ms>(std::integer_sequence<int, Ms...>) __attribute__((always_inline)) { (tile(integral_constant<int, Ms>{}), ...); }(
                std::make_integer_sequence<int, LRP_B_MT>{});
            // what this stage read from its own units has been consumed above; reads in flight come from stage s+1
            asm volatile("s_waitcnt vmcnt(10)\n\ts_barrier" ::: "memory");    // stages s+1 and s+2 landed
        };
        for (; left > 0; left -= LPB_PERIOD)
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) __attribute__((always_inline)) { (stage(integral_constant<int, Ss>{}), ...); }(
                std::make_integer_sequence<int, LPB_PERIOD>{});
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

        const int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int r16_e = lane_e & 15, q_e = lane_e >> 4;
        k1_store_q(Q, acc, wh * (16 * LRP_B_MT) + LRP_A_ROWS, q_e, (int64_t)tb * LP_T_BLK + wf * 16 + r16_e, T, K, q_stride, qscale_d);
    }
}

// d_planes: the group's planes from its first frame group on; d_nodes: the node table (one 128-row block of the phase-table
// image); d_diff: the D image in the pair layout (pd16_pair_index), one 512-row block; d_qn: (64, 3, g.T) node projections;
// dscale: the power of two the D image was multiplied by
int launch_k1_lowrank_pair(psa_ctx* c, const void* d_planes, const void* d_nodes, const void* d_diff, float2* d_qn, float2* d_q,
                           const ProjGeom& g, int64_t n_fg, float dscale) {
    PSA_REQUIRE(g.M_pad_d == LRP_ROWS && 2 * g.K <= LRP_ROWS && g.K > 0, "pair launch: one 512-row D block only");
    PSA_REQUIRE(g.A_pad % (2 * K1_BA) == 0 && g.A_pad > 0, "pair launch needs the atom axis padded to %d", 2 * K1_BA);
    PSA_REQUIRE(g.vscale > 0.f && dscale > 0.f && n_fg * 16 >= g.T, "planes do not cover the launch");
    ProjGeom g2 = g;
    g2.M_pad = 2 * LRP_ROWS;                                             // two roles per frame tile
    K1Grid gr;
    PSA_TRY(k1_grid(g2, LRP_ROWS, LP_T_BLK, gr));
    PSA_REQUIRE(gr.n_mblk == 2 && gr.n_tblk < (1 << 29) && n_fg < (1ll << 31), "projection grid too large");
    const float qscale_n = 1.f / (g.vscale * F16x2::P_SCALE) * g.wscale;      // powers of two: exact (launch_planes_family)
    const float qscale_d = 1.f / (g.vscale * dscale) * g.wscale;
    hipLaunchKernelGGL(k1_lowrank_pair_kernel, dim3(gr.blocks), dim3(512), 0, c->stream, (const _Float16*)d_planes,
                       (const _Float16*)d_nodes, (const _Float16*)d_diff, d_qn, d_q, g.T, g.q_stride, (int)n_fg, g.A_pad / K1_BA, g.K,
                       gr.n_tblk, qscale_n, qscale_d);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
