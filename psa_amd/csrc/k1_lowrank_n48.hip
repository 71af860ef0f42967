// K1 low-rank route for k-paths, the 48-NODE folded pair launch (psa_set_k1_lowrank_nodes): k1_lowrank_fold.hip's launch
// with two node row tiles fewer per stage.
//
// 64 Chebyshev nodes interpolate exp(i kappa y) over a node interval to fp64 rounding; the route does not need that,
// because the folded D image multiplies v_hi in every stage whatever it holds.  With 48 nodes the image is
//     D'[j, a] = P_ref[j, a] w_a - phi_j sum_l L[j, l] W_hi[l, a]          (diff_n48_table_kernel, k1_planes_diff.hip)
// -- everything the node rows' hi piece does not carry: D, E and the interpolation residual (<= 4.6e-7) --, the node rows
// are 96 instead of 128, and a stage is 96 x 2 + 512 = 704 row-products instead of 768.
//
// The launch has k1_lowrank_fold.hip's shape (two roles per 64-frame tile on one XCD; eight wavefronts, two per SIMD,
// wavefront w = 4 h + f owns row half h x frames [16 f, +16) x 3 components; rings of one-KiB units filled by wavefronts
// 0-3, unit 4 i + w by instruction i of wavefront w, three stages ahead; one barrier per stage behind a counted vmcnt),
// and the balanced split is 22 row-tile products per role and stage, 33 MFMAs per wavefront:
//
//   role A (mb = 0): the 96 node rows, two products per row tile and component, and D' rows 0..159, one product
//                    (6 x 2 + 10 = 22 row-tile products x 12 column tiles);
//   role B (mb = 1): D' rows 160..511, one product (22 row tiles x 12 column tiles).
//
// Role A: a stage is 40 units -- 24 plane units (unit 4 (2 c + p) + j), 6 node units (unit 24 + 2 mt + h: the hi piece of
// the node table's rows [48 h + 16 mt, +16); the table is one 128-row block whose rows 96..127 are padding and never
// fetched) and 10 D' units (unit 30 + 2 mt + h: D' rows [80 h + 16 mt, +16)) --, the ring four whole stages, the loop
// unrolled over the 8 stages of a fold.  Instruction 7 of wavefronts 0, 1 fetches a node unit, that of wavefronts 2, 3 a
// D' unit.  Node rows keep the arithmetic of k1_planes_lw.hip's two-product instantiation bit for bit: per row tile and
// component the chain mma(a, b[1]), mma(a, b[0]), restarted from zero and folded into float32 sums every 8 stages
// (k1_fold).  The five D' MFMAs of a component run between the two.  33 accumulator tiles per wavefront: 3 x 3 chains,
// their 3 x 3 sums, 5 x 3 of D'.
// Role B: the D pass's body with 11 row tiles per row half; a stage is 34 units -- 12 hi-plane units (unit 4 c + j) and
// 22 D' units (unit 12 + 2 mt + h) --, the ring four whole stages in 136 of the 160 KiB.  34 units are eight instructions
// of every filling wavefront and a ninth of wavefronts 0 and 1, whose counted wait is one longer.  33 accumulator tiles.
// D' rows: one unfolded chain over all stages in both roles, as in the D pass.  q before the combine is bit-identical
// to that of the 48-node two passes (k1_planes_lw2_kernel on the 48-node table, k1_planes_diff_kernel on the image).
#include <utility>

#include "k1_f16.h"
#include "k1_lowrank_n48.h"

namespace psa {

namespace {
constexpr int LN_T_BLK = 64, LN_PERIOD = 4;
constexpr int LNA_STAGE_UNITS = 24 + 2 * LRN_NODE_MT + LRN_A_UNITS, LNA_RING_UNITS = LN_PERIOD * LNA_STAGE_UNITS, LNA_FOLD = 8;
constexpr int LNA_NODE_U0 = 24, LNA_D_U0 = 24 + 2 * LRN_NODE_MT, LNA_DMA = LNA_STAGE_UNITS / 4;
constexpr int LNB_STAGE_UNITS = 12 + LRN_B_UNITS, LNB_RING_UNITS = LN_PERIOD * LNB_STAGE_UNITS, LNB_D_U0 = 12;
constexpr int LNB_DMA = (LNB_STAGE_UNITS + 3) / 4, LNB_LAST = LNB_STAGE_UNITS - 4 * (LNB_DMA - 1);   // 9 instructions, the last of 2 wavefronts
constexpr int LN_NODE_STAGE_BYTES = pf16_stage_bytes(128);                                          // 16 KiB, the hi piece its first 8
static_assert(LNA_STAGE_UNITS == 40 && LNA_RING_UNITS == 160 && LNA_FOLD % LN_PERIOD == 0 && LNA_DMA == 10 && LNA_D_U0 == 30,
              "role A's ring is four whole stages");
static_assert(LNB_STAGE_UNITS == 34 && LNB_RING_UNITS == 136 && LNB_DMA == 9 && LNB_LAST == 2, "role B's ring is four whole stages");
static_assert(3 * 2 * LRN_NODE_MT + 3 * LRN_A_MT == 3 * LRN_B_MT && 3 * LRN_B_MT == 33, "both roles multiply the same per stage: 33 MFMAs per wavefront");
constexpr auto a_unit_off = unit_off<LNA_STAGE_UNITS, LNA_RING_UNITS, LN_PERIOD>;
constexpr auto b_unit_off = unit_off<LNB_STAGE_UNITS, LNB_RING_UNITS, LN_PERIOD>;
// role B's A fragments, read two row tiles ahead into a ring of four: tile mt of stage s sits in slot (11 s + mt) mod 4
constexpr int lnb_slot(int s4, int mt) { return (LRN_B_MT * s4 + mt) & 3; }
static_assert((LRN_B_MT * LN_PERIOD) % 4 == 0, "the fragment slots repeat with the ring");
}  // namespace

__global__ void __launch_bounds__(512, 2)
k1_lowrank_n48_kernel(const _Float16* __restrict__ planes, const _Float16* __restrict__ Pn, const _Float16* __restrict__ Dp,
                      float2* __restrict__ Qn, float2* __restrict__ Q, int64_t T, int64_t q_stride, int n_fg, int n_stage, int K,
                      int n_tblk, float qscale_n, float qscale_d) {
    using PR = F16x2;
    using E8 = PR::v8;
    using std::integral_constant;
    __shared__ __attribute__((aligned(16))) unsigned char smem[LNA_RING_UNITS * 1024];
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
    const unsigned wbase = lds0 + 1024 * wf;                            // unit 4 i + w: 1024 w past unit 4 i (no wrap: a ring is whole stages)
    // fragment reads: every unit is 16 rows (frames) x 64 bytes, lane (r16, q) takes 16 bytes; A units come in pairs
    // 2 mt + h, B units in fours 4 x + f
    const unsigned lane_off = lds0 + r16 * (K1_BA * 2) + ((q ^ pl_swizzle(r16)) << 4);
    unsigned       lane_a[3], lane_b[3];
    unit_ring_windows(lane_off + 1024 * wh, lane_off + 1024 * wf, lane_a, lane_b);
    using I0 = integral_constant<int, 0>;
    using I1 = integral_constant<int, 1>;
    using I2 = integral_constant<int, 2>;

    if (mb == 0) {
        // =============================== role A: node rows + D' rows 0..159 ===============================
        // waves 0-3: ten source streams, instruction i = unit 4 i + w of every stage.  i = 0..5: block i = 2 c + p of
        // frame group w; units 24..29: the node table's KiB 3 h + mt (hi piece) for unit x = 2 mt + h; units 30..39:
        // D' unit x.  Instruction 7 is a node unit in wavefronts 0, 1 and a D' unit in wavefronts 2, 3.
        const unsigned char* src[LNA_DMA];
        unsigned             inc7;
#pragma unroll
        for (int i = 0; i < 6; ++i) src[i] = pl0 + 1024 * i;
#pragma unroll
        for (int i = 6; i < LNA_DMA; ++i) {
            const int u = 4 * i + wf;
            if (u < LNA_D_U0) {
                const int x = u - LNA_NODE_U0;
                src[i] = reinterpret_cast<const unsigned char*>(Pn) + 1024 * (LRN_NODE_MT * (x & 1) + (x >> 1));
            } else {
                src[i] = reinterpret_cast<const unsigned char*>(Dp) + 1024 * (u - LNA_D_U0);
            }
        }
        inc7 = 4 * 7 + wf < LNA_D_U0 ? LN_NODE_STAGE_BYTES : LRN_A_UNITS * 1024;
        auto dma = [&](auto s4_c, auto i_c) __attribute__((always_inline)) {
            constexpr int      S4 = decltype(s4_c)::value, I = decltype(i_c)::value;
            constexpr unsigned OFF = a_unit_off(S4, 4 * I);
            if constexpr (I < 6) {
                lds_dma16_at<OFF, (I & 1) != 0>(src[I], dma_voff, wbase);     // the lo piece is this role's alone: non-temporal
                src[I] += PL_STAGE_BYTES;
            } else if constexpr (I == 6) {
                lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);
                src[I] += LN_NODE_STAGE_BYTES;
            } else if constexpr (I == 7) {
                lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);
                src[I] += inc7;
            } else {
                lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);
                src[I] += LRN_A_UNITS * 1024;
            }
        };
        auto dma_stage = [&](auto s4_c) __attribute__((always_inline)) {
            [&]<int... Is>(std::integer_sequence<int, Is...>) __attribute__((always_inline)) { (dma(s4_c, integral_constant<int, Is>{}), ...); }(
                std::make_integer_sequence<int, LNA_DMA>{});
        };

        // A fragments in two sets, [stage parity]: a stage reads the next one's into the other set while it multiplies
        // (k1_lowrank_fold.hip).  B fragments are read again in place.
        E8    a[2][LRN_NODE_MT];                       // node A fragments (hi piece) [parity][row tile]
        E8    ad[2][LRN_A_MT];                         // D' A fragments [parity][row tile]
        E8    bb[3][2];                                // B fragments [component][piece]
        f32x4 hi[LRN_NODE_MT][3], lo[LRN_NODE_MT][3], accd[LRN_A_MT][3];
        auto  read_a = [&](auto s_c, auto mt_c) __attribute__((always_inline)) {
            constexpr int S = decltype(s_c)::value, MTI = decltype(mt_c)::value;
            a[S & 1][MTI] = lds_frag(lane_a, a_unit_off(S, LNA_NODE_U0 + 2 * MTI));
        };
        auto read_ad = [&](auto s_c, auto mt_c) __attribute__((always_inline)) {
            constexpr int S = decltype(s_c)::value, MTI = decltype(mt_c)::value;
            ad[S & 1][MTI] = lds_frag(lane_a, a_unit_off(S, LNA_D_U0 + 2 * MTI));
        };
        auto read_b = [&](auto s_c, auto c_c, auto p_c) __attribute__((always_inline)) {
            constexpr int S = decltype(s_c)::value, CC = decltype(c_c)::value, P = decltype(p_c)::value;
            bb[CC][P] = lds_frag(lane_b, a_unit_off(S, 4 * (2 * CC + P)));
        };
        auto each_node = [&](auto&& f) __attribute__((always_inline)) {
            [&]<int... Ms>(std::integer_sequence<int, Ms...>) __attribute__((always_inline)) { (f(integral_constant<int, Ms>{}), ...); }(
                std::make_integer_sequence<int, LRN_NODE_MT>{});
        };
        auto each_d = [&](auto&& f) __attribute__((always_inline)) {
            [&]<int... Ms>(std::integer_sequence<int, Ms...>) __attribute__((always_inline)) { (f(integral_constant<int, Ms>{}), ...); }(
                std::make_integer_sequence<int, LRN_A_MT>{});
        };
        static_assert(LNA_FOLD % 2 == 0, "the fragment sets alternate with the stage");
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int mt = 0; mt < LRN_NODE_MT; ++mt) {
                hi[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
                lo[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int mt = 0; mt < LRN_A_MT; ++mt) accd[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

        // ---- prologue: stages 0, 1 and 2; every fragment of stage 0 --------------------------------------------
        if (wh == 0) {
            dma_stage(I0{});
            dma_stage(I1{});
            dma_stage(I2{});
        }
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(LNA_DMA) : "memory");      // stages 0 and 1 landed
        each_node([&](auto mt_c) __attribute__((always_inline)) { read_a(I0{}, mt_c); });
        read_b(I0{}, I0{}, I1{});
        read_b(I0{}, I0{}, I0{});
        each_d([&](auto mt_c) __attribute__((always_inline)) { read_ad(I0{}, mt_c); });
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
            using SN = integral_constant<int, (S + 1) % LNA_FOLD>;
            using S3 = integral_constant<int, (S + 3) % LNA_FOLD>;
            if (wh == 0) dma_stage(S3{});                                  // into stage s-1's units, which are free
            auto comp = [&](auto c_c) __attribute__((always_inline)) {
                constexpr int CC = decltype(c_c)::value;
                f32x4         ch[LRN_NODE_MT];
                each_node([&](auto mt_c) __attribute__((always_inline)) {
                    constexpr int MTI = decltype(mt_c)::value;
                    ch[MTI] = PR::mma(a[PAR][MTI], bb[CC][1], restart ? f32x4{0.f, 0.f, 0.f, 0.f} : hi[MTI][CC]);
                });
                read_b(SN{}, c_c, I1{});
                if constexpr (CC == 0) each_node([&](auto mt_c) __attribute__((always_inline)) { read_a(SN{}, mt_c); });
                if constexpr (CC == 1) each_d([&](auto mt_c) __attribute__((always_inline)) { read_ad(SN{}, mt_c); });
                __builtin_amdgcn_sched_barrier(0);
                each_d([&](auto mt_c) __attribute__((always_inline)) {
                    constexpr int MTI = decltype(mt_c)::value;
                    accd[MTI][CC] = PR::mma(ad[PAR][MTI], bb[CC][0], accd[MTI][CC]);
                });
                each_node([&](auto mt_c) __attribute__((always_inline)) {
                    constexpr int MTI = decltype(mt_c)::value;
                    hi[MTI][CC] = PR::mma(a[PAR][MTI], bb[CC][0], ch[MTI]);
                });
                read_b(SN{}, c_c, I0{});
                __builtin_amdgcn_sched_barrier(0);
            };
            comp(I0{});
            comp(I1{});
            comp(I2{});
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(LNA_DMA) : "memory");     // stages s+1 and s+2 landed
        };
        // k1_chain_loop's chains: up to LNA_FOLD stages from zero, folded into lo
        for (; left > 0; left -= LNA_FOLD) {
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) __attribute__((always_inline)) { (stage(integral_constant<int, Ss>{}), ...); }(
                std::make_integer_sequence<int, LNA_FOLD>{});
            k1_fold(lo, hi);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // nothing in flight when LDS is handed on

        // ---- epilogue: the lane's coordinates are taken afresh (k1_planes_diff.hip)
        const int     lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int     r16_e = lane_e & 15, q_e = lane_e >> 4;
        const int64_t t = (int64_t)tb * LN_T_BLK + wf * 16 + r16_e;
        k1_store_q(Qn, lo, wh * LOWRANK_NODES_48, q_e, t, T, LOWRANK_NODES_48, T, qscale_n);
        k1_store_q(Q, accd, wh * (LRN_A_ROWS / 2), q_e, t, T, K, q_stride, qscale_d);
    } else {
        // =============================== role B: D' rows 160..511 ===============================
        // waves 0-3: nine source streams, the ninth in wavefronts 0 and 1 only.  i = 0..2: hi piece of component i of
        // frame group w; i = 3..8: D' unit w + 4 (i - 3)
        const unsigned char* src[LNB_DMA];
#pragma unroll
        for (int i = 0; i < 3; ++i) src[i] = pl0 + 1024 * (2 * i);
        const unsigned char* d0 = reinterpret_cast<const unsigned char*>(Dp) + lrn_b_first_unit(n_stage) * 1024;
#pragma unroll
        for (int i = 3; i < LNB_DMA; ++i) src[i] = d0 + 1024 * (wf + 4 * (i - 3));
        const bool ninth = wf < LNB_LAST;                                    // (uniform) units 32, 33 of a stage
        auto dma = [&](auto s4_c, auto i_c) __attribute__((always_inline)) {
            constexpr int      S4 = decltype(s4_c)::value, I = decltype(i_c)::value;
            constexpr unsigned OFF = b_unit_off(S4, 4 * I);
            if constexpr (I == LNB_DMA - 1) {
                if (ninth) {
                    lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);
                    src[I] += LRN_B_UNITS * 1024;
                }
            } else {
                lds_dma16_at<OFF, false>(src[I], dma_voff, wbase);      // the hi plane with the default policy: the sibling's hit
                src[I] += I < 3 ? PL_STAGE_BYTES : LRN_B_UNITS * 1024;
            }
        };
        auto dma_stage = [&](auto s4_c) __attribute__((always_inline)) {
            [&]<int... Is>(std::integer_sequence<int, Is...>) __attribute__((always_inline)) { (dma(s4_c, integral_constant<int, Is>{}), ...); }(
                std::make_integer_sequence<int, LNB_DMA>{});
        };
        // all but the last stage's instructions have completed: nine in wavefronts 0 and 1, eight in 2 and 3 (4-7 issue none)
        auto landed = [&]() __attribute__((always_inline)) {
            if (ninth)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LNB_DMA) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LNB_DMA - 1) : "memory");
            asm volatile("s_barrier" ::: "memory");
        };

        E8    a[4];                                    // A fragments of consecutive row tiles, read two ahead (lnb_slot)
        E8    bf[3];                                   // hi B fragments of the stage in work
        f32x4 acc[LRN_B_MT][3];
        auto read_a = [&](auto s4_c, auto mt_c) __attribute__((always_inline)) {
            constexpr int S4 = decltype(s4_c)::value, MTI = decltype(mt_c)::value;
            a[lnb_slot(S4, MTI)] = lds_frag(lane_a, b_unit_off(S4, LNB_D_U0 + 2 * MTI));
        };
        auto read_b = [&](auto s4_c, auto c_c) __attribute__((always_inline)) {
            constexpr int S4 = decltype(s4_c)::value, CC = decltype(c_c)::value;
            bf[CC] = lds_frag(lane_b, b_unit_off(S4, 4 * CC));
        };
#pragma unroll
        for (int mt = 0; mt < LRN_B_MT; ++mt)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[mt][c] = f32x4{0.f, 0.f, 0.f, 0.f};

        // ---- prologue: stages 0, 1 and 2 ------------------------------------------------------------------------
        if (wh == 0) {
            dma_stage(I0{});
            dma_stage(I1{});
            dma_stage(I2{});
        }
        landed();                                                          // stages 0 and 1 landed
        read_b(I0{}, I0{});
        read_b(I0{}, I1{});
        read_b(I0{}, I2{});
        read_a(I0{}, I0{});
        read_a(I0{}, I1{});

        int  left = n_stage;
        auto stage = [&](auto s4_c) __attribute__((always_inline)) {
            constexpr int S4 = decltype(s4_c)::value;
            if (left <= S4) return;                                        // past the group's last stage
            using SN = integral_constant<int, (S4 + 1) % LN_PERIOD>;
            using S3 = integral_constant<int, (S4 + 3) % LN_PERIOD>;
            if (wh == 0) dma_stage(S3{});                                  // into stage s-1's units, which are free
            auto tile = [&](auto mt_c) __attribute__((always_inline)) {
                constexpr int MTI = decltype(mt_c)::value;
                if constexpr (MTI + 2 < LRN_B_MT)
                    read_a(s4_c, integral_constant<int, MTI + 2>{});
                else
                    read_a(SN{}, integral_constant<int, MTI + 2 - LRN_B_MT>{});
                auto comp = [&](auto c_c) __attribute__((always_inline)) {
                    constexpr int CC = decltype(c_c)::value;
                    acc[MTI][CC] = PR::mma(a[lnb_slot(S4, MTI)], bf[CC], acc[MTI][CC]);
                    if constexpr (MTI == LRN_B_MT - 1) read_b(SN{}, c_c);  // behind the component's last use in this stage
                };
                comp(I0{});
                comp(I1{});
                comp(I2{});
                __builtin_amdgcn_sched_barrier(0);
            };
            [&]<int... Ms>(std::integer_sequence<int, Ms...>) __attribute__((always_inline)) { (tile(integral_constant<int, Ms>{}), ...); }(
                std::make_integer_sequence<int, LRN_B_MT>{});
            // what this stage read from its own units has been consumed above; reads in flight come from stage s+1
            landed();                                                      // stages s+1 and s+2 landed
        };
        for (; left > 0; left -= LN_PERIOD)
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) __attribute__((always_inline)) { (stage(integral_constant<int, Ss>{}), ...); }(
                std::make_integer_sequence<int, LN_PERIOD>{});
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

        const int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int r16_e = lane_e & 15, q_e = lane_e >> 4;
        k1_store_q(Q, acc, wh * (16 * LRN_B_MT) + LRN_A_ROWS, q_e, (int64_t)tb * LN_T_BLK + wf * 16 + r16_e, T, K, q_stride, qscale_d);
    }
}

// d_planes: the group's planes from its first frame group on; d_nodes: the 48-node table (one 128-row block of the
// phase-table image, rows 96..127 padding; its hi piece alone is read); d_diff: the D' image in the 48-node layout
// (pd16_n48_index), one 512-row block; d_qn: (48, 3, g.T) node projections; dscale: the power of two the image was
// multiplied by (the 48-node plan's dscale_fold)
int launch_k1_lowrank_n48(psa_ctx* c, const void* d_planes, const void* d_nodes, const void* d_diff, float2* d_qn, float2* d_q,
                          const ProjGeom& g, int64_t n_fg, float dscale) {
    PSA_REQUIRE(g.M_pad_d == LRN_ROWS && 2 * g.K <= LRN_ROWS && g.K > 0, "48-node pair launch: one 512-row D block only");
    PSA_REQUIRE(g.A_pad % (2 * K1_BA) == 0 && g.A_pad > 0, "48-node pair launch needs the atom axis padded to %d", 2 * K1_BA);
    PSA_REQUIRE(g.vscale > 0.f && dscale > 0.f && n_fg * 16 >= g.T, "planes do not cover the launch");
    ProjGeom g2 = g;
    g2.M_pad = 2 * LRN_ROWS;                                             // two roles per frame tile
    K1Grid gr;
    PSA_TRY(k1_grid(g2, LRN_ROWS, LN_T_BLK, gr));
    PSA_REQUIRE(gr.n_mblk == 2 && gr.n_tblk < (1 << 29) && n_fg < (1ll << 31), "projection grid too large");
    const float qscale_n = 1.f / (g.vscale * F16x2::P_SCALE) * g.wscale;      // powers of two: exact (launch_planes_family)
    const float qscale_d = 1.f / (g.vscale * dscale) * g.wscale;
    hipLaunchKernelGGL(k1_lowrank_n48_kernel, dim3(gr.blocks), dim3(512), 0, c->stream, (const _Float16*)d_planes,
                       (const _Float16*)d_nodes, (const _Float16*)d_diff, d_qn, d_q, g.T, g.q_stride, (int)n_fg, g.A_pad / K1_BA, g.K,
                       gr.n_tblk, qscale_n, qscale_d);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
