// K1 low-rank route for k-paths: the combine q += C Qn, the route's third pass (the node rows, the D pass and the
// tables are in k1_planes_diff.hip).  C[j, l] = phi[j] L[j, l] comes taken apart from the plan (api_lowrank.hip): L the
// real Lagrange weights, phi the row's phase, float32 each.  lowrank_combine_r_kernel sums the nodes with L and applies
// phi once per element.
#include "k1_f16.h"

namespace psa {

// ---------------------------------------------------------------------------------------------
// q[j, c, t] += phi[j] sum_l L[j, l] Qn[l, c, t]: per element, l in order, one v_pk_fma_f32 (two IEEE fmas)
//     (sr, si) = fma((L, L), (Qr, Qi), (sr, si))
// and then, once, the fixed sequence
//     pr = phi_r * sr;  pr = fma(-phi_i, si, pr)
//     pi = phi_r * si;  pi = fma( phi_i, sr, pi)
//     o  = o + (pr, pi)
// -- one packed FMA and four bytes of LDS per node and element, where a complex weight would take two and eight.  It is
// the arithmetic of every row whatever the launch holds besides it, so a list split over calls keeps its bits.  It is
// not a sum over (float)(phi L): (float)phi and (float)L are rounded apart.
// NODES = 64 or 48 (psa_set_k1_lowrank_nodes): the same chain over l = 0..NODES-1.
// A thread holds the 64 node values of one (c, t) in registers and walks every row j; the block stages L 64 rows at a
// time in LDS (16 KiB, and the 64 phases) and reads it back as broadcasts, one ds_read_b128 = four nodes of a row for
// the whole wavefront.  Rows go four at a time, four independent chains of one dependent packed FMA per node; the q
// values of a group of four rows are loaded two groups ahead of its sums.
// ---------------------------------------------------------------------------------------------
namespace {
// (sr, si) of four rows += L[l] Qn[l] for two nodes: w = (L[l], L[l + 1]) of the row, op_sel picks the half both lanes
// of the product take.  Node l of all four rows, then node l + 1: no result is read by the instruction after it.
__device__ __forceinline__ void rmac4(f32x2& s0, f32x2& s1, f32x2& s2, f32x2& s3, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 xa,
                                      f32x2 xb) {
    asm("v_pk_fma_f32 %0, %4, %8, %0 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %1, %5, %8, %1 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %2, %6, %8, %2 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %3, %7, %8, %3 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %0, %4, %9, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %1, %5, %9, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %2, %6, %9, %2 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %3, %7, %9, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]"
        : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(xa), "v"(xb));
}
// o + phi s, the sequence above
__device__ __forceinline__ float2 phase_add(float2 o, float2 ph, f32x2 s) {
    float pr = ph.x * s[0], pi = ph.x * s[1];
    pr = __builtin_fmaf(-ph.y, s[1], pr);
    pi = __builtin_fmaf(ph.y, s[0], pi);
    return make_float2(o.x + pr, o.y + pi);
}
}  // namespace

constexpr int COMBINE_R_JB = 64;
constexpr int COMBINE_R_PF = 2;            // groups of four rows whose q values are in flight ahead of the sums
template <int NODES>
__global__ void __launch_bounds__(256)
lowrank_combine_r_kernel(const float2* __restrict__ Qn, const float* __restrict__ Lm, const float2* __restrict__ phi,
                         float2* __restrict__ q, int64_t T, int64_t q_stride, int64_t qn_stride, int K) {
    __shared__ __attribute__((aligned(16))) f32x4 ls[COMBINE_R_JB * NODES / 4];   // 16 KiB at 64 nodes: rows j0.., four nodes per entry
    __shared__ float2 ps[COMBINE_R_JB];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int     c = blockIdx.y;
    const bool    live = t < T;
    const int64_t tl = live ? t : T - 1;                              // (past the end: loads in bounds, nothing stored)
    auto at = [&](int j) -> float2& { return q[((int64_t)j * 3 + c) * q_stride + tl]; };
    auto row = [&](int j) { return j < K ? j : K - 1; };               // past the last row the last one again
    // the q values of the next COMBINE_R_PF groups of four rows are in flight while a group is summed
    constexpr int PF = COMBINE_R_PF;
    float2        nx[PF][4];
#pragma unroll
    for (int d = 0; d < PF; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) nx[d][r] = at(row(4 * d + r));
    f32x2 v[NODES];
#pragma unroll
    for (int l = 0; l < NODES; ++l) {
        const float2 x = Qn[((int64_t)l * 3 + c) * qn_stride + tl];
        v[l] = f32x2{x.x, x.y};
    }
    const f32x4* l4 = reinterpret_cast<const f32x4*>(Lm);
    for (int j0 = 0; j0 < K; j0 += COMBINE_R_JB) {
        const int nj = K - j0 < COMBINE_R_JB ? K - j0 : COMBINE_R_JB;
        __syncthreads();                                                 // the previous rows are read
        for (int i = threadIdx.x; i < nj * NODES / 4; i += 256) ls[i] = l4[(size_t)j0 * (NODES / 4) + i];
        if (threadIdx.x < nj) ps[threadIdx.x] = phi[j0 + threadIdx.x];
        __syncthreads();
        if (!live) continue;                                             // (frames past the end only stage and meet the barriers)
        for (int j = 0; j < nj; j += 4) {
            int    jr[4];                                                // (past the stage's last row the last one again: computed, not stored)
            float2 ov[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                jr[r] = j + r < nj ? j + r : nj - 1;
                ov[r] = nx[0][r];
            }
#pragma unroll
            for (int d = 0; d + 1 < PF; ++d)
#pragma unroll
                for (int r = 0; r < 4; ++r) nx[d][r] = nx[d + 1][r];
#pragma unroll
            for (int r = 0; r < 4; ++r) nx[PF - 1][r] = at(row(j0 + j + 4 * PF + r));
            f32x2 s0 = {0.f, 0.f}, s1 = {0.f, 0.f}, s2 = {0.f, 0.f}, s3 = {0.f, 0.f};
            asm volatile("s_nop 0" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3));   // the zeros are VALU results read by a packed FMA
#pragma unroll
            for (int i = 0; i < NODES / 4; ++i) {
                const f32x4 w0 = ls[jr[0] * (NODES / 4) + i], w1 = ls[jr[1] * (NODES / 4) + i];
                const f32x4 w2 = ls[jr[2] * (NODES / 4) + i], w3 = ls[jr[3] * (NODES / 4) + i];
                rmac4(s0, s1, s2, s3, f32x2{w0[0], w0[1]}, f32x2{w1[0], w1[1]}, f32x2{w2[0], w2[1]}, f32x2{w3[0], w3[1]}, v[4 * i],
                      v[4 * i + 1]);
                rmac4(s0, s1, s2, s3, f32x2{w0[2], w0[3]}, f32x2{w1[2], w1[3]}, f32x2{w2[2], w2[3]}, f32x2{w3[2], w3[3]}, v[4 * i + 2],
                      v[4 * i + 3]);
            }
            asm volatile("s_nop 0" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3));   // ... and the sums are read by plain VALU
            const f32x2 s[4] = {s0, s1, s2, s3};
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (j + r < nj) at(j0 + j + r) = phase_add(ov[r], ps[j + r], s[r]);
        }
    }
}

// (the 64-node instantiation first: it stays the file's first kernel)
template __global__ void lowrank_combine_r_kernel<LOWRANK_NODES>(const float2*, const float*, const float2*, float2*, int64_t, int64_t, int64_t, int);
template __global__ void lowrank_combine_r_kernel<48>(const float2*, const float*, const float2*, float2*, int64_t, int64_t, int64_t, int);

int launch_lowrank_combine_r(psa_ctx* c, const float2* d_qn, const float* d_L, const float2* d_phi, float2* d_q, const ProjGeom& g,
                             int64_t qn_stride) {
    const int64_t nb = (g.T + 255) / 256;
    PSA_REQUIRE(nb < (1ll << 31) && g.K > 0, "combine grid too large");
    PSA_REQUIRE(g.lr_nodes == LOWRANK_NODES || g.lr_nodes == 48, "combine: 48 or 64 nodes");
    hipLaunchKernelGGL(g.lr_nodes == LOWRANK_NODES ? lowrank_combine_r_kernel<LOWRANK_NODES> : lowrank_combine_r_kernel<48>, dim3((unsigned)nb, 3),
                       dim3(256), 0, c->stream, d_qn, d_L, d_phi, d_q, g.T, g.q_stride, qn_stride, g.K);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
