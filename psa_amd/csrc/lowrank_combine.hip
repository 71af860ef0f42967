// K1 low-rank route for k-paths: the combine q += C Qn (the node rows, the D pass and the tables are in
// k1_planes_diff.hip, whose scalar lowrank_combine_kernel stays as the A/B arm: PSA_K1_COMBINE=0).
#include "k1_f16.h"

namespace psa {

// ---------------------------------------------------------------------------------------------
// q[j, c, t] += sum_l C[j, l] Qn[l, c, t], the arithmetic of lowrank_combine_kernel (k1_planes_diff.hip) bit for bit:
// per element, l in order, sr = fma(Cr, Qr, sr), sr = fma(-Ci, Qi, sr) and si = fma(Cr, Qi, si), si = fma(Ci, Qr, si),
// then o + s.  Each pair of those is one v_pk_fma_f32 (two IEEE fmas) on (sr, si), its operands picked by op_sel.
// A thread holds the 64 node values of one (c, t) in registers and walks every row j, two at a time (two independent
// chains); the block stages C 64 rows at a time in LDS and reads it back as broadcasts (one ds_read_b128 = two nodes
// of a row for the whole wavefront).
// ---------------------------------------------------------------------------------------------
namespace {
// (sr, si) of two rows += C[l] Qn[l]: A = (Cr, Ci) of the row, B = (Qr, Qi); first (Cr, Cr) x (Qr, Qi), then
// (-Ci, Ci) x (Qi, Qr).  The rows alternate, so no result is read by the instruction right after it.
__device__ __forceinline__ void cmac2(f32x2& s0, f32x2& s1, f32x2 w0, f32x2 w1, f32x2 x) {
    asm("v_pk_fma_f32 %0, %2, %4, %0 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %1, %3, %4, %1 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %0, %2, %4, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]\n\t"
        "v_pk_fma_f32 %1, %3, %4, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"
        : "+v"(s0), "+v"(s1)
        : "v"(w0), "v"(w1), "v"(x));
}
}  // namespace

constexpr int COMBINE_V_JB = 64;
__global__ void __launch_bounds__(256)
lowrank_combine_v_kernel(const float2* __restrict__ Qn, const float2* __restrict__ Cm, float2* __restrict__ q, int64_t T,
                         int64_t q_stride, int64_t qn_stride, int K) {
    __shared__ __attribute__((aligned(16))) f32x4 cs[COMBINE_V_JB * LOWRANK_NODES / 2];   // 32 KiB: rows j0.., two nodes per entry
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int     c = blockIdx.y;
    const bool    live = t < T;
    const int64_t tl = live ? t : T - 1;                              // (past the end: loads in bounds, nothing stored)
    f32x2         v[LOWRANK_NODES];
#pragma unroll
    for (int l = 0; l < LOWRANK_NODES; ++l) {
        const float2 x = Qn[((int64_t)l * 3 + c) * qn_stride + tl];
        v[l] = f32x2{x.x, x.y};
    }
    const f32x4* c4 = reinterpret_cast<const f32x4*>(Cm);
    for (int j0 = 0; j0 < K; j0 += COMBINE_V_JB) {
        const int nj = K - j0 < COMBINE_V_JB ? K - j0 : COMBINE_V_JB;
        __syncthreads();                                                 // the previous rows are read
        for (int i = threadIdx.x; i < nj * LOWRANK_NODES / 2; i += 256) cs[i] = c4[(size_t)j0 * (LOWRANK_NODES / 2) + i];
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < nj; j += 2) {
            const int    j1 = j + 1 < nj ? j + 1 : j;                   // an odd last row is computed twice, stored once
            float2&      o0 = q[((int64_t)(j0 + j) * 3 + c) * q_stride + t];
            float2&      o1 = q[((int64_t)(j0 + j1) * 3 + c) * q_stride + t];
            const float2 ov0 = o0, ov1 = o1;
            f32x2        s0 = {0.f, 0.f}, s1 = {0.f, 0.f};
            asm volatile("s_nop 0" : "+v"(s0), "+v"(s1));              // the zeros are VALU results read by a packed FMA
#pragma unroll
            for (int l2 = 0; l2 < LOWRANK_NODES / 2; ++l2) {
                const f32x4 w0 = cs[j * (LOWRANK_NODES / 2) + l2], w1 = cs[j1 * (LOWRANK_NODES / 2) + l2];
                cmac2(s0, s1, f32x2{w0[0], w0[1]}, f32x2{w1[0], w1[1]}, v[2 * l2]);
                cmac2(s0, s1, f32x2{w0[2], w0[3]}, f32x2{w1[2], w1[3]}, v[2 * l2 + 1]);
            }
            o0 = make_float2(ov0.x + s0[0], ov0.y + s0[1]);
            if (j1 != j) o1 = make_float2(ov1.x + s1[0], ov1.y + s1[1]);
        }
    }
}

int launch_lowrank_combine_v(psa_ctx* c, const float2* d_qn, const float2* d_C, float2* d_q, const ProjGeom& g, int64_t qn_stride) {
    const int64_t nb = (g.T + 255) / 256;
    PSA_REQUIRE(nb < (1ll << 31) && g.K > 0, "combine grid too large");
    hipLaunchKernelGGL(lowrank_combine_v_kernel, dim3((unsigned)nb, 3), dim3(256), 0, c->stream, d_qn, d_C, d_q, g.T, g.q_stride, qn_stride,
                       g.K);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
