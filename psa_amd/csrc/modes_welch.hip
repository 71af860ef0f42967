// Welch-averaged mode spectra (psa_sed_modes_welch; definition: include/psa_hip.h, host side: api_modes_welch.hip): the
// sibling of mode_power_kernel (modes.hip) that contracts and takes the modulus for every segment of its (k, w) and keeps
// the sum over the segments on chip,
//
//     Phi[w,k,nu] = sum_s scale | sum_{b,c} conj(eig[k,nu,b,c]) F_{b,s}[k,c,w] |^2 .
//
// Work split, coefficient table, arithmetic of one segment and hand-over are the parent's (modes_rows.h holds the shared
// row walk): four k-vectors per workgroup, one per wavefront; 64 frequencies, one per lane; MT modes per pass, further
// passes for M > MT; the segment loop sits inside the pass loop, MT fresh complex accumulators per segment.
// The running sum over the segments lives in the workgroup's LDS tile, not in MT further registers: the MT = 32 kernel
// holds 64 accumulator registers and the parent is at 86 of the 128 that four wavefronts per SIMD allow -- another 32 live
// across the row walk would leave the loads of the walk no room.  The tile is there anyway for the hand-over, and the
// element [w][k, nu] is read and written by the same lane for every segment: no barrier inside the segment loop, the
// 64 lanes of a read-modify-write fall into 64 different banks (row stride 4 MT + 1), 2 MT LDS accesses per segment
// against 12 B MT packed FMAs.
// A launch covers segments [s0, s0 + ns) of a longer sum.  With `first` the running sum starts at 0, otherwise at the
// value already in `out`, fetched with the hand-over's own coalesced pattern.  Each term is rounded to float32
// (|Q|^2 scale) and then added: the sum over the segments is one float32 chain in ascending s however the segments
// are split over launches (0 + x is exact), so a split run gives the bits of a single launch.
// Lanes beyond L read nothing from S or out and write nothing to out.
#include "modes_rows.h"
#include "psa_ctx.h"

namespace psa {

// S: (B, nk, 3, ns, L) complex64, the unscaled transforms of ns segments of one block of nk k-vectors; coef: the block's
// part of the packed table [k][pass][3B][MT]; out: the block's first column of the (L, K, M) float32 result, out_pitch =
// K M floats from one frequency to the next
template <int MT>
__global__ void __launch_bounds__(256)
mode_welch_kernel(const float2* __restrict__ S, const float2* __restrict__ coef, float* __restrict__ out, int L, int ns, int nk,
                  int B, int M, int n_pass, int64_t out_pitch, float scale, int first) {
    __shared__ float tile[MODES_TW][MODES_TK * MT + 1];
    const int     lane = threadIdx.x & 63;
    const int     wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int     t0 = blockIdx.x * MODES_TW, t = t0 + lane;
    const int     k = blockIdx.y * MODES_TK + wave;            // the same for the whole wavefront
    const bool    live = k < nk;
    const int     n3 = 3 * B;
    const size_t  stride_c = (size_t)ns * (size_t)L, stride_b = (size_t)nk * 3 * stride_c;
    for (int p = 0; p < n_pass; ++p) {
        if (!first) {                                          // (uniform) the sum so far, as the hand-over wrote it
            for (int item = threadIdx.x; item < MODES_TW * MODES_TK * MT; item += 256) {
                const int     tl = item / (MODES_TK * MT), x = item - tl * (MODES_TK * MT);
                const int     kl = x / MT, j = x - kl * MT;
                const int     kk = blockIdx.y * MODES_TK + kl, m = p * MT + j;
                const int     tt = t0 + tl;
                if (tt < L && kk < nk && m < M) tile[tl][x] = out[(size_t)tt * out_pitch + (size_t)kk * M + m];
            }
            __syncthreads();
        }
        if (live) {
            float* sum = &tile[lane][wave * MT];               // this lane's MT running sums: no other lane touches them
            if (first) {
#pragma unroll
                for (int j = 0; j < MT; ++j) sum[j] = 0.f;
            }
            const float2* cf = coef + ((size_t)k * n_pass + p) * (size_t)n3 * MT;
            const float2* rows = S + (size_t)k * 3 * stride_c + t;       // this lane's element of segment 0, group 0, x
            for (int s = 0; s < ns; ++s, rows += L) {
                f32x2 acc[MT];
#pragma unroll
                for (int j = 0; j < MT; ++j) acc[j] = f32x2{0.f, 0.f};
                mode_rows<MT>(acc, rows, stride_b, stride_c, cf, B, t < L);
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const float term = fmaf(acc[j].x, acc[j].x, acc[j].y * acc[j].y) * scale;
                    sum[j] += term;
                }
            }
        }
        __syncthreads();
        for (int item = threadIdx.x; item < MODES_TW * MODES_TK * MT; item += 256) {
            const int     tl = item / (MODES_TK * MT), x = item - tl * (MODES_TK * MT);
            const int     kl = x / MT, j = x - kl * MT;
            const int     kk = blockIdx.y * MODES_TK + kl, m = p * MT + j;
            const int     tt = t0 + tl;
            if (tt < L && kk < nk && m < M) out[(size_t)tt * out_pitch + (size_t)kk * M + m] = tile[tl][x];
        }
        __syncthreads();
    }
}

int launch_mode_welch(psa_ctx* c, const float2* d_S, const float2* d_coef, float* d_out, int64_t L, int64_t ns, int64_t nk,
                      int64_t B, int64_t M, int MT, int64_t K_pitch, int64_t k_col0, float scale, bool first) {
    if (nk == 0 || L == 0 || ns == 0) return PSA_OK;
    const int64_t gx = (L + MODES_TW - 1) / MODES_TW, gy = (nk + MODES_TK - 1) / MODES_TK;
    PSA_REQUIRE(L <= (1ll << 31) - MODES_TW && gy <= 65535 && ns < (1ll << 31) && B >= 1 && 3 * B < (1ll << 30) && M >= 1 && M < (1ll << 30),
                "segment-averaged mode contraction: block of %lld k-vectors x %lld segments of %lld frames, B = %lld, M = %lld is "
                "out of range", (long long)nk, (long long)ns, (long long)L, (long long)B, (long long)M);
    const int  n_pass = (int)((M + MT - 1) / MT);
    const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
#define PSA_MODES_LAUNCH(mt)                                                                                               \
    hipLaunchKernelGGL(mode_welch_kernel<mt>, grid, block, 0, c->stream, d_S, d_coef, d_out + k_col0 * M, (int)L, (int)ns, (int)nk, \
                       (int)B, (int)M, n_pass, K_pitch * M, scale, first ? 1 : 0)
    switch (MT) {
        case 8: PSA_MODES_LAUNCH(8); break;
        case 16: PSA_MODES_LAUNCH(16); break;
        case 24: PSA_MODES_LAUNCH(24); break;
        case 32: PSA_MODES_LAUNCH(32); break;
        default: PSA_REQUIRE(false, "segment-averaged mode contraction: no kernel for %d modes per pass", MT);
    }
#undef PSA_MODES_LAUNCH
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
