// Mode-projected SED (psa_sed_modes; definition: include/psa_hip.h, host side: api_modes.hip): one fused pass
// "contract + modulus" over the stacked spectra of the B basis-site groups,
//
//     Phi[w,k,nu] = | (1/T) sum_{b,c} conj(eig[k,nu,b,c]) S_b[k,c,w] |^2 .
//
// Work split: a workgroup of four wavefronts takes MODES_TK = 4 neighbouring k-vectors (one per wavefront) x
// MODES_TW = 64 frequencies (one per lane).  A lane walks the n = 3B rows of its (k, w) once per pass -- 8-byte loads,
// 512 contiguous bytes per wavefront and row -- and keeps MT complex accumulators (MT modes per pass, 8..32, chosen
// per M by modes_tile: any M is served, a longer M by further passes over rows that are then in L2; nothing of one w
// is ever held in registers beyond the MT accumulators, so B is free).  The coefficients of a wavefront's k-vector
// are the same for all its lanes: they are read through uniform (scalar) loads from a table the host packed as
// conj(eig), zero padded to whole passes, [k][pass][n][MT].  Arithmetic: float32 FMA chains in the order of n -- real and
// imaginary part of an accumulator side by side in a register pair, so that each of the two products of a complex
// multiply-add is one packed FMA with the coefficient as a scalar operand -- then |.|^2 as one product and one FMA,
// times 1/T^2 (a power-of-two scaling of eig therefore scales the result exactly).
// Hand-over: the result wants (w, k, nu) with nu fastest, a lane holds one w -- stored directly that would be 4-byte
// stores a whole row of the result apart.  The (w, k, nu) tile therefore goes through LDS (row stride 4 MT + 1
// floats: the column writes of the 64 lanes fall into 64 different banks) and leaves as runs of 4 MT consecutive
// floats per frequency (16 M bytes when M fits one pass), consecutive lanes on consecutive addresses.
// The tile constants and the row walk are shared with the segment-averaging sibling (modes_welch.hip): modes_rows.h.
#include "modes_rows.h"
#include "psa_ctx.h"

namespace psa {

// Modes per pass for M mode vectors.  A pass costs its rows' loads once (about 8 FMA-equivalents per row and lane)
// plus 4 MT FMAs per row, padding included: the cheapest of 8, 16, 24, 32; ties go to the wider tile.
int modes_tile(int64_t M) {
    int     best = 8;
    int64_t best_cost = -1;
    for (int mt : {8, 16, 24, 32}) {
        const int64_t cost = (M + mt - 1) / mt * (4 * mt + 8);
        if (best_cost < 0 || cost <= best_cost) best = mt, best_cost = cost;
    }
    return best;
}

// S: (B, nk, 3, T) complex64, the unscaled spectra of one block of nk k-vectors; coef: the block's part of the
// packed table; out: (T, K_pitch, M) float32, the block's columns starting at k_col0; inv_n2: 1/T^2 (1 when the
// spectra come scaled)
template <int MT>
__global__ void __launch_bounds__(256)
mode_power_kernel(const float2* __restrict__ S, const float2* __restrict__ coef, float* __restrict__ out, int64_t T, int nk,
                  int B, int M, int n_pass, int64_t K_pitch, int64_t k_col0, float inv_n2) {
    __shared__ float tile[MODES_TW][MODES_TK * MT + 1];
    const int     lane = threadIdx.x & 63;
    const int     wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t t0 = (int64_t)blockIdx.x * MODES_TW, t = t0 + lane;
    const int     k = blockIdx.y * MODES_TK + wave;            // the same for the whole wavefront
    const bool    live = k < nk;
    const int     n3 = 3 * B;
    for (int p = 0; p < n_pass; ++p) {
        if (live) {
            f32x2 acc[MT];
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[j] = f32x2{0.f, 0.f};
            const float2* cf = coef + ((size_t)k * n_pass + p) * (size_t)n3 * MT;
            mode_rows<MT>(acc, S + (size_t)k * 3 * (size_t)T + t, (size_t)nk * 3 * (size_t)T, (size_t)T, cf, B, t < T);
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                tile[lane][wave * MT + j] = fmaf(acc[j].x, acc[j].x, acc[j].y * acc[j].y) * inv_n2;
            }
        }
        __syncthreads();
        for (int item = threadIdx.x; item < MODES_TW * MODES_TK * MT; item += 256) {
            const int     tl = item / (MODES_TK * MT), x = item - tl * (MODES_TK * MT);
            const int     kl = x / MT, j = x - kl * MT;
            const int     kk = blockIdx.y * MODES_TK + kl, m = p * MT + j;
            const int64_t tt = t0 + tl;
            if (tt < T && kk < nk && m < M) out[(tt * K_pitch + k_col0 + kk) * M + m] = tile[tl][x];
        }
        __syncthreads();
    }
}

int launch_mode_power(psa_ctx* c, const float2* d_S, const float2* d_coef, float* d_out, int64_t T, int64_t nk, int64_t B,
                      int64_t M, int MT, int64_t K_pitch, int64_t k_col0, float inv_n2) {
    if (nk == 0 || T == 0) return PSA_OK;
    const int64_t gx = (T + MODES_TW - 1) / MODES_TW, gy = (nk + MODES_TK - 1) / MODES_TK;
    PSA_REQUIRE(gx < (1ll << 31) && gy <= 65535 && B >= 1 && 3 * B < (1ll << 30) && M >= 1 && M < (1ll << 30),
                "mode contraction: block of %lld k-vectors x %lld frames, B = %lld, M = %lld is out of range", (long long)nk,
                (long long)T, (long long)B, (long long)M);
    const int  n_pass = (int)((M + MT - 1) / MT);
    const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
#define PSA_MODES_LAUNCH(mt)                                                                                              \
    hipLaunchKernelGGL(mode_power_kernel<mt>, grid, block, 0, c->stream, d_S, d_coef, d_out, T, (int)nk, (int)B, (int)M, \
                       n_pass, K_pitch, k_col0, inv_n2)
    switch (MT) {
        case 8: PSA_MODES_LAUNCH(8); break;
        case 16: PSA_MODES_LAUNCH(16); break;
        case 24: PSA_MODES_LAUNCH(24); break;
        case 32: PSA_MODES_LAUNCH(32); break;
        default: PSA_REQUIRE(false, "mode contraction: no kernel for %d modes per pass", MT);
    }
#undef PSA_MODES_LAUNCH
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
