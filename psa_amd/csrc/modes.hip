// Mode-projected SED, plain and Welch-averaged (psa_sed_modes, psa_sed_modes_welch; definition: include/psa_hip.h, host
// side: api_modes.hip): one fused pass "contract + modulus" over the stacked transforms of the B basis-site groups, summed
// over the segments of its (k, w),
//
//     Phi[w,k,nu] = sum_s scale | sum_{b,c} conj(eig[k,nu,b,c]) F_{b,s}[k,c,w] |^2
//
// (psa_sed_modes: one segment of T frames, scale = 1/T^2).
// Work split: a workgroup of four wavefronts takes MODES_TK = 4 neighbouring k-vectors (one per wavefront) x
// MODES_TW = 64 frequencies (one per lane).  A lane walks the n = 3B rows of its (k, w) once per pass and segment --
// 8-byte loads, 512 contiguous bytes per wavefront and row -- and keeps MT complex accumulators (MT modes per pass, 8..32,
// chosen per M by modes_tile: any M is served, a longer M by further passes over rows that are then in L2; nothing of one
// w is ever held in registers beyond the MT accumulators, so B is free).  The coefficients of a wavefront's k-vector
// are the same for all its lanes: they are read through uniform (scalar) loads from a table the host packed as
// conj(eig), zero padded to whole passes, [k][pass][n][MT].  Arithmetic: float32 FMA chains in the order of n -- real and
// imaginary part of an accumulator side by side in a register pair, so that each of the two products of a complex
// multiply-add is one packed FMA with the coefficient as a scalar operand -- then |.|^2 as one product and one FMA,
// times the scale (a power-of-two scaling of eig therefore scales the result exactly).
// Hand-over: the result wants (w, k, nu) with nu fastest, a lane holds one w -- stored directly that would be 4-byte
// stores a whole row of the result apart.  The (w, k, nu) tile therefore goes through LDS (row stride 4 MT + 1
// floats: the column writes of the 64 lanes fall into 64 different banks) and leaves as runs of 4 MT consecutive
// floats per frequency (16 M bytes when M fits one pass), consecutive lanes on consecutive addresses.
// Two instantiations per tile.  SUM = false serves one segment that starts a sum (all of psa_sed_modes): the term goes
// straight into the tile.  SUM = true has the segment loop inside the pass loop, MT fresh accumulators per segment, and
// keeps the running sum over the segments in the tile, not in MT further registers: the MT = 32 kernel holds 64
// accumulator registers and SUM = false is at 86 of the 128 that four wavefronts per SIMD allow -- another 32 live across
// the row walk would leave the loads of the walk no room.  The tile is there anyway for the hand-over, and the element
// [w][k, nu] is read and written by the same lane for every segment: no barrier inside the segment loop, the 64 lanes of a
// read-modify-write fall into 64 different banks, 2 MT LDS accesses per segment against 12 B MT packed FMAs.  Even so it
// costs registers and occupancy (tests/test_modes_resources.py), which is why one segment is not served by it.
// A launch covers segments [s0, s0 + ns) of a longer sum.  With `first` the running sum starts at 0, otherwise at the
// value already in `out`, fetched with the hand-over's own coalesced pattern.  Each term is rounded to float32
// (|Q|^2 scale) and then added: the sum over the segments is one float32 chain in ascending s however the segments
// are split over launches (0 + x is exact), so a split run gives the bits of a single launch, and one segment those of
// SUM = false.  Lanes beyond L read nothing from S or out and write nothing to out.
#include "psa_ctx.h"

namespace psa {

constexpr int MODES_TW = 64;   // frequencies per workgroup tile: one per lane
constexpr int MODES_TK = 4;    // k-vectors per workgroup tile: one per wavefront

typedef float f32x2 __attribute__((ext_vector_type(2)));   // (re, im): one v_pk_fma_f32 per product

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

// The hand-over walk of pass p: move(tile element, its element of out) for every element of the workgroup's tile that
// lies inside the result, 4 MT consecutive floats of out per frequency on consecutive lanes
template <int MT, class Move>
__device__ __forceinline__ void mode_hand_over(float (&tile)[MODES_TW][MODES_TK * MT + 1], float* __restrict__ out, int p, int t0,
                                               int L, int nk, int M, int64_t out_pitch, Move move) {
    for (int item = threadIdx.x; item < MODES_TW * MODES_TK * MT; item += 256) {
        const int tl = item / (MODES_TK * MT), x = item - tl * (MODES_TK * MT);
        const int kl = x / MT, j = x - kl * MT;
        const int kk = blockIdx.y * MODES_TK + kl, m = p * MT + j;
        const int tt = t0 + tl;
        if (tt < L && kk < nk && m < M) move(tile[tl][x], out[(size_t)tt * out_pitch + (size_t)kk * M + m]);
    }
}

// S: (B, nk, 3, ns, L) complex64, the unscaled transforms of ns segments of one block of nk k-vectors (SUM = false: ns is
// 1 and `first` set, neither is read); coef: the block's part of the packed table [k][pass][3B][MT]; out: the block's first
// column of the (L, K, M) float32 result, out_pitch = K M floats from one frequency to the next
template <int MT, bool SUM>
__global__ void __launch_bounds__(256)
mode_power_kernel(const float2* __restrict__ S, const float2* __restrict__ coef, float* __restrict__ out, int L, int ns, int nk,
                  int B, int M, int n_pass, int64_t out_pitch, float scale, int first) {
    __shared__ float tile[MODES_TW][MODES_TK * MT + 1];
    const int     lane = threadIdx.x & 63;
    const int     wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int     t0 = blockIdx.x * MODES_TW, t = t0 + lane;
    const int     k = blockIdx.y * MODES_TK + wave;            // the same for the whole wavefront
    const bool    live = k < nk, in_range = t < L;
    const int     n_seg = SUM ? ns : 1;
    const size_t  stride_c = (size_t)n_seg * (size_t)L, stride_b = (size_t)nk * 3 * stride_c;
    for (int p = 0; p < n_pass; ++p) {
        if (SUM && !first) {                                   // (uniform) the sum so far, as the hand-over wrote it
            mode_hand_over<MT>(tile, out, p, t0, L, nk, M, out_pitch, [](float& in_tile, const float& in_out) { in_tile = in_out; });
            __syncthreads();
        }
        if (live) {
            float* sum = &tile[lane][wave * MT];               // this lane's MT running sums: no other lane touches them
            if (SUM && first) {
#pragma unroll
                for (int j = 0; j < MT; ++j) sum[j] = 0.f;
            }
            const float2* cf = coef + ((size_t)k * n_pass + p) * (size_t)(3 * B) * MT;   // uniform: scalar loads
            const float2* rows = S + (size_t)k * 3 * stride_c + t;       // this lane's element of segment 0, group 0, x
            for (int s = 0; s < n_seg; ++s, rows += L) {
                f32x2 acc[MT];
#pragma unroll
                for (int j = 0; j < MT; ++j) acc[j] = f32x2{0.f, 0.f};
                // acc[j] += sum_{b,c} cf[3 b + c][j] * rows[b stride_b + c stride_c], in the order of n = 3 b + c; a lane
                // out of range reads nothing and adds zeros
                for (int b = 0; b < B; ++b) {
                    const float2* row = rows + (size_t)b * stride_b;
                    float2        q[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[c] = in_range ? row[(size_t)c * stride_c] : make_float2(0.f, 0.f);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const f32x2   xy = {q[c].x, q[c].y}, yx = {-q[c].y, q[c].x};
                        const float2* e = cf + (size_t)(3 * b + c) * MT;
#pragma unroll
                        for (int j = 0; j < MT; ++j) {              // (p + iq)(x + iy), p + iq = conj(eig)
                            const float2 pq = e[j];
                            acc[j] = __builtin_elementwise_fma(f32x2{pq.x, pq.x}, xy, acc[j]);
                            acc[j] = __builtin_elementwise_fma(f32x2{pq.y, pq.y}, yx, acc[j]);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const float term = fmaf(acc[j].x, acc[j].x, acc[j].y * acc[j].y) * scale;
                    if (SUM) sum[j] += term;
                    else sum[j] = term;
                }
            }
        }
        __syncthreads();
        mode_hand_over<MT>(tile, out, p, t0, L, nk, M, out_pitch, [](const float& in_tile, float& in_out) { in_out = in_tile; });
        __syncthreads();
    }
}

int launch_mode_power(psa_ctx* c, const float2* d_S, const float2* d_coef, float* d_out, int64_t L, int64_t ns, int64_t nk,
                      int64_t B, int64_t M, int MT, int64_t K_pitch, int64_t k_col0, float scale, bool first) {
    if (nk == 0 || L == 0 || ns == 0) return PSA_OK;
    const int64_t gx = (L + MODES_TW - 1) / MODES_TW, gy = (nk + MODES_TK - 1) / MODES_TK;
    PSA_REQUIRE(L <= (1ll << 31) - MODES_TW && gy <= 65535 && ns < (1ll << 31) && B >= 1 && 3 * B < (1ll << 30) && M >= 1 && M < (1ll << 30),
                "mode contraction: block of %lld k-vectors x %lld segments of %lld frames, B = %lld, M = %lld is out of range",
                (long long)nk, (long long)ns, (long long)L, (long long)B, (long long)M);
    const int  n_pass = (int)((M + MT - 1) / MT);
    const bool sum = !(ns == 1 && first);                      // one segment that starts a sum needs no running sum
    const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
    decltype(&mode_power_kernel<8, false>) kernel = nullptr;
#define PSA_MODES_KERNEL(mt) \
    case mt: kernel = sum ? mode_power_kernel<mt, true> : mode_power_kernel<mt, false>; break
    switch (MT) {
        PSA_MODES_KERNEL(8);
        PSA_MODES_KERNEL(16);
        PSA_MODES_KERNEL(24);
        PSA_MODES_KERNEL(32);
        default: PSA_REQUIRE(false, "mode contraction: no kernel for %d modes per pass", MT);
    }
#undef PSA_MODES_KERNEL
    hipLaunchKernelGGL(kernel, grid, block, 0, c->stream, d_S, d_coef, d_out + k_col0 * M, (int)L, (int)ns, (int)nk, (int)B, (int)M,
                       n_pass, K_pitch * M, scale, first ? 1 : 0);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
