// Frame-dependent projections for the dynamic structure factor and the current correlations (psa_dynamic_spectra;
// definition: include/psa_hip.h, host side: api_dynamic.hip):
//
//     q_0[k,t] = sum_a w_a exp(i k.r_a(t))              q_c[k,t] = sum_a w_a v_a,c(t) exp(i k.r_a(t))    c = 1, 2, 3
//
// The phase depends on the frame, so there is no phase table and nothing for the matrix cores: one sine and one cosine
// per (k-vector, atom, frame) unit and about thirty plain VALU instructions around them.  The kernel is VALU-bound; HBM
// traffic (24 N bytes per frame and block of k-vectors) is two orders of magnitude below the arithmetic.
//
// Work split.  A workgroup of DYN_THREADS = 256 lanes projects DYN_FRAMES = 4 frames, one after the other, for one tile of
// KS k-vectors; KS = min(256, K of the whole call rounded up to a power of two), so S = 256 / KS (dynamic_slices) atom
// slices share a k-vector: lane = slice * KS + k-slot.  K = 1 keeps all 256 lanes busy on 256 slices of the atoms; from
// K = 256 on every lane owns a k-vector.  Each lane keeps the 2 NC accumulators of its k-vector in registers.
// Atoms are wave-uniform where a wavefront holds one slice (KS >= 64): a frame's atoms are staged in tiles of
// DYN_ATOMS = 512 into LDS as (x, y, z, w) and (w v_x, w v_y, w v_z, 0) -- an index list is gathered here, never in the
// inner loop -- and read back as broadcasts; with KS < 64 the lanes of a wavefront read 64 / KS neighbouring atoms.  The
// next tile is fetched into registers while the current one is consumed (two LDS images, one barrier per tile).
// Two atoms are in flight per lane: position p of the atom set (p = 0 .. N_g - 1, tile by tile) belongs to strand
// p mod 2 S; a lane works on strands `slice` and `slice + S` with separate accumulators, which is what covers the latency
// of the two transcendentals.
//
// Phase, in turns.  The host passes kappa = k / 2 pi, formed in float64 from the float32 k, as float32 parts hi + lo per
// component.  Per component the product p = hi x is made error-free (p = fl(hi x), e = fma(hi, x, -p)), its integer
// part is removed exactly (f = p - rint(p)), the three fractions are added with the integer part removed again after
// every addition (each sum is at most 1 in magnitude: rounding error at most u / 2, u = 2^-24), and the small terms
// e_x + e_y + e_z + lo . r are added last.  v_sin_f32 / v_cos_f32 take turns.  With P = sum_c |kappa_c x_c| <= 2^12 turns
// (|k.r| up to 2.5e4 rad) the argument is off by at most 1.5 u + 12 u^2 P < 1.51 u turns; for larger P by 1.5 u + 12 u^2 P
// still (the second term, the float32 evaluation of the small terms, reaches the first at P = 2^21 turns).  The float32 FMA chain k.r in
// radians would be off by about u |k.r|: 1e-4 .. 1e-3 rad at |k.r| = 1e3 .. 1e4.
//
// Summation structure (tests/dynamic_cases.py holds the kernel to the bound derived from it):
//   * a float32 accumulator sums at most DYN_CHAIN = 128 atoms of its strand, one FMA per atom (the products w cos, w sin,
//     (w v_c) cos, (w v_c) sin are not rounded; w v_c is rounded once when it is staged);
//   * it is then folded (one float32 addition) into a second float32 sum: folds(N_g) = ceil(ceil(N_g / 2) / DYN_CHAIN)
//     folds at the most (S = 1; fewer with more slices);
//   * the 2 S strands of a k-vector are added in float64 in ascending strand order (a lane's two, then the slices through
//     LDS), and the sum is rounded once to float32.
// No atomics.  The order depends on K of the whole call and on N_g alone: two identical calls give the same bits, and so
// does a call however its k-vectors are cut into blocks.
//
// Bound, per element, against the float64 evaluation q64 of the definition on the float32 inputs:
//     |q_c[k,t] - q64_c[k,t]| <= (eps_term + (DYN_CHAIN + folds(N_g) + 4) u) sum_a |w_a| |d_a,c(t)|     d = 1 (c = 0), v_c
//     eps_term = 2 pi 1.51 u + sqrt(2) DYN_SINCOS_ERR = 5.7e-7 + 3.7e-7 = 9.3e-7 = 2^-20.0  <=  2^-18
// eps_term: the error of one unit-modulus term, from the argument (in turns, times 2 pi) and from the sine and the cosine
// themselves; DYN_SINCOS_ERR = 2.6e-7 is twice the largest error of v_sin_f32 / v_cos_f32 measured against float64 on a dense
// sweep of [-2, 2] turns, 1.253e-7 on an MI355X (tests/test_gpu_dynamic.py).  The 4: the rounding of w v_c, the final
// rounding, the second-order terms of (1 + u)^(DYN_CHAIN + folds) for DYN_CHAIN + folds <= 2^12, and one to spare.
#include "psa_ctx.h"

namespace psa {

int dynamic_slices(int64_t K) {
    int ks = 1;
    while (ks < DYN_THREADS && ks < K) ks *= 2;
    return DYN_THREADS / ks;
}

namespace {

// (sin, cos)(2 pi s), s in turns, |s| <= 2
__device__ __forceinline__ void dyn_sincos(float s, float& sn, float& cs) {
    sn = __builtin_amdgcn_sinf(s);
    cs = __builtin_amdgcn_cosf(s);
}

// the phase of one atom in turns, reduced to about [-1/2, 1/2]; kh, kl: kappa = k / 2 pi as hi + lo
__device__ __forceinline__ float dyn_turns(const float4 r, const float (&kh)[3], const float (&kl)[3]) {
    const float px = __fmul_rn(kh[0], r.x), py = __fmul_rn(kh[1], r.y), pz = __fmul_rn(kh[2], r.z);
    const float ex = __fmaf_rn(kh[0], r.x, -px), ey = __fmaf_rn(kh[1], r.y, -py), ez = __fmaf_rn(kh[2], r.z, -pz);
    const float fx = px - __builtin_rintf(px), fy = py - __builtin_rintf(py), fz = pz - __builtin_rintf(pz);
    float       s = fx + fy;
    s -= __builtin_rintf(s);
    s += fz;
    s -= __builtin_rintf(s);
    float lo = (ex + ey) + ez;
    lo = __fmaf_rn(kl[0], r.x, lo);
    lo = __fmaf_rn(kl[1], r.y, lo);
    lo = __fmaf_rn(kl[2], r.z, lo);
    return s + lo;
}

template <int NC>
__device__ __forceinline__ void dyn_atom(const float4 r, const float4 wv, const float (&kh)[3], const float (&kl)[3],
                                         float (&acc)[2 * NC]) {
    float sn, cs;
    dyn_sincos(dyn_turns(r, kh, kl), sn, cs);
    acc[0] = __fmaf_rn(r.w, cs, acc[0]);
    acc[1] = __fmaf_rn(r.w, sn, acc[1]);
    if constexpr (NC == 4) {
        acc[2] = __fmaf_rn(wv.x, cs, acc[2]);
        acc[3] = __fmaf_rn(wv.x, sn, acc[3]);
        acc[4] = __fmaf_rn(wv.y, cs, acc[4]);
        acc[5] = __fmaf_rn(wv.y, sn, acc[5]);
        acc[6] = __fmaf_rn(wv.z, cs, acc[6]);
        acc[7] = __fmaf_rn(wv.z, sn, acc[7]);
    }
}

// pos, vel: (T, N, 3) float32; idx: n_g atom indices or null; kappa: (nk, 6) hi xyz, lo xyz; q: (nk, NC, T) complex64.
// Grid: (ceil(T / DYN_FRAMES), ceil(nk / KS)), KS = 256 >> s_log2 k-vectors per workgroup, S = 1 << s_log2 slices.
template <int NC>
__global__ void __launch_bounds__(DYN_THREADS, 4)
dynamic_project_kernel(const float* __restrict__ pos, const float* __restrict__ vel, const float* __restrict__ wgt,
                       const int* __restrict__ idx, const float* __restrict__ kappa, float2* __restrict__ q, int64_t T, int64_t N,
                       int n_g, int nk, int s_log2) {
    constexpr int NV = 2 * NC, PLANES = NC == 4 ? 2 : 1;
    // two images of a tile: [image][plane][atom]; after a frame's last tile the strands' float64 sums [slice][slot][NV]
    // (256 NV doubles: 16 KiB with currents, 4 KiB without) lie over the first image
    __shared__ float4 stage[2][PLANES][DYN_ATOMS];
    static_assert(sizeof(float4) * PLANES * DYN_ATOMS >= sizeof(double) * DYN_THREADS * NV, "the strand sums fit an image");
    const int tid = threadIdx.x;
    const int S = 1 << s_log2, ks = DYN_THREADS >> s_log2, G = 2 * S;
    const int slot = tid & (ks - 1), slice = tid >> (8 - s_log2);
    const int kk = blockIdx.y * ks + slot;
    const bool valid = kk < nk;
    float kh[3], kl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        kh[c] = valid ? kappa[(int64_t)kk * 6 + c] : 0.f;
        kl[c] = valid ? kappa[(int64_t)kk * 6 + 3 + c] : 0.f;
    }
    const int n_tiles = (n_g + DYN_ATOMS - 1) / DYN_ATOMS;

    for (int f = 0; f < DYN_FRAMES; ++f) {
        const int64_t t = (int64_t)blockIdx.x * DYN_FRAMES + f;
        if (t >= T) break;
        float4 nr[2], nv[2];
        // the two atoms of a tile this lane stages: positions tile DYN_ATOMS + h 256 + tid of the set (zeros beyond it)
        auto fetch = [&](int tile) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int p = tile * DYN_ATOMS + h * DYN_THREADS + tid;
                nr[h] = make_float4(0.f, 0.f, 0.f, 0.f);
                nv[h] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p < n_g) {
                    const int     a = idx ? idx[p] : p;
                    const int64_t o = (t * N + a) * 3;
                    const float   w = wgt ? wgt[a] : 1.f;
                    nr[h] = make_float4(pos[o], pos[o + 1], pos[o + 2], w);
                    if constexpr (NC == 4) nv[h] = make_float4(__fmul_rn(w, vel[o]), __fmul_rn(w, vel[o + 1]), __fmul_rn(w, vel[o + 2]), 0.f);
                }
            }
        };
        auto put = [&](int image) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                stage[image][0][h * DYN_THREADS + tid] = nr[h];
                if constexpr (NC == 4) stage[image][PLANES - 1][h * DYN_THREADS + tid] = nv[h];
            }
        };
        float acc[2][NV], fold[2][NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[0][i] = acc[1][i] = fold[0][i] = fold[1][i] = 0.f;
        int chain = 0;
        if (n_tiles > 0) {
            fetch(0);
            put(0);
        }
        __syncthreads();
        for (int tile = 0; tile < n_tiles; ++tile) {
            const int image = tile & 1;
            if (tile + 1 < n_tiles) fetch(tile + 1);
            const int n_here = min(DYN_ATOMS, n_g - tile * DYN_ATOMS), steps = (n_here + G - 1) / G;
            // runs of steps up to the end of the tile or of the chain, so that the loop that does the work holds no
            // condition but its own
            for (int j = 0; j < steps;) {
                const int run = min(steps - j, DYN_CHAIN - chain);
                for (const int e = j + run; j < e; ++j) {
                    const int p0 = j * G + slice, p1 = p0 + S;      // p1 <= (steps - 1) G + 2 S - 1 < DYN_ATOMS
                    const float4 r0 = stage[image][0][p0], r1 = stage[image][0][p1];
                    float4       v0 = r0, v1 = r1;
                    if constexpr (NC == 4) v0 = stage[image][PLANES - 1][p0], v1 = stage[image][PLANES - 1][p1];
                    dyn_atom<NC>(r0, v0, kh, kl, acc[0]);
                    dyn_atom<NC>(r1, v1, kh, kl, acc[1]);
                }
                chain += run;
                if (chain == DYN_CHAIN) {
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        fold[0][i] += acc[0][i], fold[1][i] += acc[1][i];
                        acc[0][i] = acc[1][i] = 0.f;
                    }
                    chain = 0;
                }
            }
            if (tile + 1 < n_tiles) put(image ^ 1);      // last read while tile - 1 was consumed, before the barrier below
            __syncthreads();
        }
        double tot[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) tot[i] = (double)(fold[0][i] + acc[0][i]) + (double)(fold[1][i] + acc[1][i]);
        if (S > 1) {
            double* sums = reinterpret_cast<double*>(&stage[0][0][0]);
#pragma unroll
            for (int i = 0; i < NV; ++i) sums[(slice * ks + slot) * NV + i] = tot[i];
            __syncthreads();
            if (slice == 0)
                for (int s = 1; s < S; ++s)
#pragma unroll
                    for (int i = 0; i < NV; ++i) tot[i] += sums[(s * ks + slot) * NV + i];
            __syncthreads();                                  // the next frame stages over the sums
        }
        if (slice == 0 && valid)
#pragma unroll
            for (int c = 0; c < NC; ++c) q[((int64_t)kk * NC + c) * T + t] = make_float2((float)tot[2 * c], (float)tot[2 * c + 1]);
    }
}

__global__ void __launch_bounds__(256)
dynamic_sincos_kernel(const float* __restrict__ turns, float2* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float sn, cs;
        dyn_sincos(turns[i], sn, cs);
        out[i] = make_float2(sn, cs);
    }
}

// seg: (nk, NC, ns, L) transformed segments; khat (nk, 3); out (1 or 3, L, K_pitch).  One thread per (k, bin): the sum
// over the block's segments is one float32 chain per row.  The transverse part is formed from the perpendicular
// component F_c - h_c (h.F), not as the difference |F|^2 - |h.F|^2 of two nearly equal numbers: it is a sum of squares,
// never negative, and its error is relative to sqrt(|F|^2 |F_perp|^2) instead of |F|^2 (tests/power_cases.py).
template <int NC>
__global__ void __launch_bounds__(256)
dynamic_power_kernel(const float2* __restrict__ seg, const float* __restrict__ khat, float* __restrict__ out, int64_t L, int ns,
                     int nk, int64_t K_pitch, int64_t k_col0, float scale, int first) {
    for (int k = blockIdx.y; k < nk; k += gridDim.y) {
        float h[3] = {0.f, 0.f, 0.f};
        if constexpr (NC == 4) h[0] = khat[(int64_t)k * 3], h[1] = khat[(int64_t)k * 3 + 1], h[2] = khat[(int64_t)k * 3 + 2];
        for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < L; o += (int64_t)gridDim.x * 256) {
            float den = 0.f, lon = 0.f, tra = 0.f;
            for (int s = 0; s < ns; ++s) {
                const float2 f0 = seg[(((int64_t)k * NC) * ns + s) * L + o];
                den += f0.x * f0.x + f0.y * f0.y;
                if constexpr (NC == 4) {
                    float2 fc[3];
                    float  pr = 0.f, pi = 0.f;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        fc[c] = seg[(((int64_t)k * NC + 1 + c) * ns + s) * L + o];
                        pr += h[c] * fc[c].x, pi += h[c] * fc[c].y;
                    }
                    lon += pr * pr + pi * pi;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float tx = fc[c].x - h[c] * pr, ty = fc[c].y - h[c] * pi;
                        tra += tx * tx + ty * ty;
                    }
                }
            }
            const int64_t i = o * K_pitch + k_col0 + k, row = L * K_pitch;
            const float   d = den * scale, l = lon * scale, tr = 0.5f * (tra * scale);
            out[i] = first ? d : out[i] + d;
            if constexpr (NC == 4) {
                out[row + i] = first ? l : out[row + i] + l;
                out[2 * row + i] = first ? tr : out[2 * row + i] + tr;
            }
        }
    }
}

}  // namespace

int launch_dynamic_project(psa_ctx* c, const float* d_pos, const float* d_vel, const float* d_weights, const int* d_idx,
                           const float* d_kappa, float2* d_q, int64_t T, int64_t N, int64_t n_g, int64_t nk, bool currents,
                           int slices) {
    if (nk == 0 || T == 0) return PSA_OK;
    int s_log2 = 0;
    while ((1 << s_log2) < slices) ++s_log2;
    const int     ks = DYN_THREADS >> s_log2;
    const int64_t gx = (T + DYN_FRAMES - 1) / DYN_FRAMES, gy = (nk + ks - 1) / ks;
    PSA_REQUIRE((1 << s_log2) == slices && slices <= DYN_THREADS && gx < (1ll << 31) && gy <= 65535 && n_g >= 0 &&
                    n_g < (1ll << 31) - DYN_ATOMS && N < (1ll << 31) && (!currents || d_vel),
                "dynamic projection outside its grid");
    const dim3 grid((unsigned)gx, (unsigned)gy), block(DYN_THREADS);
    if (currents)
        hipLaunchKernelGGL(dynamic_project_kernel<4>, grid, block, 0, c->stream, d_pos, d_vel, d_weights, d_idx, d_kappa, d_q, T, N,
                           (int)n_g, (int)nk, s_log2);
    else
        hipLaunchKernelGGL(dynamic_project_kernel<1>, grid, block, 0, c->stream, d_pos, d_vel, d_weights, d_idx, d_kappa, d_q, T, N,
                           (int)n_g, (int)nk, s_log2);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_dynamic_power(psa_ctx* c, const float2* d_seg, const float* d_khat, float* d_out, int64_t L, int64_t ns, int64_t nk,
                         bool currents, int64_t K_pitch, int64_t k_col0, float scale, bool first) {
    if (nk == 0) return PSA_OK;
    PSA_REQUIRE(nk < (1ll << 31) && ns < (1ll << 31), "segment block too large");
    const dim3 grid((unsigned)std::min<int64_t>((L + 255) / 256, 64), (unsigned)std::min<int64_t>(nk, 65535)), block(256);
    if (currents)
        hipLaunchKernelGGL(dynamic_power_kernel<4>, grid, block, 0, c->stream, d_seg, d_khat, d_out, L, (int)ns, (int)nk, K_pitch,
                           k_col0, scale, first ? 1 : 0);
    else
        hipLaunchKernelGGL(dynamic_power_kernel<1>, grid, block, 0, c->stream, d_seg, d_khat, d_out, L, (int)ns, (int)nk, K_pitch,
                           k_col0, scale, first ? 1 : 0);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_dynamic_sincos(psa_ctx* c, const float* d_turns, float2* d_out, int64_t n) {
    if (n == 0) return PSA_OK;
    hipLaunchKernelGGL(dynamic_sincos_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, c->stream,
                       d_turns, d_out, n);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
