// Projections on the reciprocal lattice of the simulation box and their shell sums (psa_lattice_spectra; definition:
// include/psa_hip.h, host side: api_lattice.hip):
//
//     q_0[n,t] = sum_a w_a exp(2 pi i n.s_a(t))        q_c[n,t] = sum_a w_a v_a,c(t) exp(2 pi i n.s_a(t))      c = 1, 2, 3
//     s = r . Hinv  (fractional coordinates),  n in Z^3,  |n_j| <= LAT_MAX_INDEX
//
// With integer n the phase factorises, exp(2 pi i n.s) = E_1[n_1] E_2[n_2] E_3[n_3], E_j[m] = exp(2 pi i m s_j), so the
// sine and the cosine are needed per (atom, frame, axis index) and not per (atom, frame, vector): dynamic.hip pays 33
// VALU instructions and two transcendentals per unit, this kernel two complex products and the accumulation.
//
// Work split.  A workgroup of LAT_THREADS = 256 lanes projects LAT_FRAMES = 4 frames, one after the other, for one tile
// of LAT_KS = 512 vectors: lane l owns vectors l and l + 256 of the tile and keeps their 2 x 2 NC accumulators in
// registers.  The host (api_lattice.hip) sorts a block's vectors by (n_1, n_2, n_3), cuts the tiles, and lists per tile
// the distinct (axis, m) pairs its vectors use -- its R <= 3 (2 LAT_MAX_INDEX + 1) = 387 entries -- and per vector the
// three entries it reads; a tile of a half-sphere of some thousand vectors has R = 40 .. 70.  Per frame the atoms go
// through LDS in tiles of A = min(LAT_ATOMS, LAT_TABLE / R) atoms, three steps with a barrier after each:
//   stage       lane a < A loads atom a (an index list is gathered here), forms (s_hi, s_lo)_j for the three axes and
//               (w, w v_x, w v_y, w v_z), and writes them to LDS;
//   build       the A R entries tab[a][e] = (cos, sin)(2 pi m s_j) are evaluated, one per lane and step, each directly
//               from m and s_j -- no recurrence in m, so an entry's error does not grow with |m|;
//   accumulate  per atom a lane reads (w, w v) as a broadcast and, per vector, its three entries; E = (E_1 E_2) E_3 in
//               two float32 complex products; 2 NC FMAs.  No sine, no cosine, no global load in this loop.
//
// Fractional coordinates, in turns.  The host passes Hinv as float32 hi + lo per entry.  For axis j the three products
// h_cj r_c are made error-free (p = fl(h r), e = fma(h, r, -p)), their integer parts are removed exactly (f = p - rint(p):
// n is an integer, so whole turns of s do not matter), the fractions are added with the integer part removed after each
// addition and the rounding error of each addition recovered exactly (two-sum); s_hi is that sum (|s_hi| <= 1/2) and
// s_lo = e_x + e_y + e_z + lo . r + the two recovered errors, evaluated in float32.  For an entry, m s_hi is again
// error-free (p = fl(m s_hi), e = fma(m, s_hi, -p)), reduced exactly (g = p - rint(p)), and the argument is
// fl(g + fma(m, s_lo, e)) turns.  With P = sum_c |h_cj r_c| <= 2^12 turns and |m| <= M = LAT_MAX_INDEX = 64:
//     |s_lo| <= 2 u P + 2 u;  its seven float32 operations and the unrepresented part of Hinv: 15 u^2 P + 14 u^2;
//     times M: 0.24 u;  the fma: u M (2 u P + 2 u) = 0.03 u;  the final rounding of |.| <= 1/2 + 2^-4: u / 2
//     argument error <= u / 2 + 17 M u^2 P <= 0.77 u < 1.0 u turns                       (u = 2^-24)
// independent of |r| up to P = 2^12 turns (|k.r| up to 5e4 rad with three axes); beyond that the second term grows in
// proportion.  s_j rounded to one float32 would be off by u / 2 turns, the entry by M u / 2 = 32 u turns = 1.2e-5 rad.
//
// eps_lat, the error of one unit-modulus term E_1 E_2 E_3:
//     one entry:   2 pi 1.0 u + sqrt(2) DYN_SINCOS_ERR = 3.75e-7 + 3.68e-7 = 7.43e-7   (dynamic.hip's sine and cosine)
//     a float32 complex product of two such numbers (2 mul + 2 fma): each component off by at most 2 u, the modulus by
//     2 sqrt(2) u; two products and the second-order terms: 6 u
//     eps_lat = 3 (2 pi u + sqrt(2) DYN_SINCOS_ERR) + 6 u = 2.23e-6 + 0.36e-6 = 2.59e-6 = 0.68 x 2^-18  <=  2^-18
//
// Summation structure (tests/lattice_cases.py holds the kernel to the bound derived from it): one strand per vector --
//   * a float32 accumulator sums at most LAT_CHAIN = 128 atoms, in the order of the atom set, one FMA per atom (w cos,
//     w sin, (w v_c) cos, (w v_c) sin are not rounded; w v_c is rounded once when it is staged);
//   * it is then folded (one float32 addition) into a second float32 sum, and once more at the end:
//     folds(N_g) = ceil(N_g / LAT_CHAIN).
// No float64, no atomics.  The order depends on N_g alone, and an entry on (atom, m) alone: two identical calls give the
// same bits, and so does a call however its vectors are cut into blocks and tiles.
//     |q_c[n,t] - q64_c[n,t]| <= (eps_lat + (LAT_CHAIN + folds(N_g) + 4) u) sum_a |w_a| |d_a,c(t)|     d = 1 (c = 0), v_c
//
// Shell pass (lattice_shell_kernel): after the window pass and the rocFFT of a sub-block (nb, NC, ns, L), one lane per
// (bin, frequency o) adds X_n[o] + X_n[(L - o) mod L] -- each term float32, the sum float64 -- over the sub-block's
// vectors of the bin (one contiguous range: the host orders by bin) and its segments, vector by vector, segment by
// segment, and adds the total to the float64 accumulator (1 or 3, L, n_bins), which lives across sub-blocks and blocks.
// The transverse term of a (vector, segment, side) is half the squared modulus of the perpendicular component
// F_c - h_c (h.F), as in dynamic.hip: a sum of squares, never negative.
// lattice_finish_kernel scales by 1 / (2 n_half_b n_seg U L^2) in float64 and rounds once to float32.
#include "lattice_math.h"
#include "psa_ctx.h"

namespace psa {

namespace {

constexpr int LAT_KPL = LAT_KS / LAT_THREADS;      // vectors per lane

// pos, vel: (T, N, 3) float32; idx: n_g atom indices or null.  Tiles tile0 + blockIdx.y of the call's plan: tile_off
// (n_tiles + 1) offsets into ent, the tiles' entries (axis << 8 | m + 128); per tile LAT_KS vectors: slot = its three
// entries (9 bits each), dest = its row of q (nk, NC, T) complex64 or -1.  Grid: (ceil(T / LAT_FRAMES), tiles).
template <int NC>
__global__ void __launch_bounds__(LAT_THREADS, 4)
lattice_project_kernel(const float* __restrict__ pos, const float* __restrict__ vel, const float* __restrict__ wgt,
                       const int* __restrict__ idx, const LatBox box, const int* __restrict__ tile_off,
                       const unsigned short* __restrict__ ent, const unsigned* __restrict__ slot, const int* __restrict__ dest,
                       float2* __restrict__ q, int64_t T, int64_t N, int n_g, int tile0) {
    constexpr int NV = 2 * NC;
    __shared__ float2         tab[LAT_TABLE];
    __shared__ float4         wbuf[LAT_ATOMS];
    __shared__ float2         sbuf[3][LAT_ATOMS];
    __shared__ unsigned short ents[LAT_MAX_ENTRIES + 1];
    const int tid = threadIdx.x;
    const int tile = tile0 + blockIdx.y;
    const int e0 = tile_off[tile], R = tile_off[tile + 1] - e0;          // 3 <= R <= LAT_MAX_ENTRIES (the host's plan)
    if (R < 1 || R > LAT_MAX_ENTRIES) return;
    for (int i = tid; i < R; i += LAT_THREADS) ents[i] = ent[e0 + i];
    const int   A = min(LAT_ATOMS, LAT_TABLE / R);
    const float inv_R = 1.f / (float)R;
    int         off[LAT_KPL][3], row[LAT_KPL];
#pragma unroll
    for (int j = 0; j < LAT_KPL; ++j) {
        const int64_t  p = (int64_t)tile * LAT_KS + j * LAT_THREADS + tid;
        const unsigned u = slot[p];
        off[j][0] = u & 511, off[j][1] = (u >> 9) & 511, off[j][2] = (u >> 18) & 511;    // < R
        row[j] = dest[p];
    }
    __syncthreads();

    for (int f = 0; f < LAT_FRAMES; ++f) {
        const int64_t t = (int64_t)blockIdx.x * LAT_FRAMES + f;
        if (t >= T) break;
        float acc[LAT_KPL][NV], fold[LAT_KPL][NV];
#pragma unroll
        for (int j = 0; j < LAT_KPL; ++j)
#pragma unroll
            for (int i = 0; i < NV; ++i) acc[j][i] = fold[j][i] = 0.f;
        int chain = 0;
        for (int base = 0; base < n_g; base += A) {
            const int n_here = min(A, n_g - base);
            if (tid < n_here) {                                         // stage
                const int     a = idx ? idx[base + tid] : base + tid;
                const int64_t o = (t * N + a) * 3;
                const float   w = wgt ? wgt[a] : 1.f;
                const float   x = pos[o], y = pos[o + 1], z = pos[o + 2];
                float4        wv = make_float4(w, 0.f, 0.f, 0.f);
                if constexpr (NC == 4) wv = make_float4(w, __fmul_rn(w, vel[o]), __fmul_rn(w, vel[o + 1]), __fmul_rn(w, vel[o + 2]));
                wbuf[tid] = wv;
#pragma unroll
                for (int j = 0; j < 3; ++j) sbuf[j][tid] = lat_frac(x, y, z, box, j);
            }
            __syncthreads();
            for (int i = tid; i < n_here * R; i += LAT_THREADS) {      // build: i = a R + e
                int a = (int)__fmul_rn((float)i, inv_R), e = i - a * R;
                if (e < 0) --a, e += R;
                else if (e >= R) ++a, e -= R;
                const int code = ents[e];
                tab[i] = lat_entry((float)((code & 255) - 128), sbuf[code >> 8][a]);
            }
            __syncthreads();
            // accumulate: runs up to the end of the tile or of the chain, so that the loop that does the work holds no
            // condition but its own
            for (int a = 0; a < n_here;) {
                const int run = min(n_here - a, LAT_CHAIN - chain);
                for (const int e = a + run; a < e; ++a) {
                    const float4  wv = wbuf[a];
                    const float2* ta = tab + a * R;
#pragma unroll
                    for (int j = 0; j < LAT_KPL; ++j) {
                        const float2 E = lat_cmul(lat_cmul(ta[off[j][0]], ta[off[j][1]]), ta[off[j][2]]);
                        acc[j][0] = __fmaf_rn(wv.x, E.x, acc[j][0]);
                        acc[j][1] = __fmaf_rn(wv.x, E.y, acc[j][1]);
                        if constexpr (NC == 4) {
                            acc[j][2] = __fmaf_rn(wv.y, E.x, acc[j][2]);
                            acc[j][3] = __fmaf_rn(wv.y, E.y, acc[j][3]);
                            acc[j][4] = __fmaf_rn(wv.z, E.x, acc[j][4]);
                            acc[j][5] = __fmaf_rn(wv.z, E.y, acc[j][5]);
                            acc[j][6] = __fmaf_rn(wv.w, E.x, acc[j][6]);
                            acc[j][7] = __fmaf_rn(wv.w, E.y, acc[j][7]);
                        }
                    }
                }
                chain += run;
                if (chain == LAT_CHAIN) {
#pragma unroll
                    for (int j = 0; j < LAT_KPL; ++j)
#pragma unroll
                        for (int i = 0; i < NV; ++i) fold[j][i] += acc[j][i], acc[j][i] = 0.f;
                    chain = 0;
                }
            }
            __syncthreads();                                            // the next tile is staged over this one
        }
#pragma unroll
        for (int j = 0; j < LAT_KPL; ++j)
            if (row[j] >= 0)
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    q[((int64_t)row[j] * NC + c) * T + t] = make_float2(fold[j][2 * c] + acc[j][2 * c], fold[j][2 * c + 1] + acc[j][2 * c + 1]);
    }
}

// seg: (nb, NC, ns, L) transformed segments of the vectors g0 .. g0 + nb - 1 of the processing order; khat: their rows;
// bin_start (n_bins + 1): where each bin's vectors begin in that order; acc (1 or 3, L, n_bins) float64.  One lane per
// (bin, o): blockIdx.y strides the bins, the lanes of a row of blocks the frequencies.
template <int NC>
__global__ void __launch_bounds__(256)
lattice_shell_kernel(const float2* __restrict__ seg, const float* __restrict__ khat, const int* __restrict__ bin_start,
                     double* __restrict__ acc, int64_t L, int ns, int64_t g0, int nb, int n_bins) {
    for (int b = blockIdx.y; b < n_bins; b += gridDim.y) {
        const int k_lo = (int)(max((int64_t)bin_start[b], g0) - g0), k_hi = (int)(min((int64_t)bin_start[b + 1], g0 + nb) - g0);
        if (k_lo >= k_hi) continue;
        for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < L; o += (int64_t)gridDim.x * 256) {
            const int64_t om = o == 0 ? 0 : L - o;
            double        den = 0.0, lon = 0.0, tra = 0.0;
            for (int k = k_lo; k < k_hi; ++k) {
                float h[3] = {0.f, 0.f, 0.f};
                if constexpr (NC == 4) h[0] = khat[(int64_t)k * 3], h[1] = khat[(int64_t)k * 3 + 1], h[2] = khat[(int64_t)k * 3 + 2];
                for (int s = 0; s < ns; ++s) {
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        const int64_t oo = side ? om : o;
                        const float2  f0 = seg[(((int64_t)k * NC) * ns + s) * L + oo];
                        den += (double)(f0.x * f0.x + f0.y * f0.y);
                        if constexpr (NC == 4) {
                            float2 fc[3];
                            float  pr = 0.f, pi = 0.f, t = 0.f;
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                fc[c] = seg[(((int64_t)k * NC + 1 + c) * ns + s) * L + oo];
                                pr += h[c] * fc[c].x, pi += h[c] * fc[c].y;
                            }
                            lon += (double)(pr * pr + pi * pi);
#pragma unroll
                            for (int c = 0; c < 3; ++c) {                  // the perpendicular component: dynamic.hip
                                const float tx = fc[c].x - h[c] * pr, ty = fc[c].y - h[c] * pi;
                                t += tx * tx + ty * ty;
                            }
                            tra += (double)(0.5f * t);
                        }
                    }
                }
            }
            const int64_t i = o * n_bins + b, plane = L * n_bins;
            acc[i] += den;
            if constexpr (NC == 4) acc[plane + i] += lon, acc[2 * plane + i] += tra;
        }
    }
}

// out (rows, L, n_bins) float32 = acc scale[bin], the product in float64
__global__ void __launch_bounds__(256)
lattice_finish_kernel(const double* __restrict__ acc, const double* __restrict__ scale, float* __restrict__ out, int64_t n, int n_bins) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = (float)(acc[i] * scale[i % n_bins]);
}

}  // namespace

int launch_lattice_project(psa_ctx* c, const float* d_pos, const float* d_vel, const float* d_weights, const int* d_idx,
                           const float* box_hi, const float* box_lo, const int* d_tile_off, const unsigned short* d_ent,
                           const unsigned* d_slot, const int* d_dest, float2* d_q, int64_t T, int64_t N, int64_t n_g, int64_t tile0,
                           int64_t n_tiles, bool currents) {
    if (n_tiles == 0 || T == 0) return PSA_OK;
    const int64_t gx = (T + LAT_FRAMES - 1) / LAT_FRAMES;
    PSA_REQUIRE(gx < (1ll << 31) && n_tiles <= 65535 && tile0 >= 0 && tile0 + n_tiles < (1ll << 22) && n_g >= 0 &&
                    n_g < (1ll << 31) - LAT_ATOMS && N < (1ll << 31) && (!currents || d_vel),
                "lattice projection outside its grid");
    LatBox box;
    for (int i = 0; i < 9; ++i) box.hi[i] = box_hi[i], box.lo[i] = box_lo[i];
    const dim3 grid((unsigned)gx, (unsigned)n_tiles), block(LAT_THREADS);
    if (currents)
        hipLaunchKernelGGL(lattice_project_kernel<4>, grid, block, 0, c->stream, d_pos, d_vel, d_weights, d_idx, box, d_tile_off, d_ent,
                           d_slot, d_dest, d_q, T, N, (int)n_g, (int)tile0);
    else
        hipLaunchKernelGGL(lattice_project_kernel<1>, grid, block, 0, c->stream, d_pos, d_vel, d_weights, d_idx, box, d_tile_off, d_ent,
                           d_slot, d_dest, d_q, T, N, (int)n_g, (int)tile0);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_lattice_shell(psa_ctx* c, const float2* d_seg, const float* d_khat, const int* d_bin_start, double* d_acc, int64_t L,
                         int64_t ns, int64_t g0, int64_t nb, int64_t n_bins, bool currents) {
    if (nb == 0 || n_bins == 0) return PSA_OK;
    PSA_REQUIRE(nb < (1ll << 31) && ns < (1ll << 31) && n_bins < (1ll << 31), "shell block too large");
    const dim3 grid((unsigned)std::min<int64_t>((L + 255) / 256, 1024), (unsigned)std::min<int64_t>(n_bins, 65535)), block(256);
    if (currents)
        hipLaunchKernelGGL(lattice_shell_kernel<4>, grid, block, 0, c->stream, d_seg, d_khat, d_bin_start, d_acc, L, (int)ns, g0, (int)nb,
                           (int)n_bins);
    else
        hipLaunchKernelGGL(lattice_shell_kernel<1>, grid, block, 0, c->stream, d_seg, d_khat, d_bin_start, d_acc, L, (int)ns, g0, (int)nb,
                           (int)n_bins);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_lattice_finish(psa_ctx* c, const double* d_acc, const double* d_scale, float* d_out, int64_t n, int64_t n_bins) {
    if (n == 0) return PSA_OK;
    hipLaunchKernelGGL(lattice_finish_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, c->stream, d_acc,
                       d_scale, d_out, n, (int)n_bins);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
