// Kernels of the self-overlap (psa_self_overlap; definition: include/psa_hip.h, host side: api_overlap.hip): per lag,
// group and time origin the number of atoms that are still within the cut-off a of where they were,
//     Q[j,g,k] = #{ a in g : |u[o_k + tau_j, a] - u[o_k, a]| < a },
// and its first two moments over the origins, S1 = sum_k Q and S2 = sum_k Q^2 -- the mean gives q(t), the variance the
// four-point susceptibility chi_4(t).  The moments and the histogram of msd.hip sum over origins and atoms at once; this
// is the reduction in the other order: over the atoms per (lag, origin) first, then over the origins.
//
//   overlap_count    u64 -> per (chunk of atoms, lag, origin) the uint32 count of overlapping atoms (partials)
//   overlap_reduce   the partials of a group's chunks added to Q (n_lags, G, n_o_max) uint32, which lives across blocks
//   overlap_moments  Q -> S1, S2 (n_lags, G, 2) uint64
//
// The sample is the van Hove sample of msd.hip with one bin of width a: with the origin tiles of msd_origins(step)
// origins, o_0 a tile's first origin,
//     a_c = float32(u_c[o] - u_c[o_0]),   b_c = float32(u_c[o + tau] - u_c[o_0])      (float64 subtraction, one rounding)
//     r2 = msd_unit(b, a).r2,   overlap iff radial_bin(r2, inv_a, 1, 1) == 0,  i.e.  __fmul_rn(__fsqrt_rn(r2), inv_a) < 1
// (inv_a = float32(1 / a)), so S1[j,g] is bin 0 of psa_van_hove_self(dr = a, n_r = 1) bit for bit.
//
// Count.  A workgroup of OVERLAP_LANES lanes takes a piece of one origin tile with a lane per origin, a run of OVERLAP_RUN
// of the call's lags and one chunk of atoms of one group.  Per atom a lane reads u64 at its origin once -- consecutive
// lanes on consecutive origins, 8-byte loads -- keeps a_c in registers, and reads u64 at o + tau for every lag of the run:
// 24 (1 + 1 / OVERLAP_RUN) bytes per sample where the histogram kernel reads 48.  The counts stay in registers over the
// chunk's atoms and leave with plain stores; a lane writes the partials of the lags that have its origin (k < n_o(tau))
// and nothing else, and the reduce reads nothing else.  No LDS, no atomic of any kind: every element of the partials and
// of Q has one writer per launch, and integer adds give the same bits whatever the blocking.
// All index arithmetic into u64, the partials and Q is int64.
#include <algorithm>

#include "min_image.h"
#include "msd_unit.h"
#include "psa_ctx.h"

namespace psa {

namespace {

// the chunks of group g are first[g] .. first[g + 1] - 1 of the table (the host lists them group by group)
struct OverlapGroupChunks {
    int first[MSD_MAX_GROUPS + 1];
};

// Grid ((lag runs x origin tiles x pieces of a tile), chunks).  part[chunk][lag j][origin k], k < n_o(tau_j)
__global__ void __launch_bounds__(OVERLAP_LANES)
overlap_count_kernel(const double* __restrict__ u, const MsdChunk* __restrict__ chunks, const int64_t* __restrict__ lags,
                     unsigned* __restrict__ part, int64_t T, int n_lags, int64_t step, int NO, int n_ot, int n_sub, int64_t n_o_max,
                     float inv_a) {
    const int      sub = blockIdx.x % n_sub, tile = blockIdx.x / n_sub % n_ot, run = blockIdx.x / n_sub / n_ot;
    const int      kl = sub * OVERLAP_LANES + threadIdx.x;                  // the lane's origin within the tile
    const int64_t  k = (int64_t)tile * NO + kl, o0 = (int64_t)tile * NO * step;
    const bool     here = kl < NO && k < n_o_max;                          // o <= T - 1
    const int64_t  o = here ? k * step : o0;
    const MsdChunk ch = chunks[blockIdx.y];
    int64_t        tau[OVERLAP_RUN];
    bool           mine[OVERLAP_RUN];
    unsigned       count[OVERLAP_RUN];
#pragma unroll
    for (int l = 0; l < OVERLAP_RUN; ++l) {
        const int j = run * OVERLAP_RUN + l;
        tau[l] = j < n_lags ? lags[j] : 0;
        mine[l] = here && j < n_lags && o + tau[l] <= T - 1;               // k < n_o(tau)
        count[l] = 0u;
    }
    for (int a = ch.a_lo; a < ch.a_hi; ++a) {
        const double* ux = u + (int64_t)a * 3 * T, *uy = ux + T, *uz = uy + T;
        const double  bx = ux[o0], by = uy[o0], bz = uz[o0];
        const float   ax = (float)(ux[o] - bx), ay = (float)(uy[o] - by), az = (float)(uz[o] - bz);
        double        fx[OVERLAP_RUN], fy[OVERLAP_RUN], fz[OVERLAP_RUN];
#pragma unroll
        for (int l = 0; l < OVERLAP_RUN; ++l) {                            // every load of the run in flight at once; a lane
            const int64_t f = mine[l] ? o + tau[l] : o;                    // without the sample re-reads its origin
            fx[l] = ux[f], fy[l] = uy[f], fz[l] = uz[f];
        }
#pragma unroll
        for (int l = 0; l < OVERLAP_RUN; ++l) {
            const MsdUnit q = msd_unit((float)(fx[l] - bx), (float)(fy[l] - by), (float)(fz[l] - bz), ax, ay, az);
            count[l] += mine[l] && radial_bin(q.r2, inv_a, 1.0f, 1) == 0 ? 1u : 0u;
        }
    }
#pragma unroll
    for (int l = 0; l < OVERLAP_RUN; ++l)
        if (mine[l]) part[((int64_t)blockIdx.y * n_lags + (run * OVERLAP_RUN + l)) * n_o_max + k] = count[l];
}

// q[lag][group][k] += the partials of the group's chunks, k < n_o(lag): one lane per element, the only writer of it
__global__ void __launch_bounds__(256)
overlap_reduce_kernel(const unsigned* __restrict__ part, const OverlapGroupChunks of, const int64_t* __restrict__ lags,
                      unsigned* __restrict__ q, int64_t T, int n_lags, int G, int64_t step, int64_t n_o_max) {
    const int64_t n = (int64_t)n_lags * G * n_o_max;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t k = i % n_o_max;
        const int     g = (int)(i / n_o_max % G), j = (int)(i / n_o_max / G);
        if (of.first[g + 1] == of.first[g] || k * step + lags[j] > T - 1) continue;   // k >= n_o(lag)
        unsigned sum = q[i];
        for (int64_t r = of.first[g]; r < of.first[g + 1]; ++r) sum += part[(r * n_lags + j) * n_o_max + k];
        q[i] = sum;
    }
}

// Grid (lags, groups).  sums[lag][group] = {sum_k q, sum_k q^2}, k < n_o(lag), in uint64: a shuffle reduce per
// wavefront, the four wavefronts' sums through LDS with plain stores
__global__ void __launch_bounds__(256)
overlap_moments_kernel(const unsigned* __restrict__ q, const int64_t* __restrict__ lags, unsigned long long* __restrict__ sums,
                       int64_t T, int64_t step, int64_t n_o_max) {
    __shared__ unsigned long long waves[4][2];
    const int       j = blockIdx.x, g = blockIdx.y, wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int64_t   n_o = (T - 1 - lags[j]) / step + 1;
    const unsigned* row = q + ((int64_t)j * gridDim.y + g) * n_o_max;
    unsigned long long s1 = 0, s2 = 0;
    for (int64_t k = threadIdx.x; k < n_o; k += 256) {
        const unsigned long long v = row[k];
        s1 += v, s2 += v * v;
    }
    for (int d = 32; d >= 1; d >>= 1) s1 += __shfl_xor(s1, d, 64), s2 += __shfl_xor(s2, d, 64);
    if (lane == 0) waves[wave][0] = s1, waves[wave][1] = s2;
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long* dst = sums + ((int64_t)j * gridDim.y + g) * 2;
        dst[threadIdx.x] = waves[0][threadIdx.x] + waves[1][threadIdx.x] + waves[2][threadIdx.x] + waves[3][threadIdx.x];
    }
}

}  // namespace

int launch_overlap_count(psa_ctx* c, const double* d_u, const void* d_chunks, int64_t n_chunks, const int64_t* d_lags, int64_t n_lags,
                         unsigned* d_part, int64_t T, int64_t step, int64_t n_o_max, float inv_a) {
    if (n_chunks == 0) return PSA_OK;
    const int     NO = msd_origins(step);
    const int64_t n_runs = (n_lags + OVERLAP_RUN - 1) / OVERLAP_RUN, n_ot = (n_o_max + NO - 1) / NO;
    const int64_t n_sub = (std::min<int64_t>(NO, n_o_max) + OVERLAP_LANES - 1) / OVERLAP_LANES;
    PSA_REQUIRE(n_lags >= 1 && n_lags <= OVERLAP_MAX_LAGS && step >= 1 && n_o_max >= 1 && n_o_max <= (T - 1) / step + 1 &&
                    n_ot < (1ll << 31) && n_runs * n_ot * n_sub < (1ll << 31) && n_chunks <= 65535,
                "overlap count pass outside its grid");
    hipLaunchKernelGGL(overlap_count_kernel, dim3((unsigned)(n_runs * n_ot * n_sub), (unsigned)n_chunks), dim3(OVERLAP_LANES), 0, c->stream,
                       d_u, static_cast<const MsdChunk*>(d_chunks), d_lags, d_part, T, (int)n_lags, step, NO, (int)n_ot, (int)n_sub, n_o_max,
                       inv_a);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_overlap_reduce(psa_ctx* c, const unsigned* d_part, const int32_t* group_first, const int64_t* d_lags, unsigned* d_q, int64_t T,
                          int64_t n_lags, int32_t G, int64_t step, int64_t n_o_max) {
    if (group_first[G] == 0) return PSA_OK;
    PSA_REQUIRE(G >= 1 && G <= MSD_MAX_GROUPS && n_lags >= 1 && n_lags <= OVERLAP_MAX_LAGS && n_o_max >= 1, "overlap reduce outside its grid");
    OverlapGroupChunks of = {};
    for (int g = 0; g <= G; ++g) of.first[g] = group_first[g];
    const int64_t n = n_lags * G * n_o_max;
    hipLaunchKernelGGL(overlap_reduce_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 16)), dim3(256), 0, c->stream, d_part, of,
                       d_lags, d_q, T, (int)n_lags, (int)G, step, n_o_max);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_overlap_moments(psa_ctx* c, const unsigned* d_q, const int64_t* d_lags, unsigned long long* d_sums, int64_t T, int64_t n_lags,
                           int32_t G, int64_t step, int64_t n_o_max) {
    PSA_REQUIRE(G >= 1 && G <= MSD_MAX_GROUPS && n_lags >= 1 && n_lags <= OVERLAP_MAX_LAGS && n_o_max >= 1, "overlap moments outside their grid");
    hipLaunchKernelGGL(overlap_moments_kernel, dim3((unsigned)n_lags, (unsigned)G), dim3(256), 0, c->stream, d_q, d_lags, d_sums, T, step,
                       n_o_max);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
