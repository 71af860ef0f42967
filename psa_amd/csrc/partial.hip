// The passes after the FFT of the species-resolved (partial) spectra on the box's reciprocal lattice (psa_partial_spectra;
// definition: include/psa_hip.h, host side: api_partial.hip).  Every vector holds the NC series of S species,
//
//     seg (nb, S, NC, ns, L)     F^a_c of vector k, species a, component c, segment s:  (((k S + a) NC + c) ns + s) L + o
//
// which the unchanged projection kernel (lattice.hip, one launch per species), window pass and rocFFT have filled, and a
// pair p = (a, b), a <= b -- row-major over the upper triangle, P = S (S + 1) / 2 of them -- gets the real parts
//
//     density       Re F^a_0 conj F^b_0
//     longitudinal  Re (h.F^a) conj (h.F^b)                        h = k / |k|
//     transverse    1/2 sum_c Re F_perp,c^a conj F_perp,c^b         F_perp,c = F_c - h_c (h.F)
//
// where dynamic_power_kernel and lattice_shell_kernel take the moduli of one species.  The transverse part is the product
// of the two perpendicular components, as in dynamic.hip: never a difference of the other two.  For a = b every
// expression below is the one of those kernels with both factors equal, so a diagonal pair is a sum of squares.
//
// Work split.  One lane per (pair, vector or bin, frequency): blockIdx.y strides the (vector or bin, pair) units, the
// lanes of a row of blocks the frequencies.  A lane reads the 2 NC values of its two species itself; the P lanes that
// share a (vector, frequency) reread them through L2, which is cheap beside the projection, needs no registers that grow
// with S, and gives the shell pass -- a serial walk over a bin's vectors -- P times the lanes of lattice_shell_kernel.
//
// Summation structure, that of the kernels these replace.  Per-vector form: every term float32, the sum over a
// sub-block's segments one float32 chain, the scale one float32 product, later sub-blocks of segments added in float32.
// Shell form: every term float32 -- the one at o and the one at (L - o) mod L, both factors mirrored: X^ab_-n[o] =
// X^ab_n[(L - o) mod L] holds for the real part, since q^a(-n) = conj q^a(n) for real weights --, summed in float64 over
// the sub-block's vectors of the bin (one contiguous range), vector by vector, segment by segment, side by side, and added
// to the float64 accumulator (1 or 3, P, L, n_bins); lattice_finish_kernel scales and rounds it once.  No atomics: a lane
// owns its element of the result, and the order is fixed.
#include "psa_ctx.h"

namespace psa {

namespace {

// pair p of S species, row-major over the upper triangle: (0,0), (0,1), .., (0,S-1), (1,1), ..  (uniform over a workgroup)
__device__ __forceinline__ void pair_species(int p, int S, int& a, int& b) {
    a = 0;
    while (p >= S - a) p -= S - a, ++a;
    b = a + p;
}

// the three terms of one (vector, segment, frequency) for a pair: fa, fb point at component 0 of the two species at that
// segment and frequency, `comp` is the distance between components
template <int NC>
__device__ __forceinline__ void pair_terms(const float2* __restrict__ fa, const float2* __restrict__ fb, int64_t comp,
                                           const float (&h)[3], float& den, float& lon, float& tra) {
    const float2 a0 = fa[0], b0 = fb[0];
    den = a0.x * b0.x + a0.y * b0.y;
    if constexpr (NC == 4) {
        float2 ac[3], bc[3];
        float  par = 0.f, pai = 0.f, pbr = 0.f, pbi = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ac[c] = fa[(1 + c) * comp], bc[c] = fb[(1 + c) * comp];
            par += h[c] * ac[c].x, pai += h[c] * ac[c].y;
            pbr += h[c] * bc[c].x, pbi += h[c] * bc[c].y;
        }
        lon = par * pbr + pai * pbi;
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                          // the perpendicular components: dynamic.hip
            const float ax = ac[c].x - h[c] * par, ay = ac[c].y - h[c] * pai;
            const float bx = bc[c].x - h[c] * pbr, by = bc[c].y - h[c] * pbi;
            t += ax * bx + ay * by;
        }
        tra = t;
    }
}

// seg (nk, S, NC, ns, L); khat (nk, 3); out (1 or 3, P, L, K_pitch), columns k_col0 + k
template <int NC>
__global__ void __launch_bounds__(256)
partial_power_kernel(const float2* __restrict__ seg, const float* __restrict__ khat, float* __restrict__ out, int64_t L, int ns, int nk,
                     int S, int64_t K_pitch, int64_t k_col0, float scale, int first) {
    const int     P = S * (S + 1) / 2;
    const int64_t comp = (int64_t)ns * L, units = (int64_t)nk * P;
    for (int64_t u = blockIdx.y; u < units; u += gridDim.y) {
        const int k = (int)(u / P), p = (int)(u - (int64_t)k * P);
        float     h[3] = {0.f, 0.f, 0.f};
        if constexpr (NC == 4) h[0] = khat[(int64_t)k * 3], h[1] = khat[(int64_t)k * 3 + 1], h[2] = khat[(int64_t)k * 3 + 2];
        int           sa, sb;
        pair_species(p, S, sa, sb);
        const float2* fa = seg + ((int64_t)k * S + sa) * NC * comp;
        const float2* fb = seg + ((int64_t)k * S + sb) * NC * comp;
        for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < L; o += (int64_t)gridDim.x * 256) {
            float den = 0.f, lon = 0.f, tra = 0.f;
            for (int s = 0; s < ns; ++s) {
                float d = 0.f, l = 0.f, t = 0.f;
                pair_terms<NC>(fa + (int64_t)s * L + o, fb + (int64_t)s * L + o, comp, h, d, l, t);
                den += d, lon += l, tra += t;
            }
            const int64_t i = ((int64_t)p * L + o) * K_pitch + k_col0 + k, row = (int64_t)P * L * K_pitch;
            const float   d = den * scale, l = lon * scale, tr = 0.5f * (tra * scale);
            out[i] = first ? d : out[i] + d;
            if constexpr (NC == 4) {
                out[row + i] = first ? l : out[row + i] + l;
                out[2 * row + i] = first ? tr : out[2 * row + i] + tr;
            }
        }
    }
}

// seg (nb, S, NC, ns, L) of the vectors g0 .. g0 + nb - 1 of the processing order; khat: their rows; bin_start
// (n_bins + 1): where each bin's vectors begin in that order; acc (1 or 3, P, L, n_bins) float64
template <int NC>
__global__ void __launch_bounds__(256)
partial_shell_kernel(const float2* __restrict__ seg, const float* __restrict__ khat, const int* __restrict__ bin_start,
                     double* __restrict__ acc, int64_t L, int ns, int64_t g0, int nb, int n_bins, int S) {
    const int     P = S * (S + 1) / 2;
    const int64_t comp = (int64_t)ns * L, units = (int64_t)n_bins * P;
    for (int64_t u = blockIdx.y; u < units; u += gridDim.y) {
        const int b = (int)(u / P), p = (int)(u - (int64_t)b * P);
        const int k_lo = (int)(max((int64_t)bin_start[b], g0) - g0), k_hi = (int)(min((int64_t)bin_start[b + 1], g0 + nb) - g0);
        if (k_lo >= k_hi) continue;
        int sa, sb;
        pair_species(p, S, sa, sb);
        for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < L; o += (int64_t)gridDim.x * 256) {
            const int64_t om = o == 0 ? 0 : L - o;
            double        den = 0.0, lon = 0.0, tra = 0.0;
            for (int k = k_lo; k < k_hi; ++k) {
                float h[3] = {0.f, 0.f, 0.f};
                if constexpr (NC == 4) h[0] = khat[(int64_t)k * 3], h[1] = khat[(int64_t)k * 3 + 1], h[2] = khat[(int64_t)k * 3 + 2];
                const float2* fa = seg + ((int64_t)k * S + sa) * NC * comp;
                const float2* fb = seg + ((int64_t)k * S + sb) * NC * comp;
                for (int s = 0; s < ns; ++s) {
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        const int64_t at = (int64_t)s * L + (side ? om : o);
                        float         d = 0.f, l = 0.f, t = 0.f;
                        pair_terms<NC>(fa + at, fb + at, comp, h, d, l, t);
                        den += (double)d;
                        if constexpr (NC == 4) lon += (double)l, tra += (double)(0.5f * t);
                    }
                }
            }
            const int64_t i = ((int64_t)p * L + o) * n_bins + b, plane = (int64_t)P * L * n_bins;
            acc[i] += den;
            if constexpr (NC == 4) acc[plane + i] += lon, acc[2 * plane + i] += tra;
        }
    }
}

}  // namespace

int launch_partial_power(psa_ctx* c, const float2* d_seg, const float* d_khat, float* d_out, int64_t L, int64_t ns, int64_t nk,
                         int n_species, bool currents, int64_t K_pitch, int64_t k_col0, float scale, bool first) {
    if (nk == 0) return PSA_OK;
    PSA_REQUIRE(n_species >= 1 && n_species <= PARTIAL_MAX_SPECIES, "1 to %d species are served, got %d", PARTIAL_MAX_SPECIES, n_species);
    PSA_REQUIRE(nk < (1ll << 31) && ns < (1ll << 31), "segment block too large");
    const int64_t P = (int64_t)n_species * (n_species + 1) / 2;
    const dim3 grid((unsigned)std::min<int64_t>((L + 255) / 256, 64), (unsigned)std::min<int64_t>(nk * P, 65535)), block(256);
    if (currents)
        hipLaunchKernelGGL(partial_power_kernel<4>, grid, block, 0, c->stream, d_seg, d_khat, d_out, L, (int)ns, (int)nk, n_species,
                           K_pitch, k_col0, scale, first ? 1 : 0);
    else
        hipLaunchKernelGGL(partial_power_kernel<1>, grid, block, 0, c->stream, d_seg, d_khat, d_out, L, (int)ns, (int)nk, n_species,
                           K_pitch, k_col0, scale, first ? 1 : 0);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_partial_shell(psa_ctx* c, const float2* d_seg, const float* d_khat, const int* d_bin_start, double* d_acc, int64_t L,
                         int64_t ns, int64_t g0, int64_t nb, int64_t n_bins, int n_species, bool currents) {
    if (nb == 0 || n_bins == 0) return PSA_OK;
    PSA_REQUIRE(n_species >= 1 && n_species <= PARTIAL_MAX_SPECIES, "1 to %d species are served, got %d", PARTIAL_MAX_SPECIES, n_species);
    PSA_REQUIRE(nb < (1ll << 31) && ns < (1ll << 31) && n_bins < (1ll << 24), "shell block too large");
    const int64_t P = (int64_t)n_species * (n_species + 1) / 2;
    const dim3 grid((unsigned)std::min<int64_t>((L + 255) / 256, 1024), (unsigned)std::min<int64_t>(n_bins * P, 65535)), block(256);
    if (currents)
        hipLaunchKernelGGL(partial_shell_kernel<4>, grid, block, 0, c->stream, d_seg, d_khat, d_bin_start, d_acc, L, (int)ns, g0,
                           (int)nb, (int)n_bins, n_species);
    else
        hipLaunchKernelGGL(partial_shell_kernel<1>, grid, block, 0, c->stream, d_seg, d_khat, d_bin_start, d_acc, L, (int)ns, g0,
                           (int)nb, (int)n_bins, n_species);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
