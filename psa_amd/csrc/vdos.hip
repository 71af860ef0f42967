// Kernels of the vibrational density of states (psa_vdos; the definition is in psa_hip.h).  Unlike the SED path nothing
// is summed over atoms before the FFT: every selected atom's own series is transformed and the POWER is summed.
//
// Two real series share one complex FFT.  The selected atoms are listed in "pairs": both atoms of a pair belong to
// the same group, and component c of the pair is the complex series z = d_a + i d_b (an odd group's last pair has no b:
// its imaginary part is zero).  With Z = FFT(z), X_a[o] = (Z[o] + conj Z[L-o]) / 2 and X_b[o] = (Z[o] - conj Z[L-o]) / 2i,
// so  |X_a[o]|^2 + |X_b[o]|^2 = (|Z[o]|^2 + |Z[(L-o) mod L]|^2) / 2  -- and since both atoms add into the same
// accumulator row, the power pass never untangles: it sums |Z|^2 over all L bins and the last kernel folds o with L-o.
//
//   vdos_gather   resident (T,N,3) float32 -> work buffer (3, P_b, n_s, L) complex64 of one block of P_b pairs and
//                 n_s segments: mean subtraction (displacement mode), w_a, win[tau]; through an LDS tile, so that the
//                 reads run along (atom, component) and the writes along tau
//   [rocFFT]      in place, length L, batch 3 P_b n_s  (the complex plans of api_core.hip)
//   vdos_power    sum of |Z|^2 over a chunk of the rows of one (group, component), float64, into a partial buffer
//   vdos_reduce   the chunks' partials, in order, added to the float64 accumulator (G,3,L)
//   vdos_finish   out[g,c,o] = scale (acc[g,c,o] + acc[g,c,(L-o) mod L]), o = 0 .. L/2, float32
// Every accumulator element is written by one thread per launch and the launches follow each other on the context's
// stream: no atomics, the same bits on every run.
#include <algorithm>

#include "psa_ctx.h"

namespace psa {

constexpr int VDOS_TP = VDOS_TILE_PAIRS;    // pairs per gather tile (the unit of an atom block): 32
constexpr int VDOS_TC = VDOS_TP * 6;        // columns of a tile: 64 atoms x 3 components = 192 threads
constexpr int VDOS_TT = 64;                 // frames per gather tile
constexpr int VDOS_LD = VDOS_TT + 1;        // tile row pitch: column stores walk the 32 banks

// One workgroup: pairs [pt * 32, +32) of the block, frames [tt * 64, +64) of segment s0 + s.
//   read   thread j = column (atom slot j / 3, component j % 3): consecutive threads read consecutive floats of a frame
//          when the atoms are consecutive; the frames of the tile one after the other (independent loads)
//   write  each wavefront one (component, pair) row at a time: 64 consecutive complex values along tau
// Frame (s0 + s) H + tau <= (n_seg - 1) H + L - 1 <= T - 1; atoms were checked against N on the host.
__global__ void __launch_bounds__(VDOS_TC)
vdos_gather_kernel(const float* __restrict__ d, const float* __restrict__ mean, const float* __restrict__ weights,
                   const float* __restrict__ win, const int* __restrict__ pair_atoms, float2* __restrict__ work, int64_t N,
                   int64_t L, int64_t H, int64_t s0, int ns, int n_tt, int n_pairs) {
    __shared__ float tile[VDOS_TC * VDOS_LD];
    const int     j = threadIdx.x;
    const int     s = blockIdx.x / n_tt, tt = blockIdx.x % n_tt;
    const int     p_first = blockIdx.y * VDOS_TP;
    const int64_t tau0 = (int64_t)tt * VDOS_TT;
    const int     n_tau = (int)min((int64_t)VDOS_TT, L - tau0);

    const int q = j / 3, c = j - 3 * q;                  // atom slot of the tile, component
    const int p = p_first + (q >> 1);
    const int atom = p < n_pairs ? pair_atoms[2 * (int64_t)p + (q & 1)] : -1;
    float     m = 0.f, w = 0.f;
    if (atom >= 0) {
        w = weights ? weights[atom] : 1.f;
        if (mean) m = mean[(int64_t)atom * 3 + c];
    }
    const float* src = d + (((s0 + s) * H + tau0) * N + max(atom, 0)) * 3 + c;
    const int64_t frame = N * 3;
    if (atom >= 0) {
#pragma unroll 8
        for (int t = 0; t < n_tau; ++t) tile[j * VDOS_LD + t] = w * (src[(int64_t)t * frame] - m);
    } else {
        for (int t = 0; t < n_tau; ++t) tile[j * VDOS_LD + t] = 0.f;
    }
    __syncthreads();

    const int   lane = j & 63, wave = j >> 6;
    const float wt = lane < n_tau ? (win ? win[tau0 + lane] : 1.f) : 0.f;
    const int   rows = 3 * min(VDOS_TP, n_pairs - p_first);      // (pair, component) rows of this tile
    for (int r = wave; r < rows; r += VDOS_TC / 64) {
        const int rp = r / 3, rc = r - 3 * rp;
        if (lane < n_tau) {
            const float re = tile[((2 * rp) * 3 + rc) * VDOS_LD + lane], im = tile[((2 * rp + 1) * 3 + rc) * VDOS_LD + lane];
            const int64_t row = ((int64_t)rc * n_pairs + p_first + rp) * ns + s;
            work[row * L + tau0 + lane] = make_float2(wt * re, wt * im);
        }
    }
}

int launch_vdos_gather(psa_ctx* c, const float* d_data, const float* d_mean, const float* d_weights, const float* d_win,
                       const int* d_pair_atoms, float2* d_work, int64_t T, int64_t N, int64_t L, int64_t H, int64_t s0,
                       int64_t ns, int64_t n_pairs) {
    if (ns == 0 || n_pairs == 0) return PSA_OK;
    const int64_t n_tt = (L + VDOS_TT - 1) / VDOS_TT, gx = n_tt * ns, gy = (n_pairs + VDOS_TP - 1) / VDOS_TP;
    PSA_REQUIRE((s0 + ns - 1) * H + L <= T, "segment block outside the trajectory");
    PSA_REQUIRE(gx < (1ll << 31) && gy <= 65535 && n_pairs < (1ll << 30), "VDOS block too large");
    hipLaunchKernelGGL(vdos_gather_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(VDOS_TC), 0, c->stream, d_data, d_mean,
                       d_weights, d_win, d_pair_atoms, d_work, N, L, H, s0, (int)ns, (int)n_tt, (int)n_pairs);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

// After the FFT of the work buffer (3, n_pairs, ns, L).  blockIdx.x = ((group gl of the block, component), tile of 256
// bins), blockIdx.y = chunk: the pairs of group g_first + gl inside the block, pair_off[g] clipped to [p0, p0 + n_pairs), are consecutive
// rows of the buffer; the chunk takes its share of them.  part[chunk][gl][c][o] = sum over those rows of |Z[o]|^2.
__global__ void __launch_bounds__(256)
vdos_power_kernel(const float2* __restrict__ work, const int64_t* __restrict__ pair_off, double* __restrict__ part, int64_t L,
                  int ns, int n_pairs, int64_t p0, int g_first, int n_groups, int n_ot) {
    const int     gc = blockIdx.x / n_ot, ot = blockIdx.x - gc * n_ot;
    const int     gl = gc / 3, cc = gc - 3 * gl, chunk = blockIdx.y, n_chunks = gridDim.y;
    const int64_t lo = max(pair_off[g_first + gl], p0) - p0, hi = min(pair_off[g_first + gl + 1], p0 + n_pairs) - p0;
    const int64_t n_rows = max((int64_t)0, hi - lo) * ns, row0 = ((int64_t)cc * n_pairs + lo) * ns;
    const int64_t r_begin = n_rows * chunk / n_chunks, r_end = n_rows * (chunk + 1) / n_chunks;
    double*       dst = part + ((int64_t)chunk * n_groups * 3 + gc) * L;
    for (int64_t o = (int64_t)ot * 256 + threadIdx.x; o < L; o += (int64_t)n_ot * 256) {
        const float2* src = work + (row0 + r_begin) * L + o;
        double        sum = 0.0;
        int64_t       r = r_begin;
        for (; r + 4 <= r_end; r += 4) {
            const float2 v0 = src[0], v1 = src[L], v2 = src[2 * L], v3 = src[3 * L];
            src += 4 * L;
            sum += (double)v0.x * v0.x + (double)v0.y * v0.y;
            sum += (double)v1.x * v1.x + (double)v1.y * v1.y;
            sum += (double)v2.x * v2.x + (double)v2.y * v2.y;
            sum += (double)v3.x * v3.x + (double)v3.y * v3.y;
        }
        for (; r < r_end; ++r, src += L) {
            const float2 v = *src;
            sum += (double)v.x * v.x + (double)v.y * v.y;
        }
        dst[o] = sum;
    }
}

// acc[g_first + gl][c][o] += part[0][gl][c][o] + part[1][gl][c][o] + ...  (chunks in order)
__global__ void __launch_bounds__(256)
vdos_reduce_kernel(const double* __restrict__ part, double* __restrict__ acc, int64_t n, int n_chunks) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double sum = acc[i];
        for (int k = 0; k < n_chunks; ++k) sum += part[(int64_t)k * n + i];
        acc[i] = sum;
    }
}

int launch_vdos_power(psa_ctx* c, const float2* d_work, const int64_t* d_pair_off, double* d_part, double* d_acc, int64_t L,
                      int64_t ns, int64_t n_pairs, int64_t p0, int64_t g_first, int64_t n_groups, int64_t n_chunks) {
    if (ns == 0 || n_pairs == 0 || n_groups == 0) return PSA_OK;
    const int64_t n_ot = std::min<int64_t>((L + 255) / 256, 1 << 12), gx = n_ot * 3 * n_groups;
    PSA_REQUIRE(gx < (1ll << 31) && n_chunks >= 1 && n_chunks <= 65535 && ns < (1ll << 31), "VDOS block too large");
    hipLaunchKernelGGL(vdos_power_kernel, dim3((unsigned)gx, (unsigned)n_chunks), dim3(256), 0, c->stream, d_work, d_pair_off,
                       d_part, L, (int)ns, (int)n_pairs, p0, (int)g_first, (int)n_groups, (int)n_ot);
    PSA_HIP_CHECK(hipGetLastError());
    const int64_t n = n_groups * 3 * L;
    hipLaunchKernelGGL(vdos_reduce_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 16)), dim3(256), 0, c->stream,
                       d_part, d_acc + g_first * 3 * L, n, (int)n_chunks);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

// out (rows, F) float32, F = L/2 + 1, from acc (rows, L) float64: the one-sided fold of the header's definition
__global__ void __launch_bounds__(256)
vdos_finish_kernel(const double* __restrict__ acc, float* __restrict__ out, int64_t L, int64_t F, int64_t rows, double scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows * F; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / F, o = i - row * F;
        const double* a = acc + row * L;
        out[i] = (float)(scale * (a[o] + a[o ? L - o : 0]));
    }
}

int launch_vdos_finish(psa_ctx* c, const double* d_acc, float* d_out, int64_t L, int64_t rows, double scale) {
    const int64_t F = L / 2 + 1, n = rows * F;
    if (n == 0) return PSA_OK;
    hipLaunchKernelGGL(vdos_finish_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 16)), dim3(256), 0, c->stream,
                       d_acc, d_out, L, F, rows, scale);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
