// Kernels of the real-space self dynamics (psa_displacement_moments, psa_van_hove_self, psa_debug_unwrap; definition:
// include/psa_hip.h, host side: api_msd.hip): the unwrapped displacement u[t,a] of every atom, the moments of
// D = u[o + t] - u[o] summed directly over time origins o and atoms, and the histogram of |D|.
//
//   msd_unwrap_count   positions -> per (tile of MSD_UNWRAP_FRAMES frames, atom, axis) the int32 sum of the hops m
//   msd_unwrap_scan    exclusive scan of those sums over the tiles, one lane per (atom, axis)
//   msd_unwrap_write   positions + tile offsets -> u64 (n_a, 3, T) float64 (and, for psa_debug_unwrap, the image counts)
//   msd_moments        u64 -> float64 chunk sums (partials) of D_x^2, D_y^2, D_z^2, |D|^4 per lag
//   msd_moments_reduce the partials, in order, added to the float64 accumulator (n_lags, G, 4) that lives across blocks
//   msd_moments_finish scale by 1 / (N_g n_o(t)) in float64
//   msd_hist           u64 -> per-workgroup 32-bit histograms of floor(|D| / dr) in LDS -> partials
//   hist_reduce (hist_reduce.hip)  the partials summed in 64-bit integers into the accumulator (n_vh, G, n_r + 1)
//
// Unwrapping.  All of it float64 from the float32 positions.  For t >= 1, with e = r[t,a] - r[t-1,a] (exact in float64)
//     d_j = fma(e_z, Hinv[2][j], fma(e_y, Hinv[1][j], e_x Hinv[0][j]))      m_j = rint(d_j)      (ties to even)
//     n_j[t] = -(m_j[1] + ... + m_j[t])  (int32)
//     u_c[t] = fma(n_2, H[2][c], fma(n_1, H[1][c], fma(n_0, H[0][c], r_c[t,a] - r_c[0,a])))
// four roundings per element, so |u - u_exact| <= 4 2^-53 (|r(t) - r(0)| + sum_j |n_j| |H_jc|) (to first order).  The image
// counts are integer sums: the count kernel reduces a tile's hops over a wavefront, the scan adds the tiles, the write
// kernel takes the inclusive scan inside the tile -- integer adds, the same counts however the frames are cut.  A
// workgroup takes MSD_UNWRAP_ATOMS atoms x MSD_UNWRAP_FRAMES frames: it stages the frames' positions (and the frame
// before the tile) in LDS with consecutive lanes on consecutive floats of a frame -- an index list is gathered here --,
// then each wavefront takes its atoms one after the other with a lane per frame, so the store of u64 is 512 contiguous
// bytes of one (atom, component) row.  Both passes read the positions: 2 reads, one write of u64.
//
// Moments.  A workgroup of MSD_LAGS = 256 lanes takes a tile of MSD_LAGS lags (one per lane), a run of origin tiles and a
// chunk of atoms of one group.  An origin tile is NO = msd_origins(step) origins o_0 + k step; per atom it stages
//     org_c[k] = float32(u_c[o_0 + k step] - u_c[o_0])                      k < NO
//     win_c[j] = float32(u_c[o_0 + l_0 + j] - u_c[o_0])                     j < (NO - 1) step + MSD_LAGS <= MSD_WINDOW
// (l_0 the tile's first lag; the subtraction in float64, one rounding), so every staged value has the size of the
// atom's excursion since o_0, not of its total displacement.  Per (lag t = l_0 + lane, origin k):
//     D_c = win_c[k step + lane] - org_c[k]                                  (float32 subtraction)
//     q_x = D_x D_x, q_y = D_y D_y, q_z = D_z D_z                            (__fmul_rn)
//     r2  = fma(D_z, D_z, fma(D_y, D_y, q_x))                                (__fmaf_rn)
//     M2_c += (double)q_c,   M4 += (double)(r2 r2)                           (float64 adds, origins then atoms in order)
// Lanes on consecutive lags read consecutive words of win (no bank conflict); org is read as a broadcast, four origins
// per 16-byte read.  The chunk sums go to partials with plain stores, one workgroup per element; the reduce kernel adds
// a group's chunks in order.  No atomics: two identical calls give the same bits, another blocking regroups the float64
// sums.  LDS: 3 (MSD_WINDOW + MSD_ORIGINS) floats = 27 KiB: five workgroups per compute unit.
//
// Self van Hove.  The same D and r2 from values rounded like the staged ones, a_c = float32(u_c[o] - u_c[o_0]) and
// b_c = float32(u_c[o + tau] - u_c[o_0]) with the same origin tiles, D_c = b_c - a_c -- but read straight from u64, a
// lane per origin: a call has one lag per workgroup, so a staged value would be read once.  Then
//     r = __fsqrt_rn(r2),   x = __fmul_rn(r, inv_dr),   bin = x < n_r ? (int)floorf(x) : n_r    (inv_dr = float32(1 / dr))
// (min_image.h's radial_bin, the one pair.hip bins with)
// and a 32-bit integer add into the workgroup's histogram in LDS (n_r + 1 counters) -- the one place where this project
// uses LDS atomics: integer adds commute, so the counts are bit-identical whatever the order.  The host bounds a
// workgroup's samples below 2^32, the histogram goes to partials with plain stores, the reduce kernel sums in uint64.
#include <algorithm>

#include "min_image.h"
#include "msd_unit.h"
#include "psa_ctx.h"

namespace psa {

namespace {

struct MsdBox {
    double h[9], inv[9];   // H (rows = box vectors), Hinv
};

// the hops of one frame: rint of the fractional step, float64 (frame 0: none)
__device__ inline void msd_hops(const float* cur, const float* prev, const MsdBox& box, int m[3]) {
    const double ex = (double)cur[0] - (double)prev[0], ey = (double)cur[1] - (double)prev[1], ez = (double)cur[2] - (double)prev[2];
    for (int j = 0; j < 3; ++j)
        m[j] = (int)rint(__fma_rn(ez, box.inv[6 + j], __fma_rn(ey, box.inv[3 + j], __dmul_rn(ex, box.inv[j]))));
}

// frames [f0 - 1, f0 + MSD_UNWRAP_FRAMES) of atoms [a0, a0 + na) -> raw[frame - f0 + 1][atom][3]; frames outside [0, T): zeros
__device__ inline void msd_stage_positions(const float* __restrict__ pos, const int* __restrict__ idx, int64_t a_first, int na,
                                           int64_t f0, int64_t T, int64_t N, float (*raw)[MSD_UNWRAP_ATOMS * 3]) {
    for (int i = threadIdx.x; i < (MSD_UNWRAP_FRAMES + 1) * MSD_UNWRAP_ATOMS * 3; i += blockDim.x) {
        const int     fr = i / (MSD_UNWRAP_ATOMS * 3), e = i - fr * (MSD_UNWRAP_ATOMS * 3), al = e / 3;
        const int64_t t = f0 - 1 + fr;
        float         v = 0.f;
        if (al < na && t >= 0 && t < T) {
            const int64_t a = idx ? idx[a_first + al] : a_first + al;
            v = pos[(t * N + a) * 3 + (e - al * 3)];
        }
        raw[fr][e] = v;
    }
}

// Grid (frame tiles, atom tiles).  sums[tile][atom of the block][3]
__global__ void __launch_bounds__(256)
msd_unwrap_count_kernel(const float* __restrict__ pos, const int* __restrict__ idx, int64_t a0, int na, const MsdBox box,
                        int* __restrict__ sums, int64_t T, int64_t N) {
    __shared__ float raw[MSD_UNWRAP_FRAMES + 1][MSD_UNWRAP_ATOMS * 3];
    const int     wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int     at0 = blockIdx.y * MSD_UNWRAP_ATOMS, nat = min(MSD_UNWRAP_ATOMS, na - at0);
    const int64_t f0 = (int64_t)blockIdx.x * MSD_UNWRAP_FRAMES, t = f0 + lane;
    msd_stage_positions(pos, idx, a0 + at0, nat, f0, T, N, raw);
    __syncthreads();
    for (int al = wave; al < nat; al += 4) {
        int m[3] = {0, 0, 0};
        if (t >= 1 && t < T) msd_hops(&raw[lane + 1][al * 3], &raw[lane][al * 3], box, m);
        for (int j = 0; j < 3; ++j) {
            int s = m[j];
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
            if (lane == 0) sums[((int64_t)blockIdx.x * na + at0 + al) * 3 + j] = s;
        }
    }
}

// offs[tile][i] = sums[0][i] + ... + sums[tile - 1][i], i over the block's (atom, axis)
__global__ void __launch_bounds__(256)
msd_unwrap_scan_kernel(const int* __restrict__ sums, int* __restrict__ offs, int n_tiles, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int run = 0;
#pragma unroll 8
    for (int k = 0; k < n_tiles; ++k) {
        const int v = sums[(int64_t)k * n + i];
        offs[(int64_t)k * n + i] = run;
        run += v;
    }
}

// Grid as the count kernel's.  offs null: no image search (n = 0).  u (na, 3, T) float64; img (na, 3, T) int32 or null
__global__ void __launch_bounds__(256)
msd_unwrap_write_kernel(const float* __restrict__ pos, const int* __restrict__ idx, int64_t a0, int na, const MsdBox box,
                        const int* __restrict__ offs, double* __restrict__ u, int* __restrict__ img, int64_t T, int64_t N) {
    __shared__ float raw[MSD_UNWRAP_FRAMES + 1][MSD_UNWRAP_ATOMS * 3];
    const int     wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int     at0 = blockIdx.y * MSD_UNWRAP_ATOMS, nat = min(MSD_UNWRAP_ATOMS, na - at0);
    const int64_t f0 = (int64_t)blockIdx.x * MSD_UNWRAP_FRAMES, t = f0 + lane;
    msd_stage_positions(pos, idx, a0 + at0, nat, f0, T, N, raw);
    __syncthreads();
    for (int al = wave; al < nat; al += 4) {
        const int64_t a = idx ? idx[a0 + at0 + al] : a0 + at0 + al;
        int           n[3] = {0, 0, 0};
        if (offs) {
            int m[3] = {0, 0, 0};
            if (t >= 1 && t < T) msd_hops(&raw[lane + 1][al * 3], &raw[lane][al * 3], box, m);
            for (int j = 0; j < 3; ++j) {
                int s = m[j];                                              // inclusive scan over the wavefront's frames
                for (int d = 1; d < 64; d <<= 1) {
                    const int up = __shfl_up(s, d, 64);
                    if (lane >= d) s += up;
                }
                n[j] = -(offs[((int64_t)blockIdx.x * na + at0 + al) * 3 + j] + s);
            }
        }
        if (t >= T) continue;
        for (int c = 0; c < 3; ++c) {
            const double  e = (double)raw[lane + 1][al * 3 + c] - (double)pos[a * 3 + c];
            const int64_t o = ((int64_t)(at0 + al) * 3 + c) * T + t;
            u[o] = __fma_rn((double)n[2], box.h[6 + c], __fma_rn((double)n[1], box.h[3 + c], __fma_rn((double)n[0], box.h[c], e)));
            if (img) img[o] = n[c];
        }
    }
}

// (MsdUnit, msd_unit and MsdChunk -- the (lag, origin) unit and the chunk table's entry: msd_unit.h, shared with overlap.hip)

// Grid (lag tiles x origin slabs, chunks).  Origin tile j holds the origins (j NO + k) step, k < NO; slab s of n_os takes
// the tiles j = s, s + n_os, ...  part[(chunk n_os + slab)][lag][4]
__global__ void __launch_bounds__(MSD_LAGS)
msd_moments_kernel(const double* __restrict__ u, const MsdChunk* __restrict__ chunks, double* __restrict__ part, int64_t T,
                   int n_lags, int64_t step, int NO, int n_ot, int n_os) {
    __shared__ __attribute__((aligned(16))) float org[3][MSD_ORIGINS];
    __shared__ float win[3][MSD_WINDOW];
    const int      lt = blockIdx.x / n_os, slab = blockIdx.x - lt * n_os, lane = threadIdx.x;
    const int      l0 = lt * MSD_LAGS, t = l0 + lane;
    const int      t_hi = min(l0 + MSD_LAGS, n_lags) - 1;                  // the tile's largest lag in use
    const MsdChunk ch = chunks[blockIdx.y];
    const int      sw = NO > 1 ? (int)step : 0;                            // the origins' spacing in the window (one origin: unused)
    const int      W = (NO - 1) * sw + MSD_LAGS;                           // <= MSD_WINDOW (msd_origins)
    double         s_x = 0.0, s_y = 0.0, s_z = 0.0, s_4 = 0.0;
    for (int j = slab; j < n_ot; j += n_os) {
        const int64_t o0 = (int64_t)j * NO * step;
        // origins of the tile every lag in use has; some lag has; this lane's lag has (o + t <= T - 1)
        const auto    count = [&](int lag) -> int {
            const int64_t room = T - 1 - lag - o0;
            return room < 0 ? 0 : (int)min((int64_t)NO, room / step + 1);
        };
        const int k_all = count(t_hi), k_any = count(l0), k_mine = t < n_lags ? count(t) : 0;
        if (k_any == 0) break;                                             // later tiles hold fewer still
        for (int a = ch.a_lo; a < ch.a_hi; ++a) {
            const double* ua = u + (int64_t)a * 3 * T;
            __syncthreads();                                               // the last atom's reads have ended
            for (int c = 0; c < 3; ++c) {
                const double* uc = ua + (int64_t)c * T;
                const double  base = uc[o0];
                for (int k = lane; k < NO; k += MSD_LAGS) {
                    const int64_t f = o0 + (int64_t)k * step;
                    org[c][k] = f < T ? (float)(uc[f] - base) : 0.f;
                }
                for (int i = lane; i < W; i += MSD_LAGS) {
                    const int64_t f = o0 + l0 + i;
                    win[c][i] = f < T ? (float)(uc[f] - base) : 0.f;
                }
            }
            __syncthreads();
            const float* wx = win[0] + lane, *wy = win[1] + lane, *wz = win[2] + lane;
            int          k = 0;
            for (; k + 4 <= k_all; k += 4) {                               // the inner loop: four origins per org read
                const float4 ax = *reinterpret_cast<const float4*>(&org[0][k]);
                const float4 ay = *reinterpret_cast<const float4*>(&org[1][k]);
                const float4 az = *reinterpret_cast<const float4*>(&org[2][k]);
                const float  oxs[4] = {ax.x, ax.y, ax.z, ax.w}, oys[4] = {ay.x, ay.y, ay.z, ay.w}, ozs[4] = {az.x, az.y, az.z, az.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int     w = (k + i) * sw;
                    const MsdUnit q = msd_unit(wx[w], wy[w], wz[w], oxs[i], oys[i], ozs[i]);
                    s_x += (double)q.qx, s_y += (double)q.qy, s_z += (double)q.qz, s_4 += (double)__fmul_rn(q.r2, q.r2);
                }
            }
            for (; k < k_any; ++k) {                                       // the tile's edge: lanes drop out lag by lag
                if (k >= k_mine) continue;
                const int     w = k * sw;
                const MsdUnit q = msd_unit(wx[w], wy[w], wz[w], org[0][k], org[1][k], org[2][k]);
                s_x += (double)q.qx, s_y += (double)q.qy, s_z += (double)q.qz, s_4 += (double)__fmul_rn(q.r2, q.r2);
            }
        }
    }
    if (t < n_lags) {
        double* dst = part + (((int64_t)blockIdx.y * n_os + slab) * n_lags + t) * 4;
        dst[0] = s_x, dst[1] = s_y, dst[2] = s_z, dst[3] = s_4;
    }
}

// the chunks of group g are first[g] .. first[g + 1] - 1 of the table (the host lists them group by group)
struct MsdGroupChunks {
    int first[MSD_MAX_GROUPS + 1];
};

// acc[lag][group][4] += the partials of the group's chunks and slabs, in order
__global__ void __launch_bounds__(256)
msd_moments_reduce_kernel(const double* __restrict__ part, const MsdGroupChunks of, double* __restrict__ acc, int n_lags, int G,
                          int n_os) {
    const int64_t n = (int64_t)n_lags * G * 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int f = (int)(i % 4), g = (int)(i / 4 % G), lag = (int)(i / (4 * G));
        double    sum = acc[i];
        for (int64_t r = (int64_t)of.first[g] * n_os; r < (int64_t)of.first[g + 1] * n_os; ++r) sum += part[(r * n_lags + lag) * 4 + f];
        acc[i] = sum;
    }
}

// out[lag][group][4] = acc / (N_g n_o(lag)) in float64, an empty group: 0
__global__ void __launch_bounds__(256)
msd_moments_finish_kernel(const double* __restrict__ acc, const int64_t* __restrict__ group_size, double* __restrict__ out, int64_t T,
                          int n_lags, int G, int64_t step) {
    const int64_t n = (int64_t)n_lags * G * 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int     g = (int)(i / 4 % G), lag = (int)(i / (4 * G));
        const int64_t n_o = (T - 1 - lag) / step + 1, n_g = group_size[g];
        out[i] = n_g ? acc[i] / ((double)n_g * (double)n_o) : 0.0;
    }
}

// Grid (lags of the call x origin slabs, chunks); origin tiles and slabs as in the moments kernel, a lane per origin.
// part[(chunk n_os + slab)][lag j][n_r + 1] uint32: a workgroup's samples stay below 2^32 (the host's chunk rule)
__global__ void __launch_bounds__(256)
msd_hist_kernel(const double* __restrict__ u, const MsdChunk* __restrict__ chunks, const int64_t* __restrict__ lags,
                unsigned* __restrict__ part, int64_t T, int n_vh, int64_t step, int NO, int n_os, float inv_dr, int n_r) {
    __shared__ unsigned hist[MSD_MAX_BINS + 1];
    const int      j = blockIdx.x / n_os, slab = blockIdx.x - j * n_os;
    const int64_t  tau = lags[j], n_o = (T - 1 - tau) / step + 1;          // origins of this lag, >= 1
    const int64_t  n_ot = (n_o + NO - 1) / NO;
    const MsdChunk ch = chunks[blockIdx.y];
    for (int i = threadIdx.x; i <= n_r; i += 256) hist[i] = 0u;
    __syncthreads();
    const float edge = (float)n_r;
    for (int64_t tile = slab; tile < n_ot; tile += n_os) {
        const int64_t k0 = tile * NO, o0 = k0 * step;
        const int     nk = (int)min((int64_t)NO, n_o - k0);
        for (int a = ch.a_lo; a < ch.a_hi; ++a) {
            const double* ux = u + (int64_t)a * 3 * T, *uy = ux + T, *uz = uy + T;
            const double  bx = ux[o0], by = uy[o0], bz = uz[o0];
            for (int k = threadIdx.x; k < nk; k += 256) {
                const int64_t o = o0 + (int64_t)k * step, f = o + tau;     // f <= T - 1
                const MsdUnit q = msd_unit((float)(ux[f] - bx), (float)(uy[f] - by), (float)(uz[f] - bz), (float)(ux[o] - bx),
                                           (float)(uy[o] - by), (float)(uz[o] - bz));
                atomicAdd(&hist[radial_bin(q.r2, inv_dr, edge, n_r)], 1u);
            }
        }
    }
    __syncthreads();
    unsigned* dst = part + (((int64_t)blockIdx.y * n_os + slab) * n_vh + j) * (n_r + 1);
    for (int i = threadIdx.x; i <= n_r; i += 256) dst[i] = hist[i];
}

MsdBox msd_box(const double* box, const double* box_inverse) {
    MsdBox b;
    for (int i = 0; i < 9; ++i) b.h[i] = box[i], b.inv[i] = box_inverse[i];
    return b;
}

}  // namespace

int msd_origins(int64_t step) {
    return (int)std::min<int64_t>(MSD_ORIGINS, (MSD_WINDOW - MSD_LAGS) / step + 1);
}

int launch_msd_unwrap(psa_ctx* c, const float* d_pos, const int* d_idx, int64_t a0, int64_t na, const double* box,
                      const double* box_inverse, bool unwrap, int* d_sums, int* d_offs, double* d_u, int* d_img, int64_t T, int64_t N) {
    if (na == 0) return PSA_OK;
    const int64_t n_ft = (T + MSD_UNWRAP_FRAMES - 1) / MSD_UNWRAP_FRAMES, n_at = (na + MSD_UNWRAP_ATOMS - 1) / MSD_UNWRAP_ATOMS;
    PSA_REQUIRE(T >= 1 && n_ft < (1ll << 31) && n_at <= 65535 && a0 >= 0 && a0 + na <= (1ll << 31) - 1 && N < (1ll << 31),
                "unwrap pass outside its grid");
    const MsdBox b = msd_box(box, box_inverse);
    const dim3   grid((unsigned)n_ft, (unsigned)n_at), block(256);
    if (unwrap) {
        hipLaunchKernelGGL(msd_unwrap_count_kernel, grid, block, 0, c->stream, d_pos, d_idx, a0, (int)na, b, d_sums, T, N);
        PSA_HIP_CHECK(hipGetLastError());
        const int64_t n = na * 3;
        hipLaunchKernelGGL(msd_unwrap_scan_kernel, dim3((unsigned)((n + 255) / 256)), block, 0, c->stream, d_sums, d_offs, (int)n_ft, n);
        PSA_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(msd_unwrap_write_kernel, grid, block, 0, c->stream, d_pos, d_idx, a0, (int)na, b, unwrap ? d_offs : nullptr, d_u,
                       d_img, T, N);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_msd_moments(psa_ctx* c, const double* d_u, const void* d_chunks, int64_t n_chunks, double* d_part, int64_t T, int64_t n_lags,
                       int64_t step, int64_t n_os) {
    if (n_chunks == 0) return PSA_OK;
    const int     NO = msd_origins(step);
    const int64_t n_lt = (n_lags + MSD_LAGS - 1) / MSD_LAGS, n_ot = ((T - 1) / step + 1 + NO - 1) / NO;
    PSA_REQUIRE(n_lags >= 1 && n_lags <= T && step >= 1 && n_os >= 1 && n_os <= n_ot && n_lt * n_os < (1ll << 31) && n_chunks <= 65535 &&
                    n_ot < (1ll << 31) && n_lags < (1ll << 31) && (NO == 1 || (int64_t)(NO - 1) * step + MSD_LAGS <= MSD_WINDOW),
                "moments pass outside its grid");
    hipLaunchKernelGGL(msd_moments_kernel, dim3((unsigned)(n_lt * n_os), (unsigned)n_chunks), dim3(MSD_LAGS), 0, c->stream, d_u,
                       static_cast<const MsdChunk*>(d_chunks), d_part, T, (int)n_lags, step, NO, (int)n_ot, (int)n_os);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_msd_moments_reduce(psa_ctx* c, const double* d_part, const int32_t* group_first, double* d_acc, int64_t n_lags, int64_t n_os,
                              int32_t G) {
    if (group_first[G] == 0) return PSA_OK;
    MsdGroupChunks of = {};
    for (int g = 0; g <= G; ++g) of.first[g] = group_first[g];
    const int64_t n = n_lags * G * 4;
    hipLaunchKernelGGL(msd_moments_reduce_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 16)), dim3(256), 0, c->stream,
                       d_part, of, d_acc, (int)n_lags, (int)G, (int)n_os);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_msd_moments_finish(psa_ctx* c, const double* d_acc, const int64_t* d_group_size, double* d_out, int64_t T, int64_t n_lags,
                              int32_t G, int64_t step) {
    const int64_t n = n_lags * G * 4;
    hipLaunchKernelGGL(msd_moments_finish_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 16)), dim3(256), 0, c->stream,
                       d_acc, d_group_size, d_out, T, (int)n_lags, (int)G, step);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_msd_hist(psa_ctx* c, const double* d_u, const void* d_chunks, int64_t n_chunks, const int64_t* d_lags, int64_t n_vh,
                    unsigned* d_part, int64_t T, int64_t step, int64_t n_os, float inv_dr, int32_t n_r) {
    if (n_chunks == 0) return PSA_OK;
    PSA_REQUIRE(n_vh >= 1 && n_vh <= MSD_MAX_VH_LAGS && n_r >= 1 && n_r <= MSD_MAX_BINS && step >= 1 && n_os >= 1 &&
                    n_vh * n_os < (1ll << 31) && n_chunks <= 65535,
                "histogram pass outside its grid");
    hipLaunchKernelGGL(msd_hist_kernel, dim3((unsigned)(n_vh * n_os), (unsigned)n_chunks), dim3(256), 0, c->stream, d_u,
                       static_cast<const MsdChunk*>(d_chunks), d_lags, d_part, T, (int)n_vh, step, msd_origins(step), (int)n_os, inv_dr,
                       (int)n_r);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
