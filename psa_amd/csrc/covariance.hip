// Spectral covariance of the B site groups' projections (psa_sed_covariance; definition: include/psa_hip.h, host side:
// api_covariance.hip): a reduction over frequency of the stacked transforms of one block of k-vectors,
//
//     G^(m)[k,i,j] = scale sum_w g_m[w] S_i[k,w] conj(S_j[k,w])        i, j = 3 b + c < n = 3 B,  m < n_w <= 2
//
// as a real rank-T update on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: four frequencies per instruction, rows
// padded to NB blocks of 16).  With X_r, X_i the real and imaginary planes (n x T),
//     Re G = X_r g X_r^T + X_i g X_i^T        Im G = X_i g X_r^T - X_r g X_i^T
// The A operand is a plane of row block I as it is, the B operand the plane of row block J times the weight -- and, for
// the second term of Im, times -1 --, rounded once to float32.  Only tile pairs J <= I are computed (NP = NB (NB + 1) / 2).
// Work split: a workgroup of four wavefronts takes one (k-vector, frequency chunk).  Every wavefront sums every tile
// pair -- the pair loop holds no condition, the accumulators never leave the MFMA's own registers -- of one part
// (wavefront w: part = w & 1, 0: Re, 1: Im; the part only selects which plane is which operand) and one slot
// (slot = w >> 1): with two weight rows the slot is the weight row, with one row it is every other chain of COV_CHAIN
// frequencies of the chunk (chain c belongs to slot c & 1).  So nothing is ever combined between wavefronts in float32:
// each (slot, pair, part) tile is summed by exactly one of them, and per four frequencies a wavefront reads its 2 NB
// operand values once, forms the 2 NB weighted ones and issues two MFMAs per tile pair (all first terms, then all second
// terms: neighbouring MFMAs are independent).
// Staging: COV_TILE = 64 frequencies of all n rows per step -- one 512-byte row read per wavefront and row, held in
// registers while the previous tile is consumed -- into an LDS image [row][COV_PITCH complex].  COV_PITCH = 66: the
// operand read of lane l is the 8 bytes of (row 16 R + (l & 15), frequency 4 s + (l >> 4)); a 32-lane half then covers
// dwords 4 (l & 15) + 2 (l >> 4) + {0, 1} of the 64 banks (132 mod 64 = 4): no two lanes on one bank.  Rows beyond n and
// frequencies beyond T are staged as zeros with weight zero.
// Summation structure (tests/cov64.py holds the kernel to the bound derived from it):
//   * a float32 accumulator (the MFMA's C/D) sums at most COV_CHAIN = 128 frequencies: per four frequencies the four
//     products of the first term in ascending frequency, then the four of the second, one FMA each -- a chain of
//     2 COV_CHAIN FMAs;
//   * it is then folded (one float32 addition) into a second float32 set, at most COV_FOLDS = 32 times;
//     (with one weight row a slot holds every other chain: at most COV_FOLDS / 2 folds);
//   * the workgroup writes that set as one partial slab per (k, frequency chunk of COV_CHUNK = COV_CHAIN COV_FOLDS = 4096
//     frequencies): [k][chunk][slot][pair][part][256 floats in accumulator order];
//   * covariance_finish_kernel sums a k-vector's slabs in ascending chunk order (with one weight row: slot 0, then slot 1
//     of each chunk) in float64, scales in float64, mirrors
//     (the upper triangle is the exact conjugate, the diagonal's imaginary part exact 0) and stores complex128.
// No atomics: the result depends neither on arrival order nor on how the k-vectors are blocked, and the chunking over
// w depends on T alone.
#include "psa_ctx.h"

namespace psa {

constexpr int COV_CHAIN = 128;                    // frequencies one float32 accumulator sums before it is folded
constexpr int COV_FOLDS = 32;                     // folds into the second float32 set per slab
constexpr int COV_CHUNK = COV_CHAIN * COV_FOLDS;  // frequencies per workgroup and slab
constexpr int COV_TILE = 64;                      // frequencies per staged tile
constexpr int COV_PITCH = COV_TILE + 2;           // complex values from one row of the LDS image to the next
constexpr int COV_MAX_BLOCKS = 6;                 // 16-row blocks served: n = 3 B <= 96

typedef float f32x4 __attribute__((ext_vector_type(4)));

int64_t covariance_chunks(int64_t T) { return (T + COV_CHUNK - 1) / COV_CHUNK; }
// floats of the slabs of one k-vector: two slots per chunk whatever n_w
int64_t covariance_slab_floats(int64_t T, int64_t n, int) {
    const int64_t nb = (n + 15) / 16;
    return covariance_chunks(T) * 2 * (nb * (nb + 1) / 2) * 2 * 256;
}

// One staged tile consumed by a wavefront: acc[p] += (first term) + (second term) over the tile's 64 frequencies, for
// every tile pair p.  part (uniform) selects the planes: Re: X_r (g X_r)^T + X_i (g X_i)^T;  Im: X_i (g X_r)^T + X_r (-g X_i)^T
template <int NB>
__device__ __forceinline__ void covariance_tile(const float2* __restrict__ img, const float* __restrict__ gw, f32x4 (&acc)[NB * (NB + 1) / 2],
                                                int lane, bool part) {
    const int r = lane & 15, q = lane >> 4;
#pragma unroll 2
    for (int s = 0; s < COV_TILE / 4; ++s) {
        const float g = gw[4 * s + q], gs = part ? -g : g;
        float       a0[NB], a1[NB], b0[NB], b1[NB];
#pragma unroll
        for (int R = 0; R < NB; ++R) {
            const float2 x = img[(16 * R + r) * COV_PITCH + 4 * s + q];
            a0[R] = part ? x.y : x.x;
            a1[R] = part ? x.x : x.y;
            b0[R] = g * x.x;
            b1[R] = gs * x.y;
        }
        int p = 0;
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = 0; J <= I; ++J, ++p) acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[I], b0[J], acc[p], 0, 0, 0);
        p = 0;
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = 0; J <= I; ++J, ++p) acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[I], b1[J], acc[p], 0, 0, 0);
    }
}

// S: (B, nk, 3, T) complex64, the unscaled transforms of one block of nk k-vectors; g: (n_w, T) float32; slab: the
// block's slabs [k][chunk][slot][pair][part][256].  Grid: nk n_chunks workgroups of 256 threads, blockIdx.x = k n_chunks + chunk.
template <int NB>
__global__ void __launch_bounds__(256)
covariance_kernel(const float2* __restrict__ S, const float* __restrict__ g, float* __restrict__ slab, int T, int nk, int n, int n_w,
                  int n_chunks) {
    constexpr int NP = NB * (NB + 1) / 2, ROWS = 16 * NB, PER = ROWS / 4;   // rows staged per wavefront
    __shared__ float2 img[ROWS * COV_PITCH];
    __shared__ float  gw[2][COV_TILE];
    __shared__ int64_t row_start[ROWS];
    const int  lane = threadIdx.x & 63;
    const int  wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool part = wave & 1;
    const int  slot = wave >> 1;
    const bool rows2 = n_w == 2;                                // the slot is a weight row; otherwise every other chain of row 0
    const int  m = rows2 ? slot : 0;
    const int  k = blockIdx.x / n_chunks, chunk = blockIdx.x - k * n_chunks;
    const int  w_begin = chunk * COV_CHUNK, w_end = (int)min((int64_t)T, (int64_t)w_begin + COV_CHUNK);   // T <= 2^31 - 64
    const int  n_tiles = (w_end - w_begin + COV_TILE - 1) / COV_TILE;

    // row i = 3 b + c of this k-vector starts at ((b nk + k) 3 + c) T (-1: a padding row, staged as zeros); the table is read
    // back per tile so that the 4 NB row starts of a wavefront are not held in registers.  Wavefront `wave` stages rows
    // wave, wave + 4, ...
    if (threadIdx.x < ROWS) {
        const int i = threadIdx.x, b = i / 3, cc = i - 3 * b;
        row_start[i] = i < n ? (int64_t)((((size_t)b * nk + k) * 3 + cc) * (size_t)T) : -1;
    }
    __syncthreads();
    float2 pre[PER];
    float  pre_g = 0.f;
    auto   fetch = [&](int tile) {
        const int w = w_begin + tile * COV_TILE + lane;
#pragma unroll
        for (int it = 0; it < PER; ++it) {
            const int64_t at = row_start[it * 4 + wave];
            pre[it] = (at >= 0 && w < w_end) ? S[at + w] : make_float2(0.f, 0.f);
        }
        if (wave < n_w) pre_g = w < w_end ? g[(size_t)wave * T + w] : 0.f;
    };
    f32x4 acc[NP], fold[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = fold[p] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    for (int tile = 0; tile < n_tiles; ++tile) {
#pragma unroll
        for (int it = 0; it < PER; ++it) img[(it * 4 + wave) * COV_PITCH + lane] = pre[it];
        if (wave < n_w) gw[wave][lane] = pre_g;
        __syncthreads();
        if (tile + 1 < n_tiles) fetch(tile + 1);               // in flight while this tile is consumed
        if (rows2 || ((tile / (COV_CHAIN / COV_TILE)) & 1) == slot) covariance_tile<NB>(img, gw[m], acc, lane, part);
        if ((tile + 1) % (COV_CHAIN / COV_TILE) == 0 || tile + 1 == n_tiles) {     // (a chain that was not this slot's adds zeros)
#pragma unroll
            for (int p = 0; p < NP; ++p) fold[p] += acc[p], acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
    }
    // lane l holds rows 4 (l >> 4) + reg, column l & 15 of a tile: stored as 256 floats [l][reg]
    float* out = slab + ((size_t)blockIdx.x * 2 + slot) * NP * 2 * 256;
#pragma unroll
    for (int p = 0; p < NP; ++p) *reinterpret_cast<f32x4*>(out + ((size_t)p * 2 + (part ? 1 : 0)) * 256 + lane * 4) = fold[p];
}

// out (n_w, K, n, n) complex128, k-vectors k_col0 .. k_col0 + nk - 1: scale x the float64 sum of the k-vector's slabs in
// ascending chunk order (weight row m is slot m of two rows, both slots in turn of one); [j][i] = conj [i][j],
// Im [i][i] = 0.  Grid (nk, n_w).
__global__ void __launch_bounds__(256)
covariance_finish_kernel(const float* __restrict__ slab, double2* __restrict__ out, int n, int n_w, int n_chunks, int np, int64_t K,
                         int64_t k_col0, double scale) {
    const int k = blockIdx.x, m = blockIdx.y;
    double2*  o = out + ((size_t)m * (size_t)K + (size_t)(k_col0 + k)) * (size_t)n * n;
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        if (j > i) continue;
        const int    I = i >> 4, J = j >> 4, p = I * (I + 1) / 2 + J, r = i & 15, col = j & 15;
        const int    at = (((r >> 2) * 16 + col) << 2) + (r & 3);
        const size_t slot_floats = (size_t)np * 2 * 256;
        const float* s = slab + ((size_t)k * n_chunks * 2 * np + p) * 2 * 256 + at;      // slot 0 of chunk 0
        double       re = 0.0, im = 0.0;
        for (int ch = 0; ch < n_chunks; ++ch, s += 2 * slot_floats)
            for (int sl = (n_w == 2 ? m : 0); sl <= (n_w == 2 ? m : 1); ++sl)
                re += (double)s[sl * slot_floats], im += (double)s[sl * slot_floats + 256];
        re *= scale, im *= scale;
        if (i == j) im = 0.0;
        o[(size_t)i * n + j] = make_double2(re, im);
        if (i != j) o[(size_t)j * n + i] = make_double2(re, -im);
    }
}

int launch_covariance(psa_ctx* c, const float2* d_S, const float* d_g, float* d_slab, double2* d_out, int64_t T, int64_t nk, int64_t B,
                      int n_w, int64_t K_pitch, int64_t k_col0, double scale) {
    if (nk == 0) return PSA_OK;
    const int64_t n = 3 * B, nb = (n + 15) / 16, n_chunks = covariance_chunks(T);
    PSA_REQUIRE(B >= 1 && nb <= COV_MAX_BLOCKS && T >= 1 && T <= (1ll << 31) - 64 && (n_w == 1 || n_w == 2) && nk <= 65535 * 4 &&
                    nk * n_chunks < (1ll << 31) && k_col0 >= 0 && k_col0 + nk <= K_pitch,
                "spectral covariance: block of %lld k-vectors x %lld frames, B = %lld, %d weight rows is out of range", (long long)nk,
                (long long)T, (long long)B, n_w);
    const dim3 grid((unsigned)(nk * n_chunks)), block(256);
    decltype(&covariance_kernel<1>) kernel = nullptr;
    switch ((int)nb) {
        case 1: kernel = covariance_kernel<1>; break;
        case 2: kernel = covariance_kernel<2>; break;
        case 3: kernel = covariance_kernel<3>; break;
        case 4: kernel = covariance_kernel<4>; break;
        case 5: kernel = covariance_kernel<5>; break;
        default: kernel = covariance_kernel<6>; break;
    }
    hipLaunchKernelGGL(kernel, grid, block, 0, c->stream, d_S, d_g, d_slab, (int)T, (int)nk, (int)n, n_w, (int)n_chunks);
    PSA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(covariance_finish_kernel, dim3((unsigned)nk, (unsigned)n_w), block, 0, c->stream, d_slab, d_out, (int)n, n_w,
                       (int)n_chunks, (int)(nb * (nb + 1) / 2), K_pitch, k_col0, scale);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
