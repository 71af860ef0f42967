// Kernels of the self (incoherent) dynamic structure factor on the reciprocal lattice of the box (psa_self_spectra;
// definition: include/psa_hip.h, host side: api_self.hip):
//
//     z[a,n,t] = w_a exp(2 pi i n.s_a(t))          density[o,n] = 1/(n_seg U L^2) sum_a sum_s |FFT_l(win[l] z[a,n,sH+l])[o]|^2
//
// Nothing is summed over atoms before the FFT: every (atom, vector) pair is a series of its own, N_g K of them where the
// coherent spectra have K.  What makes that affordable is the factorisation of lattice.hip, exp(2 pi i n.s) = E_1[n_1]
// E_2[n_2] E_3[n_3]: a sine and a cosine per (atom, frame, distinct (axis, m)), two complex products per unit.  The
// arithmetic of a term is lattice.hip's, through the same functions (lattice_math.h): lat_frac, lat_entry -- each entry
// directly from m, no recurrence --, lat_cmul; its error is that file's eps_lat.
//
//   self_series   resident positions -> work (na, nv, ns, L) complex64 of one block of na atoms, nv vectors, ns segments
//   [rocFFT]      in place, length L, batch na nv ns  (the complex plans of api_core.hip)
//   self_power    sum of |Z|^2 over the block's segments, an atom chunk and a column's vectors, float64, into partials
//   self_reduce   the chunks' partials, in order, added to the float64 accumulator (L, columns)
//   [lattice_finish_kernel]  scale in float64, one rounding to float32
//
// Series kernel.  A workgroup of SELF_THREADS = 256 lanes takes one atom tile (SELF_ATOMS = 4 atoms, one per wavefront),
// one frame tile (SELF_FRAMES = 64 consecutive frames of one segment, one per lane) and one vector tile of the host's plan (at most
// SELF_KS vectors that use R <= SELF_ENTRIES distinct (axis, m) pairs).  A lane
//   build    loads its atom's position in its frame (an index list is gathered here), forms (s_hi, s_lo)_j of the three
//            axes in registers, and evaluates the R entries tab[atom][e][frame] = (cos, sin)(2 pi m_e s_j(e)) into LDS;
//   series   per vector of the tile: reads its three entries, E = (E_1 E_2) E_3 in two float32 complex products, z = w_a E,
//            and stores win[l] z.  No sine, no cosine, no global load but the vector's three entry numbers (uniform) in
//            this loop.
// The table is laid out tab[entry][frame]: a wavefront's 64 lanes read 64 consecutive 8-byte words of a row -- one
// ds_read_b64 over all 64 four-byte banks twice, no conflict --, and a lane reads only what it wrote itself, so the kernel
// has no barrier.  SELF_ATOMS SELF_ENTRIES 512 B = 48 KiB of LDS: three workgroups per compute unit.  A wavefront's store
// is 64 consecutive complex64 of one row of the work buffer: 512 contiguous bytes.
// The position load is the kernel's one scattered access: a wavefront's lanes read 12 bytes each from 64 different frames, a
// stride of 3 N floats, so 64 cache lines per wavefront, shared only with the neighbouring atoms' wavefronts, and repeated
// for every vector tile and every segment.  It is amortised over up to SELF_KS stores and is the likely
// share of what the kernel takes above its store floor.
//
// Overlapping segments (hop < L).  A frame that belongs to several segments is evaluated once PER SEGMENT -- position,
// fractional coordinates, table --: a workgroup's frame tile is 64 frames of one segment.  The other form, evaluating a
// frame once per block and storing it once per segment that holds it with that segment's window value, was built first
// and both were measured on one problem (512 atoms, 64 vectors, 31 segments of 4096 at hop 2048, 4 and
// 31 segments per block): sharing 6.86 and 6.71 ms, re-evaluating 6.60 and 6.37 ms -- the evaluation is cheap beside up to
// 64 stores per lane, and sharing pays for it with a loop over a lane's segments, a second stream of stores and the
// 64-bit divisions that find the segments.  So frames are re-evaluated: the simpler kernel, and no slower.
//
// Error of a series element, before the window (what psa_debug_self_series returns and tests/self_cases.py bounds):
//     |z - z64| <= (eps_lat + c u) |w_a|,   c = 1,   u = 2^-24
// eps_lat (lattice.hip) covers the three entries and the two complex products; after them ONE float32 multiplication is
// applied per component, w_a E.  The window's multiplication follows it in the full path (a second u, inside the spectra's
// 1e-5 bar).  An element depends on (atom, frame, n) alone: the same bits however the call is cut into blocks and tiles.
//
// Power pass.  One lane per (column, frequency o), adjacent lanes adjacent o: the reads of a wavefront are 512 contiguous
// bytes of one transformed row, also at the mirror (L - o) mod L.  |Z|^2 is formed in float32 and summed in float64, vector
// by vector, atom by atom, segment by segment.  A column is one
// vector (per-vector form) or one shell's vectors with the mirror term (shell form: -n is n read at the mirrored
// frequency, as in lattice.hip).  Where columns x L cannot fill the device the block's atoms are split into chunks whose
// float64 partial sums are added in order (as vdos.hip does).  Every accumulator element is written by one lane per
// launch, the launches follow each other on the context's stream: no atomics, no float64 anywhere but these sums, the same
// bits on every run; another blocking regroups the float64 sums and may move the float32 result by one unit in the last
// place.
#include <algorithm>

#include "lattice_math.h"
#include "psa_ctx.h"

namespace psa {

namespace {

// Grid: (segments of the block x frame tiles of a segment, atom tiles of the block, vector tiles of the block).  tile
// (2 (tiles + 1)): per tile of the plan its offset into ent and its first vector of the processing order; slot: per vector
// its three entries.  Frame (s0 + s) H + l <= (s0 + ns - 1) H + L - 1 <= T - 1 (the launcher's check).
__global__ void __launch_bounds__(SELF_THREADS)
self_series_kernel(const float* __restrict__ pos, const float* __restrict__ wgt, const int* __restrict__ idx, int64_t a0,
                   const LatBox box, const int* __restrict__ tile, const unsigned short* __restrict__ ent,
                   const unsigned* __restrict__ slot, const float* __restrict__ win, float2* __restrict__ work, int64_t N, int na,
                   int tile0, int v0, int nv, int64_t L, int64_t H, int64_t s0, int ns, int n_ft, int64_t pitch) {
    __shared__ float2 tab[SELF_ATOMS][SELF_ENTRIES][SELF_FRAMES];
    const int     wave = threadIdx.x / SELF_FRAMES, lane = threadIdx.x % SELF_FRAMES;
    const int     tl = tile0 + blockIdx.z;
    const int     e0 = tile[2 * tl], R = tile[2 * tl + 2] - e0;            // 1 <= R <= SELF_ENTRIES (the host's plan)
    const int     p0 = tile[2 * tl + 1], nt = tile[2 * tl + 3] - p0;
    const int     al = blockIdx.y * SELF_ATOMS + wave;
    const int     s = blockIdx.x / n_ft;                                   // < ns: segment of the block
    const int64_t l = (int64_t)(blockIdx.x - s * n_ft) * SELF_FRAMES + lane, t = (s0 + s) * H + l;
    if (R < 1 || R > SELF_ENTRIES || al >= na || l >= L) return;
    float2 (*mine)[SELF_FRAMES] = tab[wave];

    // build
    const int64_t a = idx ? idx[a0 + al] : a0 + al;
    const int64_t o = (t * N + a) * 3;
    const float   w = wgt ? wgt[a] : 1.f;
    const float   x = pos[o], y = pos[o + 1], z = pos[o + 2];
    const float2  sx = lat_frac(x, y, z, box, 0), sy = lat_frac(x, y, z, box, 1), sz = lat_frac(x, y, z, box, 2);
    for (int e = 0; e < R; ++e) {
        const int    code = ent[e0 + e], axis = code >> 8;
        const float2 sj = axis == 0 ? sx : axis == 1 ? sy : sz;
        mine[e][lane] = lat_entry((float)((code & 255) - 128), sj);
    }

    // series
    const float wv = win ? win[l] : 1.f;
    float2*     dst = work + (((int64_t)al * nv + (p0 - v0)) * ns + s) * pitch + l;
    for (int v = 0; v < nt; ++v, dst += (int64_t)ns * pitch) {
        const unsigned u = slot[p0 + v];                                   // < R each
        const float2   E = lat_cmul(lat_cmul(mine[u & 511][lane], mine[(u >> 9) & 511][lane]), mine[(u >> 18) & 511][lane]);
        const float    re = __fmul_rn(w, E.x), im = __fmul_rn(w, E.y);
        *dst = make_float2(__fmul_rn(wv, re), __fmul_rn(wv, im));
    }
}

// After the FFT of work (na, nv, ns, L).  blockIdx.x = (column group gl of the block, tile of 256 frequencies), blockIdx.y
// = atom chunk.  part[chunk][gl][o] = sum over the group's vectors inside the block, the chunk's atoms and the segments.
template <bool MIRROR>
__global__ void __launch_bounds__(256)
self_power_kernel(const float2* __restrict__ work, const int* __restrict__ groups, double* __restrict__ part, int64_t L, int ns,
                  int na, int v0, int nv, int g_first, int ng, int n_ot) {
    const int     gl = blockIdx.x / n_ot, ot = blockIdx.x - gl * n_ot, chunk = blockIdx.y, n_chunks = gridDim.y;
    const int     g = g_first + gl;
    const int     k_lo = max(groups[2 * g], v0) - v0, k_hi = min(groups[2 * g + 2], v0 + nv) - v0;
    const int     a_lo = (int)((int64_t)na * chunk / n_chunks), a_hi = (int)((int64_t)na * (chunk + 1) / n_chunks);
    const int64_t row = (int64_t)ns * L;
    for (int64_t o = (int64_t)ot * 256 + threadIdx.x; o < L; o += (int64_t)n_ot * 256) {
        const int64_t om = o == 0 ? 0 : L - o;
        double        sum = 0.0;
        for (int k = k_lo; k < k_hi; ++k)
            for (int a = a_lo; a < a_hi; ++a) {
                const float2* src = work + ((int64_t)a * nv + k) * row;
                for (int s = 0; s < ns; ++s, src += L) {
                    const float2 f = src[o];
                    sum += (double)(f.x * f.x + f.y * f.y);
                    if constexpr (MIRROR) {
                        const float2 m = src[om];
                        sum += (double)(m.x * m.x + m.y * m.y);
                    }
                }
            }
        part[((int64_t)chunk * ng + gl) * L + o] = sum;
    }
}

// acc[o][column of group g_first + gl] += part[0][gl][o] + part[1][gl][o] + ...  (chunks in order)
__global__ void __launch_bounds__(256)
self_reduce_kernel(const double* __restrict__ part, const int* __restrict__ groups, double* __restrict__ acc, int64_t L, int g_first,
                   int ng, int64_t cols, int n_chunks) {
    const int64_t n = (int64_t)ng * L;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t gl = i / L, o = i - gl * L;
        double*       dst = acc + o * cols + groups[2 * (g_first + gl) + 1];
        double        sum = *dst;
        for (int k = 0; k < n_chunks; ++k) sum += part[(int64_t)k * n + i];
        *dst = sum;
    }
}

}  // namespace

int launch_self_series(psa_ctx* c, const float* d_pos, const float* d_weights, const int* d_idx, int64_t a0, const float* box_hi,
                       const float* box_lo, const int* d_tile, const unsigned short* d_ent, const unsigned* d_slot, const float* d_win,
                       float2* d_work, int64_t T, int64_t N, int64_t na, int64_t tile0, int64_t n_tiles, int64_t v0, int64_t nv,
                       int64_t L, int64_t H, int64_t s0, int64_t ns, int64_t pitch) {
    if (na == 0 || n_tiles == 0 || ns == 0) return PSA_OK;
    const int64_t n_ft = (L + SELF_FRAMES - 1) / SELF_FRAMES, gx = n_ft * ns, gy = (na + SELF_ATOMS - 1) / SELF_ATOMS;
    PSA_REQUIRE(L >= 1 && H >= 1 && s0 >= 0 && (s0 + ns - 1) * H + L <= T && pitch >= L, "segment block outside the trajectory");
    PSA_REQUIRE(gx < (1ll << 31) && gy <= 65535 && n_tiles <= 65535 && tile0 >= 0 && tile0 + n_tiles < (1ll << 30) && a0 >= 0 &&
                    a0 + na <= (1ll << 31) - 1 && N < (1ll << 31) && v0 >= 0 && v0 + nv < (1ll << 31) && ns < (1ll << 31),
                "self series outside its grid");
    LatBox box;
    for (int i = 0; i < 9; ++i) box.hi[i] = box_hi[i], box.lo[i] = box_lo[i];
    hipLaunchKernelGGL(self_series_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)n_tiles), dim3(SELF_THREADS), 0, c->stream, d_pos,
                       d_weights, d_idx, a0, box, d_tile, d_ent, d_slot, d_win, d_work, N, (int)na, (int)tile0, (int)v0, (int)nv, L, H, s0,
                       (int)ns, (int)n_ft, pitch);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_self_power(psa_ctx* c, const float2* d_work, const int* d_groups, double* d_part, double* d_acc, int64_t L, int64_t ns,
                      int64_t na, int64_t v0, int64_t nv, int64_t g_first, int64_t ng, int64_t cols, int64_t n_chunks, bool mirror) {
    if (ns == 0 || na == 0 || nv == 0 || ng == 0) return PSA_OK;
    const int64_t n_ot = std::min<int64_t>((L + 255) / 256, 1 << 12), gx = n_ot * ng;
    PSA_REQUIRE(gx < (1ll << 31) && n_chunks >= 1 && n_chunks <= 65535 && ns < (1ll << 31) && na < (1ll << 31) && v0 + nv < (1ll << 31) &&
                    g_first + ng < (1ll << 30),
                "self power block too large");
    const dim3 grid((unsigned)gx, (unsigned)n_chunks), block(256);
    if (mirror)
        hipLaunchKernelGGL(self_power_kernel<true>, grid, block, 0, c->stream, d_work, d_groups, d_part, L, (int)ns, (int)na, (int)v0,
                           (int)nv, (int)g_first, (int)ng, (int)n_ot);
    else
        hipLaunchKernelGGL(self_power_kernel<false>, grid, block, 0, c->stream, d_work, d_groups, d_part, L, (int)ns, (int)na, (int)v0,
                           (int)nv, (int)g_first, (int)ng, (int)n_ot);
    PSA_HIP_CHECK(hipGetLastError());
    const int64_t n = ng * L;
    hipLaunchKernelGGL(self_reduce_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 16)), dim3(256), 0, c->stream, d_part,
                       d_groups, d_acc, L, (int)g_first, (int)ng, cols, (int)n_chunks);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
