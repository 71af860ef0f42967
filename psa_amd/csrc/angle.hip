// Kernels of the bond-angle distributions and coordination statistics (psa_angle_histogram, psa_debug_neighbour_lists;
// definition: include/psa_hip.h, host side: api_angle.hip): the neighbour shell of every atom at every origin -- b in beta is
// a neighbour of a in alpha when b != a, r_cut[alpha,beta] > 0 and |mi(r_b - r_a)| < r_cut[alpha,beta] --, the histogram
// of the angle at a between every unordered pair of its neighbours and the histogram of its neighbour counts per species.
//
//   pair_frac (pair.hip)   positions -> c (origins of a block, 3, n_a) float32, the centred fractional coordinates
//   angle_neighbours       c -> per (origin, centre) the true neighbour count and the first 64 neighbours {d_x, d_y, d_z, tag}
//   angle_hist             the lists -> per-workgroup 32-bit histograms in LDS (angles, coordination, truncated) -> partials
//   hist_reduce (hist_reduce.hip)  the partials summed in 64-bit integers into the accumulator (S, row)
//
// Arithmetic.  The neighbour test is the displacement chain stated in pair.hip's header, through the same functions
// (min_image.h: min_image, radial_x), with dr = r_cut[alpha,beta]:
//     neighbour: x = __fmul_rn(__fsqrt_rn(r2), inv_rc) < 1                       inv_rc = float32(1 / r_cut)
// so with one cut-off the neighbours are bit for bit what pair.hip counts in bin 0 of dr = r_cut, n_r = 1.  The angle at a
// between the legs b and c, float32, every operation rounded once but the square root (v_sqrt_f32 behind __fsqrt_rn: within
// one ulp), from the stored d (r2 is formed again from d: the same bits):
//     dot = fma(d_z(b), d_z(c), fma(d_y(b), d_y(c), d_x(b) d_x(c)));   q = r2(b) r2(c);   cos = dot / sqrt(q)
// (shell.h: shell_r2, shell_cos -- order.hip's cosine is this one by construction: it calls the same two functions)
// clamped to [-1, 1]; every step is symmetric in b <-> c bit for bit.  The bin is the i with cedge[i + 1] < cos <=
// cedge[i] of the host's table cedge[i] = float32(cos(i pi / n_theta)) (cedge[0] = 1, cedge[n_theta] = -1), found by
// bisection of the table in LDS; cos = -1 is in the last bin; a cos that is not a number (r2 = 0, a coincident neighbour)
// goes to counter n_theta.
//
// Tiling.  Neighbour pass: the loop of pair_hist_kernel with another tail.  A workgroup of 256 lanes takes a tile of 256
// centres of one species, one per lane with c in registers, at one origin, and walks ALL beta-tiles of all species, staged
// in LDS as three rows and read four atoms at a time as broadcasts: the inner loop loads nothing from global memory.  A
// hit goes to the lane's own list; the count goes on counting beyond 64.  One writer per list: no atomic of any kind, and
// the list is in the order of the atom list.  Angle pass: a workgroup of four wavefronts takes an item of the host's table
// (64 centres of one species, a slab of origins) and a chunk of species pairs whose histograms fit the LDS; a wavefront
// takes a centre, its lanes load the list once (64 x 16 bytes, one coalesced read, issued while the centre before is
// counted: shell.h's centre walk) and lane j takes the pairs (j, j + m mod n), m = 1 .. n / 2, the partner's leg by
// cross-lane reads -- every unordered pair once (shell.h's leg-pair step).  Counts are 32-bit integer adds in LDS (the
// host keeps an item's samples below 2^32), written to partials with plain stores and summed in uint64: integer adds
// commute, so the counts are the same bits whatever the blocking and the order of the atoms in a species.
#include <algorithm>

#include "min_image.h"
#include "shell.h"

namespace psa {

namespace {

// One pair: is b a neighbour of a?  d is left in dx, dy, dz
__device__ inline bool angle_leg(float ax, float ay, float az, float bx, float by, float bz, const Box32& B, float inv_rc, float& dx,
                                 float& dy, float& dz) {
    const MinImage m = min_image(ax, ay, az, bx, by, bz, B);
    dx = m.dx, dy = m.dy, dz = m.dz;
    return radial_x(m.r2, inv_rc) < 1.f;                                   // (a value that is not a number: no neighbour)
}

// a hit goes to the lane's own list; the count goes on beyond the capacity
#define ANGLE_PUT(DX, DY, DZ, POS)                                                                             \
    {                                                                                                          \
        if (n < ANGLE_MAX_NEIGHBOURS) mine[n] = make_float4(DX, DY, DZ, __int_as_float((POS) | tag_hi));        \
        ++n;                                                                                                   \
    }
#define ANGLE_TRY(BX, BY, BZ, POS) \
    if (angle_leg(ax, ay, az, BX, BY, BZ, B, inv_rc, dx, dy, dz)) ANGLE_PUT(dx, dy, dz, POS)

// Grid (centre tiles of all species, origins of the block).  c (n_ob, 3, n_a); count (n_ob, n_a); list (n_ob, n_a, 64)
__global__ void __launch_bounds__(ANGLE_CENTRES)
angle_neighbours_kernel(const float* __restrict__ c, int* __restrict__ count, float4* __restrict__ list, const AngleSpecies sp,
                        const Box32 B, int n_a) {
    __shared__ __attribute__((aligned(16))) float sb[3][ANGLE_CENTRES];
    const int lane = threadIdx.x, k = blockIdx.y;
    int       al = 0;
    while (al + 1 < sp.S && (int)blockIdx.x >= sp.tile_first[al + 1]) ++al;
    const int    a_lo = sp.start[al] + ((int)blockIdx.x - sp.tile_first[al]) * ANGLE_CENTRES;
    const bool   active = a_lo + lane < sp.start[al + 1];
    const float* b = c + (int64_t)k * 3 * n_a;
    float        ax = 0.f, ay = 0.f, az = 0.f, dx, dy, dz;
    if (active) ax = b[a_lo + lane], ay = b[(int64_t)n_a + a_lo + lane], az = b[2 * (int64_t)n_a + a_lo + lane];
    float4* mine = list + ((int64_t)k * n_a + a_lo + lane) * ANGLE_MAX_NEIGHBOURS;
    int     n = 0;
    for (int be = 0; be < sp.S; ++be) {
        const float inv_rc = sp.inv_rc[al * sp.S + be];
        if (inv_rc == 0.f) continue;                                       // no bond between these species
        const int tag_hi = be << ANGLE_SPECIES_SHIFT;
        for (int bt = sp.start[be]; bt < sp.start[be + 1]; bt += ANGLE_CENTRES) {
            const int nb = min(ANGLE_CENTRES, sp.start[be + 1] - bt);
            __syncthreads();                                               // the last tile's reads have ended
            for (int j = 0; j < 3; ++j) sb[j][lane] = lane < nb ? b[(int64_t)j * n_a + bt + lane] : 0.f;
            __syncthreads();
            if (!active) continue;
            if (bt == a_lo) {                                              // the centre's own tile: b != a
                for (int i = 0; i < nb; ++i) {
                    if (i == lane) continue;
                    ANGLE_TRY(sb[0][i], sb[1][i], sb[2][i], bt + i)
                }
                continue;
            }
            int i = 0;
            for (; i + 4 <= nb; i += 4) {                                  // the inner loop: four beta-atoms per row read
                const float4 bx = *reinterpret_cast<const float4*>(&sb[0][i]);
                const float4 by = *reinterpret_cast<const float4*>(&sb[1][i]);
                const float4 bz = *reinterpret_cast<const float4*>(&sb[2][i]);
                float        d0[3], d1[3], d2[3], d3[3];
                const bool   h0 = angle_leg(ax, ay, az, bx.x, by.x, bz.x, B, inv_rc, d0[0], d0[1], d0[2]);
                const bool   h1 = angle_leg(ax, ay, az, bx.y, by.y, bz.y, B, inv_rc, d1[0], d1[1], d1[2]);
                const bool   h2 = angle_leg(ax, ay, az, bx.z, by.z, bz.z, B, inv_rc, d2[0], d2[1], d2[2]);
                const bool   h3 = angle_leg(ax, ay, az, bx.w, by.w, bz.w, B, inv_rc, d3[0], d3[1], d3[2]);
                if (!(h0 | h1 | h2 | h3)) continue;                        // the common case: no store, one branch
                if (h0) ANGLE_PUT(d0[0], d0[1], d0[2], bt + i)
                if (h1) ANGLE_PUT(d1[0], d1[1], d1[2], bt + i + 1)
                if (h2) ANGLE_PUT(d2[0], d2[1], d2[2], bt + i + 2)
                if (h3) ANGLE_PUT(d3[0], d3[1], d3[2], bt + i + 3)
            }
            for (; i < nb; ++i) ANGLE_TRY(sb[0][i], sb[1][i], sb[2][i], bt + i)
        }
    }
    if (active) count[(int64_t)k * n_a + a_lo + lane] = n;
}
#undef ANGLE_TRY
#undef ANGLE_PUT

// Grid (items, chunks of species pairs).  part[item][row]: P (n_theta + 1) angle counters (this workgroup: the pairs of its
// chunk), then S 65 coordination counters and the truncated centres (the workgroups of chunk 0)
__global__ void __launch_bounds__(ANGLE_CENTRES)
angle_hist_kernel(const int* __restrict__ count, const float4* __restrict__ list, const AngleItem* __restrict__ items,
                  const float* __restrict__ edges, unsigned* __restrict__ part, int S, int n_a, int n_ob, int n_theta, int per_chunk) {
    extern __shared__ unsigned hist[];                                     // per_chunk (n_theta + 1) counters: the launch's dynamic LDS
    __shared__ unsigned coord[PAIR_MAX_SPECIES * (ANGLE_MAX_NEIGHBOURS + 1) + 1];
    __shared__ float    cedge[ANGLE_MAX_BINS + 1];
    const AngleItem it = items[blockIdx.x];
    const int       P = S * (S + 1) / 2, n1 = n_theta + 1, p0 = blockIdx.y * per_chunk, np = min(per_chunk, P - p0);
    const int       n_coord = S * (ANGLE_MAX_NEIGHBOURS + 1) + 1;
    const bool      first = blockIdx.y == 0;
    for (int i = threadIdx.x; i < np * n1; i += ANGLE_CENTRES) hist[i] = 0u;
    for (int i = threadIdx.x; i < n_coord; i += ANGLE_CENTRES) coord[i] = 0u;
    for (int i = threadIdx.x; i < n1; i += ANGLE_CENTRES) cedge[i] = edges[i];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    // the wavefront's centres in turn, the next one's count and list on their way while this one is counted: every lane
    // loads a slot of the list whether it is filled or not (the slots are there; the lanes at and beyond n are masked)
    SHELL_WALK_FIRST(it, wave, n_a, n_ob);
    int    n_next = more ? count[row] : 0;
    float4 e_next = more ? list[row * ANGLE_MAX_NEIGHBOURS + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    while (more) {
        const int    n = __builtin_amdgcn_readfirstlane(n_next);
        const float4 e = e_next;
        SHELL_WALK_NEXT(it, wave, n_a, n_ob, (n_next = count[row], e_next = list[row * ANGLE_MAX_NEIGHBOURS + lane]))
        if (n > ANGLE_MAX_NEIGHBOURS) {                                // truncated: all or nothing
            if (first && lane == 0) atomicAdd(&coord[n_coord - 1], 1u);
            continue;
        }
        const int s = lane < n ? __float_as_int(e.w) >> ANGLE_SPECIES_SHIFT : -1;
        if (first)
            for (int be = 0; be < S; ++be) {
                const int m = __popcll(__ballot(s == be));
                if (lane == 0) atomicAdd(&coord[be * (ANGLE_MAX_NEIGHBOURS + 1) + m], 1u);
            }
        const float r2 = shell_r2(e);
        for (int m = 1; 2 * m <= n; ++m) {
            const int    src = shell_partner(lane, m, n);
            const float4 o = shell_partner_leg(e, r2, src);
            const int    os = __shfl(s, src);
            if (!shell_has_pair(lane, m, n)) continue;
            const int lo = min(s, os), hi = max(s, os), p = lo * S - lo * (lo - 1) / 2 + hi - lo - p0;
            if (p < 0 || p >= np) continue;
            float cs = shell_cos(e, r2, o);
            int         bin = n_theta;                                 // not a number: undefined
            if (cs == cs) {
                cs = fminf(1.f, fmaxf(-1.f, cs));
                int left = 0, right = n_theta;                         // cedge[left] >= cs, and cedge[right] < cs or right = n_theta
                while (right - left > 1) {
                    const int mid = (left + right) >> 1;
                    if (cedge[mid] >= cs) left = mid; else right = mid;
                }
                bin = left;
            }
            atomicAdd(&hist[p * n1 + bin], 1u);
        }
        }
    __syncthreads();
    unsigned* dst = part + (int64_t)blockIdx.x * ((int64_t)P * n1 + n_coord);
    for (int i = threadIdx.x; i < np * n1; i += ANGLE_CENTRES) dst[(int64_t)p0 * n1 + i] = hist[i];
    if (first)
        for (int i = threadIdx.x; i < n_coord; i += ANGLE_CENTRES) dst[(int64_t)P * n1 + i] = coord[i];
}

}  // namespace

int launch_angle_neighbours(psa_ctx* c, const float* d_c, int* d_count, void* d_list, const AngleSpecies& sp, const double* box,
                            int64_t n_a, int64_t n_ob) {
    const int64_t tiles = sp.tile_first[sp.S];
    if (tiles == 0 || n_ob == 0) return PSA_OK;
    PSA_REQUIRE(sp.S >= 1 && sp.S <= PAIR_MAX_SPECIES && n_a == sp.start[sp.S] && n_a < (1ll << ANGLE_SPECIES_SHIFT) && n_ob >= 1 &&
                    n_ob <= 65535, "neighbour pass outside its grid");
    hipLaunchKernelGGL(angle_neighbours_kernel, dim3((unsigned)tiles, (unsigned)n_ob), dim3(ANGLE_CENTRES), 0, c->stream, d_c, d_count,
                       static_cast<float4*>(d_list), sp, Box32(box), (int)n_a);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_angle_hist(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const float* d_edges,
                      unsigned* d_part, int32_t S, int64_t n_a, int64_t n_ob, int32_t n_theta) {
    if (n_items == 0) return PSA_OK;
    PSA_REQUIRE(shell_grid_check(n_items, n_a, n_ob) && S >= 1 && S <= PAIR_MAX_SPECIES && n_theta >= 1 && n_theta <= ANGLE_MAX_BINS,
                "angle pass outside its grid");
    const int P = S * (S + 1) / 2, per_chunk = std::min(P, ANGLE_HIST_WORDS / (n_theta + 1));
    hipLaunchKernelGGL(angle_hist_kernel, dim3((unsigned)n_items, (unsigned)((P + per_chunk - 1) / per_chunk)), dim3(ANGLE_CENTRES),
                       (size_t)per_chunk * (size_t)(n_theta + 1) * sizeof(unsigned), c->stream, d_count, static_cast<const float4*>(d_list), static_cast<const AngleItem*>(d_items), d_edges, d_part,
                       (int)S, (int)n_a, (int)n_ob, (int)n_theta, per_chunk);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
