// Kernels of the common-neighbour analysis (psa_common_neighbours; definition: include/psa_hip.h, host side: api_cna.hip):
// per bond a-b_i of the neighbour pass's lists the signature (j, k, l) of Honeycutt-Andersen and Faken-Jonsson -- the common
// neighbours of a and b_i, the bonds among them, the bonds of the largest connected piece of those --, and per centre the
// structure type its bonds' signatures add up to (fcc, hcp, bcc, ico, other).
//
//   pair_frac (pair.hip)         positions -> c (origins of a block, 3, n_a) float32, the centred fractional coordinates
//   angle_neighbours (angle.hip) c -> per (origin, centre) the true neighbour count and the first 64 neighbours
//   cna_signature                c, the lists -> per centre its type (-1: truncated), optionally its bonds' signatures, and the
//                                signature table, the bonds outside it and the truncated centres -> partials
//   cna_census                   the types -> (origin, species, 5) counts, one workgroup per origin
//   hist_reduce (hist_reduce.hip)  the partials summed in 64-bit integers into the accumulator (S, row)
//
// Arithmetic.  Two listed neighbours b_i (species beta), b_j (gamma) of a are bonded when the neighbour pass's own chain holds
// for them at that origin, through the same functions (min_image.h: min_image, radial_x) on the same fractions:
//     x = __fmul_rn(__fsqrt_rn(r2), inv_rc[beta][gamma]) < 1,   inv_rc = float32(1 / r_cut), 0: no bond
// The chain is odd in e bit for bit and r_cut is symmetric, so the adjacency is symmetric, and it is "b_j is in b_i's list"
// wherever that list is complete; it asks for no list of the neighbour's, so a neighbour that is truncated itself changes
// nothing.  Everything after the adjacency is integers.
//
// Tiling.  A workgroup of four wavefronts takes an item of the host's table, a wavefront a centre (shell.h's centre walk, the
// next centre's count and tags on their way while this one is worked on), lane i < n its i-th neighbour, whose three
// fractions it gathers once.  The n (n - 1) / 2 pairs of neighbours go through shell.h's leg-pair rounds, m = 1 .. n / 2:
// lane i tests (i, i + m mod n), the partner's fractions and species by cross-lane reads; the round's ballot holds every
// tested pair once, and lane i takes from it its own bit (the partner's column) and the bit of the lane whose partner it is
// (that lane's column).  After the rounds lane i holds row i of the 64 x 64 adjacency as one uint64; the rows are parked in
// the wavefront's 512 bytes of LDS.  With C = row i (the common neighbours of a and b_i): j = popcount(C); one flood over
// masks pops every member c of C once, from the lowest bit of the frontier, and adds popcount(row c & C) to k2 and to the
// running piece's e2; a piece ends when its frontier runs dry; k = k2 / 2, l = max e2 / 2.  At most 64 pops, no shift by 64
// anywhere (the n low bits are never formed: the lanes at and beyond n park a row of zeros).  The type is five ballots.
// Counts are 32-bit integer adds in LDS (the host keeps an item's samples below 2^32), written to the item's partial with
// plain stores.  No float atomics, no global atomics: the same bits whatever the budget, the blocking and the order of the
// atoms inside a species.
#include "min_image.h"
#include "shell.h"

namespace psa {

namespace {

constexpr int CNA_TAG_MASK = (1 << ANGLE_SPECIES_SHIFT) - 1;
constexpr int CNA_TABLE = CNA_MAX_J * CNA_MAX_K * CNA_MAX_L;               // the table; behind it: outside, truncated
constexpr int CNA_CENSUS_THREADS = 256;

__device__ __forceinline__ unsigned cna_word(int j, int k, int l) { return (unsigned)j | (unsigned)k << 8 | (unsigned)l << 16; }

// Grid (items).  c (n_ob, 3, n_a); count, list as the neighbour pass leaves them; types (n_ob, n_a); sigs (n_ob, n_a, 64) or
// null; part[item][CNA_ROW_WORDS]
__global__ void __launch_bounds__(ANGLE_CENTRES)
cna_signature_kernel(const float* __restrict__ c, const int* __restrict__ count, const float4* __restrict__ list,
                     const AngleItem* __restrict__ items, int* __restrict__ types, unsigned* __restrict__ sigs,
                     unsigned* __restrict__ part, const AngleSpecies sp, const Box32 B, int n_a, int n_ob) {
    __shared__ unsigned           hist[CNA_ROW_WORDS];
    __shared__ unsigned long long rows[ANGLE_CENTRES / 64][64];
    __shared__ float              inv_rc[PAIR_MAX_SPECIES * PAIR_MAX_SPECIES];
    const AngleItem it = items[blockIdx.x];
    const int       S = sp.S;
    for (int i = threadIdx.x; i < CNA_ROW_WORDS; i += ANGLE_CENTRES) hist[i] = 0u;
    if (threadIdx.x < S * S) inv_rc[threadIdx.x] = sp.inv_rc[threadIdx.x];
    __syncthreads();
    const int           wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    unsigned long long* mine = rows[wave];
    // the tag is the fourth word of a list entry: the legs themselves are not read
    const int* tags = reinterpret_cast<const int*>(list) + 3;
    SHELL_WALK_FIRST(it, wave, n_a, n_ob);
    int k_row = k;                                                         // the origin of the row on its way
    int n_next = more ? count[row] : 0;
    int tag_next = more ? tags[(row * ANGLE_MAX_NEIGHBOURS + lane) * 4] : 0;
    while (more) {
        const int     n = __builtin_amdgcn_readfirstlane(n_next);
        const int     tag = tag_next;
        const int64_t cur = row;
        const float*  f = c + (int64_t)k_row * 3 * n_a;                    // the fractions of this origin
        SHELL_WALK_NEXT(it, wave, n_a, n_ob, (k_row = k, n_next = count[row], tag_next = tags[(row * ANGLE_MAX_NEIGHBOURS + lane) * 4]))
        if (n > ANGLE_MAX_NEIGHBOURS) {                                    // truncated: all or nothing
            if (lane == 0) {
                atomicAdd(&hist[CNA_TABLE + 1], 1u);
                types[cur] = -1;
            }
            if (sigs != nullptr) sigs[cur * ANGLE_MAX_NEIGHBOURS + lane] = 0xffffffffu;
            continue;
        }
        const bool held = lane < n;
        const int  b = held ? tag & CNA_TAG_MASK : 0;                      // below n_a by the neighbour pass
        const int  be = held ? tag >> ANGLE_SPECIES_SHIFT : 0;
        float      bx = 0.f, by = 0.f, bz = 0.f;
        if (held) bx = f[b], by = f[(int64_t)n_a + b], bz = f[2 * (int64_t)n_a + b];
        // ---- the adjacency among the neighbours: row `lane` of it
        unsigned long long adj = 0ull;
        for (int m = 1; 2 * m <= n; ++m) {
            const int   src = shell_partner(lane, m, n);
            const float ox = __shfl(bx, src), oy = __shfl(by, src), oz = __shfl(bz, src);
            const int   os = __shfl(be, src);
            bool        hit = false;
            if (shell_has_pair(lane, m, n)) {
                const float inv = inv_rc[be * S + os];
                hit = inv != 0.f && radial_x(min_image(bx, by, bz, ox, oy, oz, B).r2, inv) < 1.f;
            }
            const unsigned long long round = __ballot(hit);
            int                      from = lane - m;                      // the lane whose partner this one is
            from = from < 0 ? from + n : from;
            if (held) {
                if (round >> lane & 1ull) adj |= 1ull << src;
                if (round >> from & 1ull) adj |= 1ull << from;
            }
        }
        wave_sync();                                                       // the last centre's reads of the rows have ended
        mine[lane] = adj;
        wave_sync();
        // ---- the signature of the bond a - b_lane
        unsigned sig = 0xffffffffu;
        if (held) {
            const unsigned long long C = adj;
            unsigned long long       rem = C, frontier = 0ull;
            int                      k2 = 0, e2 = 0, best = 0;
            for (int pop = 0; pop < ANGLE_MAX_NEIGHBOURS && rem != 0ull; ++pop) {
                if (frontier == 0ull) {                                    // the piece has run dry: the next one starts
                    best = max(best, e2), e2 = 0;
                    frontier = rem & (0ull - rem);
                }
                const int                at = __ffsll((long long)frontier) - 1;
                const unsigned long long bit = 1ull << at;
                frontier &= ~bit, rem &= ~bit;
                const unsigned long long to = mine[at] & C;
                const int                deg = __popcll(to);
                k2 += deg, e2 += deg;
                frontier |= to & rem;
            }
            best = max(best, e2);
            const int nj = __popcll(C), nk = k2 >> 1, nl = best >> 1;
            // beyond 8 bits k and l are clamped in the word (such a bond lies outside the table in any case)
            sig = cna_word(nj, min(nk, 255), min(nl, 255));
            if (nj < CNA_MAX_J && nk < CNA_MAX_K && nl < CNA_MAX_L)
                atomicAdd(&hist[(nj * CNA_MAX_K + nk) * CNA_MAX_L + nl], 1u);
            else
                atomicAdd(&hist[CNA_TABLE], 1u);
        }
        if (sigs != nullptr) sigs[cur * ANGLE_MAX_NEIGHBOURS + lane] = sig;
        // ---- the type of the centre
        int type = 0;
        if (n == 12) {
            const int n421 = __popcll(__ballot(sig == cna_word(4, 2, 1))), n422 = __popcll(__ballot(sig == cna_word(4, 2, 2)));
            const int n555 = __popcll(__ballot(sig == cna_word(5, 5, 5)));
            type = n421 == 12 ? 1 : n421 == 6 && n422 == 6 ? 2 : n555 == 12 ? 4 : 0;
        } else if (n == 14) {
            const int n666 = __popcll(__ballot(sig == cna_word(6, 6, 6))), n444 = __popcll(__ballot(sig == cna_word(4, 4, 4)));
            type = n666 == 8 && n444 == 6 ? 3 : 0;
        }
        if (lane == 0) types[cur] = type;
    }
    __syncthreads();
    unsigned* dst = part + (int64_t)blockIdx.x * CNA_ROW_WORDS;
    for (int i = threadIdx.x; i < CNA_ROW_WORDS; i += ANGLE_CENTRES) dst[i] = hist[i];
}

// Grid (origins of the block).  types (n_ob, n_a) -> out[origin][species][5] uint64: per thread five counters in registers,
// a wave sum, one 32-bit integer add per wavefront, species and type in LDS (n_a < 2^28), plain stores
__global__ void __launch_bounds__(CNA_CENSUS_THREADS)
cna_census_kernel(const int* __restrict__ types, unsigned long long* __restrict__ out, const AngleSpecies sp, int n_a) {
    __shared__ unsigned cnt[PAIR_MAX_SPECIES * CNA_TYPES];
    const int           S = sp.S, lane = threadIdx.x % 64;
    if (threadIdx.x < S * CNA_TYPES) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int* t = types + (int64_t)blockIdx.x * n_a;
    for (int s = 0; s < S; ++s) {
        long long n[CNA_TYPES] = {0, 0, 0, 0, 0};
        for (int a = sp.start[s] + threadIdx.x; a < sp.start[s + 1]; a += CNA_CENSUS_THREADS) {
            const int ty = t[a];
            for (int j = 0; j < CNA_TYPES; ++j) n[j] += ty == j;
        }
        for (int j = 0; j < CNA_TYPES; ++j) {
            const long long all = wave_sum(n[j]);
            if (lane == 0 && all) atomicAdd(&cnt[s * CNA_TYPES + j], (unsigned)all);
        }
    }
    __syncthreads();
    if (threadIdx.x < S * CNA_TYPES) out[(int64_t)blockIdx.x * S * CNA_TYPES + threadIdx.x] = cnt[threadIdx.x];
}

}  // namespace

int launch_cna_signature(psa_ctx* c, const float* d_c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items,
                         int* d_types, unsigned* d_sigs, unsigned* d_part, const AngleSpecies& sp, const double* box, int64_t n_a,
                         int64_t n_ob) {
    if (n_items == 0 || n_ob == 0) return PSA_OK;
    PSA_REQUIRE(shell_grid_check(n_items, n_a, n_ob) && sp.S >= 1 && sp.S <= PAIR_MAX_SPECIES && n_a == sp.start[sp.S],
                "signature pass outside its grid");
    hipLaunchKernelGGL(cna_signature_kernel, dim3((unsigned)n_items), dim3(ANGLE_CENTRES), 0, c->stream, d_c, d_count,
                       static_cast<const float4*>(d_list), static_cast<const AngleItem*>(d_items), d_types, d_sigs, d_part, sp, Box32(box),
                       (int)n_a, (int)n_ob);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_cna_census(psa_ctx* c, const int* d_types, unsigned long long* d_out, const AngleSpecies& sp, int64_t n_a, int64_t n_ob) {
    if (n_a == 0 || n_ob == 0) return PSA_OK;
    PSA_REQUIRE(shell_grid_check(1, n_a, n_ob) && sp.S >= 1 && sp.S <= PAIR_MAX_SPECIES && n_a == sp.start[sp.S],
                "census pass outside its grid");
    hipLaunchKernelGGL(cna_census_kernel, dim3((unsigned)n_ob), dim3(CNA_CENSUS_THREADS), 0, c->stream, d_types, d_out, sp, (int)n_a);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
