// Kernel of the adaptive common-neighbour analysis (psa_adaptive_common_neighbours; definition: include/psa_hip.h, host side:
// api_acna.hip; Stukowski, Modelling Simul. Mater. Sci. Eng. 20, 045021, 2012): every centre derives its own cut-off from its
// nearest candidates, and the signatures (j, k, l) of cna.hip are taken on its 12 nearest (fcc, hcp, ico) and, where that
// gives nothing, on its 14 nearest (bcc).  r_cut is a candidate radius only.
//
//   pair_frac (pair.hip)         positions -> c (origins of a block, 3, n_a) float32, the centred fractional coordinates
//   angle_neighbours (angle.hip) c -> per (origin, centre) the true candidate count and the first 64 candidates {d, tag}
//   acna_signature               c, the lists -> per centre its type (-1: truncated), its cut-off, optionally its members by
//                                rank and their bonds' signatures, and the signature table, the bonds outside it, the
//                                truncated and the short centres -> partials
//   cna_census (cna.hip)         the types -> (origin, species, 5) counts, one workgroup per origin
//   hist_reduce (hist_reduce.hip)  the partials summed in 64-bit integers into the accumulator (S, row)
//
// Arithmetic, float32, every operation rounded once but the root (v_sqrt_f32 behind __fsqrt_rn: within one ulp).
//     s_i = shell_r2(leg_i)                                the neighbour pass's r2, the same bits
//     rank(i) = #{j : s_j < s_i} + #{j < i : s_j = s_i}    exact compares, no root; a tie goes to the earlier list position
//     rho_k = __fsqrt_rn(s) of the candidate of rank k
//     test A (n >= 12): L = rho_0 + .. + rho_11 in ascending rank; r_A = __fmul_rn(L, float32(K / 12)), K = (1 + sqrt 2) / 2
//     test B (A gave other, n >= 14): P = rho_0 + .. + rho_7, Q = rho_8 + .. + rho_13, each in ascending rank;
//                                L = __fadd_rn(__fmul_rn(P, float32(2 / sqrt 3)), Q); r_B = __fmul_rn(L, float32(K / 14))
//     members u, v bonded: radial_x(min_image(frac_u, frac_v, B).r2, __fdiv_rn(1.f, r)) < 1
// The bond test is cna.hip's chain (min_image.h) on the same centred fractions, not a difference of legs (wrong beyond half
// a box); it is odd in e bit for bit, so the adjacency is symmetric; a value that is not a number is no bond.  Everything
// after the adjacency is integers.
//
// Tiling.  A workgroup of four wavefronts takes an item of the host's table, a wavefront a centre (shell.h's centre walk),
// lane i its i-th candidate, loaded as one float4 while the centre before is worked on.  Ranking: the 64 s_i are parked in
// the wavefront's LDS (+inf at and beyond n) and every lane reads them back four at a time as same-address broadcasts and
// counts -- no cross-lane shuffle.  A lane whose rank is below 14 writes {its three fractions gathered from c, its column}
// and rho to LDS slot `rank`; lanes 0 .. 13 then are the members.  The pairs of members go through shell.h's leg-pair rounds
// with n = 12 (six rounds), then where test B runs n = 14 (seven), each round's ballot taken as in cna.hip; lane u ends with
// row u of the adjacency as one 32-bit word, parked in LDS.  The flood and the type ballots are cna.hip's operations on 32-bit
// masks (this file keeps its own text of them: see DESIGN section 7).  The branch into test B is wave-uniform.  Counts are
// 32-bit integer adds in LDS (the host keeps an item's samples below 2^32), written to the item's partial with plain stores.
// No float atomics, no global atomics: the same bits whatever the budget and the blocking.
#include "min_image.h"
#include "shell.h"

namespace psa {

namespace {

constexpr int    ACNA_TAG_MASK = (1 << ANGLE_SPECIES_SHIFT) - 1;
constexpr int    ACNA_TABLE = CNA_MAX_J * CNA_MAX_K * CNA_MAX_L;           // the table; behind it: outside, truncated, short
constexpr double ACNA_K = 1.2071067811865475244;                           // (1 + sqrt 2) / 2
constexpr float  ACNA_SCALE_A = (float)(ACNA_K / 12.0), ACNA_SCALE_B = (float)(ACNA_K / 14.0);
constexpr float  ACNA_WEIGHT = (float)1.1547005383792515290;               // 2 / sqrt 3

__device__ __forceinline__ unsigned acna_word(int j, int k, int l) { return (unsigned)j | (unsigned)k << 8 | (unsigned)l << 16; }

// (j, k, l) of the bond to the member whose row is C, from the rows parked in LDS: one flood that pops every member of C once
__device__ __forceinline__ unsigned acna_flood(const unsigned* rows, unsigned C) {
    unsigned rem = C, frontier = 0u;
    int      k2 = 0, e2 = 0, best = 0;
    for (int pop = 0; pop < ACNA_MEMBERS && rem != 0u; ++pop) {
        if (frontier == 0u) {                                              // the piece has run dry: the next one starts
            best = max(best, e2), e2 = 0;
            frontier = rem & (0u - rem);
        }
        const int      at = __ffs((int)frontier) - 1;
        const unsigned bit = 1u << at;
        frontier &= ~bit, rem &= ~bit;
        const unsigned to = rows[at] & C;
        const int      deg = __popc(to);
        k2 += deg, e2 += deg;
        frontier |= to & rem;
    }
    best = max(best, e2);
    return acna_word(__popc(C), k2 >> 1, best >> 1);                       // (at most 13, 78, 78: nothing to clamp)
}

// Grid (items).  c (n_ob, 3, n_a); count, list as the neighbour pass leaves them; types, cut (n_ob, n_a); near, sigs (n_ob,
// n_a, 14) or both null; part[item][ACNA_ROW_WORDS]
__global__ void __launch_bounds__(ANGLE_CENTRES)
acna_signature_kernel(const float* __restrict__ c, const int* __restrict__ count, const float4* __restrict__ list,
                      const AngleItem* __restrict__ items, int* __restrict__ types, float* __restrict__ cut, int* __restrict__ near,
                      unsigned* __restrict__ sigs, unsigned* __restrict__ part, const Box32 box, int n_a, int n_ob) {
    __shared__ unsigned                                hist[ACNA_ROW_WORDS];
    __shared__ __attribute__((aligned(16))) float  keys[ANGLE_CENTRES / 64][ANGLE_MAX_NEIGHBOURS];
    __shared__ __attribute__((aligned(16))) float4 member[ANGLE_CENTRES / 64][ACNA_MEMBERS];
    __shared__ float                                   rho[ANGLE_CENTRES / 64][ACNA_MEMBERS];
    __shared__ unsigned                                rows[ANGLE_CENTRES / 64][ACNA_MEMBERS];
    __shared__ float                                   h[9];
    const AngleItem it = items[blockIdx.x];
    for (int i = threadIdx.x; i < ACNA_ROW_WORDS; i += ANGLE_CENTRES) hist[i] = 0u;
    if (threadIdx.x < 9) h[threadIdx.x] = box.h[threadIdx.x];
    __syncthreads();
    // Scalar registers are what this kernel is short of (the walk's state, nine pointers, the wave-uniform loops): as first
    // written it spilled 23 of them.  Four things below keep values in vector registers on purpose; none changes a result,
    // and each is to be re-checked against `SGPRs Spill` = 0 of tests/test_acna_resources.py when the compiler changes.
    // (1) The box: copied (Box32 has no default constructor) and overwritten at once from LDS, so that its nine words are
    // vector registers, not the kernel argument's scalar ones.
    Box32 B = box;
    for (int i = 0; i < 9; ++i) B.h[i] = h[i];
    // (2) The wavefront's number twice: `wave`, uniform, for the walk (shell.h's macros want it scalar), and `wv`, the same
    // value per lane, for the four LDS row pointers, which then are vector registers.
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    const int wv = threadIdx.x / 64;
    float*    key = keys[wv];
    float4*   mem = member[wv];
    float*    rh = rho[wv];
    unsigned* mine = rows[wv];
    unsigned* dst = part + (int64_t)blockIdx.x * ACNA_ROW_WORDS + threadIdx.x;
    SHELL_WALK_FIRST(it, wave, n_a, n_ob);
    int    k_row = k;                                                      // the origin of the row on its way
    int    n_next = more ? count[row] : 0;
    float4 e_next = more ? list[row * ANGLE_MAX_NEIGHBOURS + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    while (more) {
        const int     n = __builtin_amdgcn_readfirstlane(n_next);
        const float4  e = e_next;
        // (3) The places of this centre's outputs and of the lane's fractions, formed per lane before the walk moves on, so
        // that the row and the origin need no scalar copy across the body.  atom_at is the centre's cell in lane 0 alone,
        // and lane 0 alone stores through it (the other lanes' values are never used); b is below n_a in the held lanes
        // by the neighbour pass and is read in no other.
        const int     b = __float_as_int(e.w) & ACNA_TAG_MASK;
        const int64_t frac_at = (int64_t)k_row * 3 * n_a + b;              // the lane's candidate in the fractions of this origin
        const int64_t atom_at = row + lane, bond_at = row * ACNA_MEMBERS + lane;
        SHELL_WALK_NEXT(it, wave, n_a, n_ob, (k_row = k, n_next = count[row], e_next = list[row * ANGLE_MAX_NEIGHBOURS + lane]))
        int      type = 0, nm = 0, col = -1;
        float    r_loc = __int_as_float(0x7fc00000);                       // not a number: no test ran
        unsigned sig = 0xffffffffu;
        if (n > ANGLE_MAX_NEIGHBOURS) {                                    // truncated: all or nothing
            type = -1;
            if (lane == 0) atomicAdd(&hist[ACNA_TABLE + 1], 1u);
        } else if (n < ACNA_MEMBERS_A) {                                   // short: other, no bonds
            if (lane == 0) atomicAdd(&hist[ACNA_TABLE + 2], 1u);
        } else {
            // ---- the rank of this lane's candidate among the n
            const bool  held = lane < n;
            const float s = held ? shell_r2(e) : __int_as_float(0x7f800000);
            wave_sync();                                                   // the last centre's reads of the LDS have ended
            key[lane] = s;
            wave_sync();
            int rank = 0, ahead = lane;                                    // ahead: list positions from j up to this lane's
#pragma unroll 1                                                           // (4) unrolled, its compare masks spill scalar registers
            for (int j = 0; j < n; j += 4, ahead -= 4) {
                const float4 o = *reinterpret_cast<const float4*>(key + j);
                rank += (o.x < s || (o.x == s && ahead > 0)) + (o.y < s || (o.y == s && ahead > 1)) +
                        (o.z < s || (o.z == s && ahead > 2)) + (o.w < s || (o.w == s && ahead > 3));
            }
            // ---- the members: slot `rank` of the LDS takes the candidate's fractions, column and length
            if (held && rank < ACNA_MEMBERS) {
                mem[rank] = make_float4(c[frac_at], c[frac_at + n_a], c[frac_at + 2 * (int64_t)n_a], __int_as_float(b));
                rh[rank] = __fsqrt_rn(s);
            }
            wave_sync();
            float bx = 0.f, by = 0.f, bz = 0.f;
            if (lane < min(n, ACNA_MEMBERS)) {
                const float4 m = mem[lane];
                bx = m.x, by = m.y, bz = m.z, col = __float_as_int(m.w);
            }
            nm = ACNA_MEMBERS_A;
            for (;;) {
                // ---- the cut-off of this test from the members' lengths, in ascending rank
                if (nm == ACNA_MEMBERS_A) {
                    float L = rh[0];
                    for (int i = 1; i < ACNA_MEMBERS_A; ++i) L = __fadd_rn(L, rh[i]);
                    r_loc = __fmul_rn(L, ACNA_SCALE_A);
                } else {
                    float P = rh[0], Q = rh[8];
                    for (int i = 1; i < 8; ++i) P = __fadd_rn(P, rh[i]);
                    for (int i = 9; i < ACNA_MEMBERS; ++i) Q = __fadd_rn(Q, rh[i]);
                    r_loc = __fmul_rn(__fadd_rn(__fmul_rn(P, ACNA_WEIGHT), Q), ACNA_SCALE_B);
                }
                const float inv = __fdiv_rn(1.f, r_loc);
                // ---- the adjacency among the nm members: row `lane` of it
                unsigned adj = 0u;
#pragma unroll 1                                                           // (4) likewise: the rounds' ballots
                for (int m = 1; 2 * m <= nm; ++m) {
                    const int   src = shell_partner(lane, m, nm);
                    const float ox = __shfl(bx, src), oy = __shfl(by, src), oz = __shfl(bz, src);
                    bool        hit = false;
                    if (shell_has_pair(lane, m, nm)) hit = radial_x(min_image(bx, by, bz, ox, oy, oz, B).r2, inv) < 1.f;
                    const unsigned long long round = __ballot(hit);
                    int                      from = lane - m;              // the lane whose partner this one is
                    from = from < 0 ? from + nm : from;
                    if (lane < nm) {
                        if (round >> lane & 1ull) adj |= 1u << src;
                        if (round >> from & 1ull) adj |= 1u << from;
                    }
                }
                wave_sync();                                               // the last test's reads of the rows have ended
                if (lane < ACNA_MEMBERS) mine[lane] = adj;
                wave_sync();
                // ---- the signature of the bond a - member `lane`, the type of the centre
                sig = lane < nm ? acna_flood(mine, adj) : 0xffffffffu;
                if (nm == ACNA_MEMBERS_A) {
                    const int n421 = __popcll(__ballot(sig == acna_word(4, 2, 1))), n422 = __popcll(__ballot(sig == acna_word(4, 2, 2)));
                    const int n555 = __popcll(__ballot(sig == acna_word(5, 5, 5)));
                    type = n421 == 12 ? 1 : n421 == 6 && n422 == 6 ? 2 : n555 == 12 ? 4 : 0;
                } else {
                    const int n666 = __popcll(__ballot(sig == acna_word(6, 6, 6))), n444 = __popcll(__ballot(sig == acna_word(4, 4, 4)));
                    type = n666 == 8 && n444 == 6 ? 3 : 0;
                }
                if (type != 0 || nm == ACNA_MEMBERS || n < ACNA_MEMBERS) break;   // (wave-uniform)
                nm = ACNA_MEMBERS;
            }
            // ---- the bonds of the test that ran last are the centre's
            if (lane < nm) {
                const int nj = (int)(sig & 255u), nk = (int)(sig >> 8 & 255u), nl = (int)(sig >> 16);
                if (nj < CNA_MAX_J && nk < CNA_MAX_K && nl < CNA_MAX_L)
                    atomicAdd(&hist[(nj * CNA_MAX_K + nk) * CNA_MAX_L + nl], 1u);
                else
                    atomicAdd(&hist[ACNA_TABLE], 1u);
            }
        }
        if (lane == 0) types[atom_at] = type, cut[atom_at] = r_loc;
        if (near != nullptr && lane < ACNA_MEMBERS) {
            near[bond_at] = lane < nm ? col : -1;
            sigs[bond_at] = sig;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ACNA_ROW_WORDS; i += ANGLE_CENTRES, dst += ANGLE_CENTRES) *dst = hist[i];
}

}  // namespace

int launch_acna_signature(psa_ctx* c, const float* d_c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items,
                          int* d_types, float* d_cut, int* d_near, unsigned* d_sigs, unsigned* d_part, const double* box, int64_t n_a,
                          int64_t n_ob) {
    if (n_items == 0 || n_ob == 0) return PSA_OK;
    PSA_REQUIRE(shell_grid_check(n_items, n_a, n_ob) && (d_near == nullptr) == (d_sigs == nullptr), "adaptive signature pass outside its grid");
    hipLaunchKernelGGL(acna_signature_kernel, dim3((unsigned)n_items), dim3(ANGLE_CENTRES), 0, c->stream, d_c, d_count,
                       static_cast<const float4*>(d_list), static_cast<const AngleItem*>(d_items), d_types, d_cut, d_near, d_sigs, d_part,
                       Box32(box), (int)n_a, (int)n_ob);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
