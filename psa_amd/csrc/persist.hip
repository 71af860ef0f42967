// Kernels of the bond persistence (psa_bond_persistence; definition: include/psa_hip.h, host side: api_persist.hip): the pairs
// that the neighbour pass (angle.hip) lists at an origin o, tested again at the later frames o + f -- is the bond still
// alive (intermittent), has it been alive at every visited frame so far (continuous), how many of its bonds has a centre
// lost (the cage).
//
//   pair_frac (pair.hip)        positions -> c (origins of a block, 3, n_a) float32 at the origins, and again at o + f
//   angle_neighbours (angle.hip) c -> per (origin, centre) the true neighbour count and the first 64 neighbours
//   persist_tags                the lists -> tags (n_ob, n_a, 64) int32, the survivor mask of every centre (its n low bits,
//                               0 for a truncated centre): once per block
//   persist_step                per visited frame f, over the origins of the block with o + f <= T - 1: the alive mask of
//                               every centre, survivors &= alive, and at a listed lag the counts -> partials
//   hist_reduce (hist_reduce.hip)  the partials -- per item the counters of every listed lag -- summed in 64-bit integers
//
// Arithmetic.  alive(a, b, o, f): the displacement chain stated in pair.hip's header, through the same functions
// (min_image.h: min_image, radial_x) on the centred fractions of frame o + f, with float32(1 / r_break[alpha,beta]) in place
// of the reciprocal of r_cut: x < 1.  At f = 0 the chain is the one that listed the pair and the reciprocal is not larger,
// so every listed neighbour is alive.  The chain is odd in e bit for bit, so alive(a, b) = alive(b, a).
//
// Tiling.  The step pass runs once per visited frame, so it reads per centre the count (4 bytes), the 64 tags (256), the
// survivor mask (8) and per lane the lagged fractions of the centre and of its neighbour (24), and writes the two masks: the
// 1-KiB list of legs is read once per block, by persist_tags.  A workgroup of four wavefronts takes an item of the host's
// table, a wavefront a centre (shell.h's centre walk, the next centre's count, tag and survivors on their way while this
// one is tested), lane i < n its i-th neighbour; the ballot is the alive mask in list order.  Between two listed lags of a
// continuous call only the bonds that still survive are tested: nothing else can change.  At a listed lag the per-species
// popcounts of the list, of the alive mask and of the survivor mask and the centre's lost count go by 32-bit integer adds
// into the workgroup's counters in LDS (the host keeps an item's samples below 2^32), written to the item's partial with
// plain stores.  No float atomics, no global atomics: the same bits whatever the budget, the blocking and the order of the
// atoms inside a species.
#include "min_image.h"
#include "shell.h"

namespace psa {

namespace {

constexpr int PERSIST_TAG_MASK = (1 << ANGLE_SPECIES_SHIFT) - 1;

// the n low bits
__device__ __forceinline__ unsigned long long persist_low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

// Grid (rows of 4 centres).  list (rows, 64) float4 -> tags (rows, 64) int32; surv (rows): the n low bits, 0 where truncated
__global__ void __launch_bounds__(ANGLE_CENTRES)
persist_tags_kernel(const int* __restrict__ count, const float4* __restrict__ list, int* __restrict__ tags,
                    unsigned long long* __restrict__ surv, int64_t rows) {
    const int64_t row = (int64_t)blockIdx.x * (ANGLE_CENTRES / 64) + threadIdx.x / 64;
    const int     lane = threadIdx.x % 64;
    if (row >= rows) return;
    tags[row * ANGLE_MAX_NEIGHBOURS + lane] = __float_as_int(list[row * ANGLE_MAX_NEIGHBOURS + lane].w);
    if (lane == 0) {
        const int n = count[row];
        surv[row] = n > ANGLE_MAX_NEIGHBOURS ? 0ull : persist_low_bits(n);
    }
}

// Grid (items).  cl (n_ob, 3, n_a): the fractions at the lagged frames of the first n_ob origins of the block.  keep: AND
// the alive mask into surv (a continuous call); part not null: a listed lag -- alive_out (rows) and the lag's
// persist_row_words counters of every item, part[item part_stride ...], are written: per beta the bonds, the alive and the
// unbroken ones (S each), lost[65], the truncated centres
__global__ void __launch_bounds__(ANGLE_CENTRES)
persist_step_kernel(const int* __restrict__ count, const int* __restrict__ tags, const AngleItem* __restrict__ items,
                    const float* __restrict__ cl, unsigned long long* __restrict__ surv, unsigned long long* __restrict__ alive_out,
                    unsigned* __restrict__ part, int64_t part_stride, const AngleSpecies sp, const Box32 B, int n_a, int n_ob, int keep) {
    __shared__ unsigned hist[3 * PAIR_MAX_SPECIES + ANGLE_MAX_NEIGHBOURS + 2];
    __shared__ float    inv_rb[PAIR_MAX_SPECIES];
    const AngleItem it = items[blockIdx.x];
    const int       S = sp.S, words = 3 * S + ANGLE_MAX_NEIGHBOURS + 2, at_lost = 3 * S;
    const bool      counted = part != nullptr;
    for (int i = threadIdx.x; i < words; i += ANGLE_CENTRES) hist[i] = 0u;
    if (threadIdx.x < S) inv_rb[threadIdx.x] = sp.inv_rc[it.species * S + threadIdx.x];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    SHELL_WALK_FIRST(it, wave, n_a, n_ob);
    int                k_row = k;                                          // the origin of the row on its way
    int                n_next = more ? count[row] : 0;
    int                tag_next = more ? tags[row * ANGLE_MAX_NEIGHBOURS + lane] : 0;
    unsigned long long sv_next = more && keep ? surv[row] : 0ull;
    while (more) {
        const int                n = __builtin_amdgcn_readfirstlane(n_next);
        const int                tag = tag_next;
        const unsigned long long sv = sv_next;
        const int64_t            cur = row;
        const float*             f = cl + (int64_t)k_row * 3 * n_a;        // the lagged frame of this origin
        const int                a = (int)(cur - (int64_t)k_row * n_a);
        SHELL_WALK_NEXT(it, wave, n_a, n_ob, (k_row = k, n_next = count[row], tag_next = tags[row * ANGLE_MAX_NEIGHBOURS + lane],
                                              sv_next = keep ? surv[row] : 0ull))
        if (n > ANGLE_MAX_NEIGHBOURS) {                                    // truncated: all or nothing (surv is 0 already)
            if (counted && lane == 0) {
                atomicAdd(&hist[words - 1], 1u);
                alive_out[cur] = 0ull;
            }
            continue;
        }
        const bool mine = lane < n;
        // between two listed lags only a survivor's test can change anything
        const bool test = mine && (counted || (sv >> lane & 1ull));
        const int  b = test ? tag & PERSIST_TAG_MASK : a;                  // below n_a by the neighbour pass
        const int  be = mine ? tag >> ANGLE_SPECIES_SHIFT : -1;
        bool       up = false;
        if (test) {
            const float ax = f[a], ay = f[(int64_t)n_a + a], az = f[2 * (int64_t)n_a + a];
            const float bx = f[b], by = f[(int64_t)n_a + b], bz = f[2 * (int64_t)n_a + b];
            up = radial_x(min_image(ax, ay, az, bx, by, bz, B).r2, inv_rb[be]) < 1.f;
        }
        const unsigned long long alive = __ballot(up), left = sv & alive;
        if (keep && lane == 0 && left != sv) surv[cur] = left;
        if (!counted) continue;
        unsigned n_be = 0u, n_alive = 0u, n_left = 0u;                     // lane beta < S keeps species beta's counts
        for (int s = 0; s < S; ++s) {
            const unsigned long long of = __ballot(be == s);
            if (lane == s) n_be = __popcll(of), n_alive = __popcll(of & alive), n_left = __popcll(of & left);
        }
        if (lane < S) {
            if (n_be) atomicAdd(&hist[lane], n_be);
            if (n_alive) atomicAdd(&hist[S + lane], n_alive);
            if (n_left) atomicAdd(&hist[2 * S + lane], n_left);
        }
        if (lane == 0) {
            atomicAdd(&hist[at_lost + n - __popcll(alive)], 1u);
            alive_out[cur] = alive;
        }
    }
    if (!counted) return;
    __syncthreads();
    unsigned* dst = part + (int64_t)blockIdx.x * part_stride;
    for (int i = threadIdx.x; i < words; i += ANGLE_CENTRES) dst[i] = hist[i];
}

}  // namespace

int launch_persist_tags(psa_ctx* c, const int* d_count, const void* d_list, int* d_tags, unsigned long long* d_surv, int64_t n_a,
                        int64_t n_ob) {
    const int64_t rows = n_a * n_ob, groups = (rows + ANGLE_CENTRES / 64 - 1) / (ANGLE_CENTRES / 64);
    if (rows == 0) return PSA_OK;
    PSA_REQUIRE(n_a < (1ll << ANGLE_SPECIES_SHIFT) && n_ob >= 1 && n_ob <= 65535 && groups < (1ll << 31), "tag pass outside its grid");
    hipLaunchKernelGGL(persist_tags_kernel, dim3((unsigned)groups), dim3(ANGLE_CENTRES), 0, c->stream, d_count,
                       static_cast<const float4*>(d_list), d_tags, d_surv, rows);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_persist_step(psa_ctx* c, const int* d_count, const int* d_tags, const void* d_items, int64_t n_items, const float* d_cl,
                        unsigned long long* d_surv, unsigned long long* d_alive, unsigned* d_part, int64_t part_stride,
                        const AngleSpecies& rb, const double* box, int64_t n_a, int64_t n_ob, bool keep) {
    if (n_items == 0 || n_ob == 0) return PSA_OK;
    PSA_REQUIRE(shell_grid_check(n_items, n_a, n_ob) && rb.S >= 1 && rb.S <= PAIR_MAX_SPECIES && n_a == rb.start[rb.S] &&
                    part_stride >= persist_row_words(rb.S), "persistence pass outside its grid");
    hipLaunchKernelGGL(persist_step_kernel, dim3((unsigned)n_items), dim3(ANGLE_CENTRES), 0, c->stream, d_count, d_tags,
                       static_cast<const AngleItem*>(d_items), d_cl, d_surv, d_alive, d_part, part_stride, rb, Box32(box), (int)n_a,
                       (int)n_ob, keep ? 1 : 0);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
