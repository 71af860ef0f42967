// Kernels of the solid-like cluster analysis (psa_solid_clusters, psa_debug_cluster_labels; definition: include/psa_hip.h,
// host side: api_cluster.hip): the connected components of the solid atoms over the neighbour lists that the neighbour pass
// (angle.hip) leaves, from the table of the Q_lm of the order solid_l that qlm_sum_kernel (qlm.hip) leaves.  Four passes on
// one stream, all integer but the bond test, which is psa_local_order's operation for operation (shell.h).
//
// cluster_bonds_kernel.  The items and the walk of shell.h; a wavefront takes a centre a, lane b its leg b.  The centre is
// left out by local_order_kernel's rules (the mark in Im Q of the first column; `incomplete` through the neighbours' marks).
// Else Q(a) 2^-40 goes to the wavefront's LDS stage, A = shell_norm2, lane b tests its bond; the ballot is the centre's
// mask in list order, xi its popcount.  parent[row] = the own column where xi >= min_connections, else -1; size[row] = 0.
// connections[65] and the four left-out kinds are counted per species with 32-bit integer LDS adds and leave through
// hist_reduce.hip.
//
// cluster_hook_kernel.  The same walk.  Lane b of a solid centre a takes the edge to its neighbour b where b is solid, b < a
// (both_ways: b != a, for lists that are not symmetric) and, with link 1, the mask bit is set: a lock-free union "larger
// root under smaller root" -- find both roots with path halving, CAS parent[hi] from hi to lo, on failure go on from the
// value the CAS returned.  parent[x] <= x always, so there is no cycle and a component's root is its smallest member:
// the labels do not depend on the order in which the edges arrive.  Workgroups on different XCDs touch the same words, so
// every access to `parent` in this kernel is a relaxed atomic of agent scope.  Every loop is bounded by n_a; a lane that
// runs out sets the error word.
//
// cluster_flatten_kernel.  A thread per (origin, column), after the launch boundary, so plain loads: label = the root, written
// over parent -- a thread that still walks through the word reads the old ancestor or the root, both lead to the root --,
// and size[origin, label] += 1 with one integer atomic add per distinct label of a wavefront.
//
// cluster_stats_kernel.  A workgroup takes up to CLUSTER_STATS_ORIGINS origins, one after the other: n_solid, n_clusters,
// largest and largest_label by wave reductions and integer LDS atomics, size_atoms written over size (a root writes its own
// value again, every other atom a word nobody else reads), the size histogram and large_atoms in 32-bit LDS counters that
// leave as a partial row through hist_reduce.hip.
//
// No float atomics; integer global atomics (CAS on parent, add on size) only: a minimum and integer sums, the same bits in
// any order.
#include "shell.h"

namespace psa {

namespace {

constexpr int CLUSTER_TAG_MASK = (1 << ANGLE_SPECIES_SHIFT) - 1;
constexpr int CLUSTER_STAGE = 2 * (ORDER_MAX_L + 1);
constexpr int CLUSTER_THREADS = 256;

// a counter of the stats pass holds at most the atoms of a workgroup's origins
static_assert(((uint64_t)CLUSTER_STATS_ORIGINS << ANGLE_SPECIES_SHIFT) <= (1ull << 32), "a workgroup's atoms fit 32 bits");
// ... and a counter of the bonds pass the centres of an item over the origins of a block
static_assert((uint64_t)64 * 65535 < (1ull << 32), "an item's samples fit 32 bits");

// Grid (items).  part[item][CLUSTER_ROW_WORDS]
__global__ void __launch_bounds__(ANGLE_CENTRES)
cluster_bonds_kernel(const int* __restrict__ count, const float4* __restrict__ list, const AngleItem* __restrict__ items,
                     const long long* __restrict__ q, unsigned* __restrict__ part, unsigned long long* __restrict__ mask_out,
                     int* __restrict__ xi_out, int* __restrict__ parent, int* __restrict__ size, int l, double thr2, int min_connections,
                     int n_a, int n_ob) {
    __shared__ unsigned hist[CLUSTER_ROW_WORDS];
    __shared__ double   stage[ANGLE_CENTRES / 64][CLUSTER_STAGE];          // per wavefront Q(a) 2^-40
    const AngleItem it = items[blockIdx.x];
    const int       V = 2 * (l + 1), at_out = ANGLE_MAX_NEIGHBOURS + 1;
    for (int i = threadIdx.x; i < CLUSTER_ROW_WORDS; i += ANGLE_CENTRES) hist[i] = 0u;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    double*   va = stage[wave];
    SHELL_WALK_FIRST(it, wave, n_a, n_ob);
    int   k_row = k;                                                       // the origin of the row on its way
    int   n_next = more ? count[row] : 0;
    float tag_next = more ? list[row * ANGLE_MAX_NEIGHBOURS + lane].w : 0.f;
    while (more) {
        const int     n = __builtin_amdgcn_readfirstlane(n_next);
        const int     tag = __float_as_int(tag_next);
        const int64_t cur = row, origin = (int64_t)k_row * n_a;
        SHELL_WALK_NEXT(it, wave, n_a, n_ob, (k_row = k, n_next = count[row], tag_next = list[row * ANGLE_MAX_NEIGHBOURS + lane].w))
        const bool    mine = lane < n && n <= ANGLE_MAX_NEIGHBOURS;
        const int64_t nrow = origin + (mine ? tag & CLUSTER_TAG_MASK : 0); // the neighbour's row, below (n_ob, n_a) by the neighbour pass
        int           out = n > ANGLE_MAX_NEIGHBOURS ? 0 : n == 0 ? 1 : -1;   // truncated, isolated: all or nothing
        if (out < 0 && q[cur * V + 1] != 0) out = 2;                       // undefined
        if (out < 0 && __any(mine && q[nrow * V + 1] != 0)) out = 3;       // incomplete: a neighbour without a vector
        if (out >= 0) {
            if (lane == 0) {
                atomicAdd(&hist[at_out + out], 1u);
                xi_out[cur] = -1, mask_out[cur] = 0ull, parent[cur] = -1, size[cur] = 0;
            }
            continue;
        }
        wave_sync();
        if (lane < V) va[lane] = __dmul_rn((double)q[cur * V + lane], SHELL_Q_EPS);
        wave_sync();
        const double             A = shell_norm2(va, l);
        const bool               solid = mine && shell_solid_bond(va, q + nrow * V, l, A, thr2);
        const unsigned long long bonds = __ballot(solid);
        const int                xi = __popcll(bonds);
        if (lane == 0) {
            atomicAdd(&hist[xi], 1u);
            xi_out[cur] = xi, mask_out[cur] = bonds, parent[cur] = xi >= min_connections ? (int)(cur - origin) : -1, size[cur] = 0;
        }
    }
    __syncthreads();
    unsigned* dst = part + (int64_t)blockIdx.x * CLUSTER_ROW_WORDS;
    for (int i = threadIdx.x; i < CLUSTER_ROW_WORDS; i += ANGLE_CENTRES) dst[i] = hist[i];
}

// `parent` inside the hook pass: relaxed, agent scope
__device__ __forceinline__ int hook_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void hook_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x (a solid column of the origin whose row 0 is `par`), halving the path on the way: x's word is replaced by
// an ancestor of x only, and only once x is no root, so no CAS on it can succeed afterwards.  Every step goes down: at most
// `bound` of them, else -1
__device__ __forceinline__ int hook_find(int* par, int x, int bound) {
    for (int s = 0; s < bound; ++s) {
        const int p = hook_load(par + x);
        if (p == x) return x;
        const int g = hook_load(par + p);
        if (g == p) return p;
        hook_store(par + x, g);
        x = g;
    }
    return -1;
}

// Grid (items)
__global__ void __launch_bounds__(ANGLE_CENTRES)
cluster_hook_kernel(const int* __restrict__ count, const float4* __restrict__ list, const AngleItem* __restrict__ items,
                    const unsigned long long* __restrict__ mask, int* parent, int* __restrict__ err, int link, int both_ways, int n_a,
                    int n_ob) {
    const AngleItem it = items[blockIdx.x];
    const int       wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    SHELL_WALK_FIRST(it, wave, n_a, n_ob);
    int   k_row = k;
    int   n_next = more ? count[row] : 0;
    float tag_next = more ? list[row * ANGLE_MAX_NEIGHBOURS + lane].w : 0.f;
    while (more) {
        const int     n = __builtin_amdgcn_readfirstlane(n_next);
        const int     tag = __float_as_int(tag_next);
        const int64_t cur = row, origin = (int64_t)k_row * n_a;
        SHELL_WALK_NEXT(it, wave, n_a, n_ob, (k_row = k, n_next = count[row], tag_next = list[row * ANGLE_MAX_NEIGHBOURS + lane].w))
        int*      par = parent + origin;
        const int ca = (int)(cur - origin);
        if (n == 0 || n > ANGLE_MAX_NEIGHBOURS || hook_load(par + ca) < 0) continue;   // no leg, or the centre is not solid
        const bool mine = lane < n;
        const int  cb = mine ? tag & CLUSTER_TAG_MASK : ca;                // the neighbour's column, below n_a by the neighbour pass
        bool       edge = mine && cb != ca && (both_ways || cb < ca) && (link == 0 || (mask[cur] >> lane & 1ull));
        edge = edge && hook_load(par + cb) >= 0;
        int  x = ca, y = cb;
        bool done = !edge;                                                 // (the lanes without an edge wait for the others)
        for (int t = 0; t < n_a && !done; ++t) {
            x = hook_find(par, x, n_a), y = hook_find(par, y, n_a);
            if (x < 0 || y < 0) break;
            if (x == y) {
                done = true;
                break;
            }
            const int hi = x > y ? x : y, lo = x > y ? y : x;
            int       seen = hi;
            done = __hip_atomic_compare_exchange_strong(par + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            x = seen, y = lo;                                              // (after a failure: hi's new parent, below hi)
        }
        if (!done) *err = 1;
    }
}

// Grid (tiles of CLUSTER_THREADS columns, origins)
__global__ void __launch_bounds__(CLUSTER_THREADS)
cluster_flatten_kernel(int* parent, int* __restrict__ size, int* __restrict__ err, int n_a) {
    const int     a = blockIdx.x * CLUSTER_THREADS + threadIdx.x, lane = threadIdx.x % 64;
    const int64_t origin = (int64_t)blockIdx.y * n_a;
    int*          par = parent + origin;
    int           lab = -1;
    if (a < n_a && par[a] >= 0) {
        int x = a, steps = 0;
        for (; steps < n_a; ++steps) {
            const int p = par[x];
            if (p == x) break;
            x = p;
        }
        if (steps == n_a) *err = 1;
        lab = x;
        par[a] = lab;
    }
    // one add per distinct label of the wavefront: the first lane still in the loop names a label, its lanes leave together
    bool todo = lab >= 0;
    while (todo) {
        const int                first = __builtin_amdgcn_readfirstlane(lab);
        const unsigned long long same = __ballot(lab == first);
        if (lab == first) {
            if (lane == __ffsll((long long)same) - 1) atomicAdd(size + origin + first, __popcll(same));
            todo = false;
        }
    }
}

// Grid (cluster_stat_groups).  part[workgroup][n_sizes + 3]; origin_out[origin][4]
__global__ void __launch_bounds__(CLUSTER_THREADS)
cluster_stats_kernel(const int* __restrict__ label, int* size, int* __restrict__ origin_out, unsigned* __restrict__ part, int n_sizes,
                     int n_a, int n_ob, int each) {
    __shared__ unsigned           hist[CLUSTER_MAX_SIZES + 3];
    __shared__ unsigned           n_solid, n_clusters;
    __shared__ unsigned long long best;                                    // size << 32 | ~label: the largest, then the smallest label
    const int words = n_sizes + 3, lane = threadIdx.x % 64;
    for (int i = threadIdx.x; i < words; i += CLUSTER_THREADS) hist[i] = 0u;
    const int k_end = min(n_ob, ((int)blockIdx.x + 1) * each);
    for (int k = blockIdx.x * each; k < k_end; ++k) {
        if (threadIdx.x == 0) n_solid = 0u, n_clusters = 0u, best = 0ull;
        __syncthreads();
        const int64_t      origin = (int64_t)k * n_a;
        long long          solid = 0, clusters = 0;
        unsigned long long mine = 0ull;
        for (int a = threadIdx.x; a < n_a; a += CLUSTER_THREADS) {
            const int lab = label[origin + a];
            const int s = lab >= 0 ? size[origin + lab] : 0;
            size[origin + a] = s;
            solid += lab >= 0;
            if (lab != a) continue;
            ++clusters;
            atomicAdd(&hist[s <= n_sizes ? s : n_sizes + 1], 1u);
            if (s > n_sizes) atomicAdd(&hist[n_sizes + 2], (unsigned)s);
            const unsigned long long key = (unsigned long long)s << 32 | (0xffffffffu - (unsigned)a);
            mine = key > mine ? key : mine;
        }
        solid = wave_sum(solid), clusters = wave_sum(clusters);
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long other = __shfl_xor(mine, o);
            mine = other > mine ? other : mine;
        }
        if (lane == 0) {
            atomicAdd(&n_solid, (unsigned)solid);
            atomicAdd(&n_clusters, (unsigned)clusters);
            atomicMax(&best, mine);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int* out = origin_out + (int64_t)k * 4;
            out[0] = (int)n_solid, out[1] = (int)n_clusters, out[2] = (int)(best >> 32);
            out[3] = best ? (int)(0xffffffffu - (unsigned)(best & 0xffffffffull)) : -1;
        }
        __syncthreads();
    }
    __syncthreads();
    unsigned* dst = part + (int64_t)blockIdx.x * words;
    for (int i = threadIdx.x; i < words; i += CLUSTER_THREADS) dst[i] = hist[i];
}

}  // namespace

int launch_cluster_bonds(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const long long* d_q,
                         unsigned* d_part, const ClusterWork& w, const LocalLs& ls, double thr2, int min_connections, int64_t n_a,
                         int64_t n_ob) {
    if (n_items == 0) return PSA_OK;
    PSA_REQUIRE(shell_grid_check(n_items, n_a, n_ob) && ls.n_l == 1 && ls.solid_l == ls.l_max && ls.columns == ls.l_max + 1 &&
                    ls.l_max >= 2 && ls.l_max <= ORDER_MAX_L && min_connections >= 0 && min_connections <= ANGLE_MAX_NEIGHBOURS,
                "cluster bonds pass outside its grid");
    hipLaunchKernelGGL(cluster_bonds_kernel, dim3((unsigned)n_items), dim3(ANGLE_CENTRES), 0, c->stream, d_count,
                       static_cast<const float4*>(d_list), static_cast<const AngleItem*>(d_items), d_q, d_part, w.mask, w.xi, w.parent, w.size,
                       ls.solid_l, thr2, min_connections, (int)n_a, (int)n_ob);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_cluster_hook(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const ClusterWork& w,
                        int link, bool both_ways, int* d_err, int64_t n_a, int64_t n_ob) {
    if (n_items == 0) return PSA_OK;
    PSA_REQUIRE(shell_grid_check(n_items, n_a, n_ob) && (link == 0 || link == 1), "cluster hook pass outside its grid");
    hipLaunchKernelGGL(cluster_hook_kernel, dim3((unsigned)n_items), dim3(ANGLE_CENTRES), 0, c->stream, d_count,
                       static_cast<const float4*>(d_list), static_cast<const AngleItem*>(d_items), w.mask, w.parent, d_err, link,
                       both_ways ? 1 : 0, (int)n_a, (int)n_ob);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_cluster_flatten(psa_ctx* c, const ClusterWork& w, int* d_err, int64_t n_a, int64_t n_ob) {
    if (n_a == 0 || n_ob == 0) return PSA_OK;
    PSA_REQUIRE(shell_grid_check(1, n_a, n_ob), "cluster flatten pass outside its grid");
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3((unsigned)((n_a + CLUSTER_THREADS - 1) / CLUSTER_THREADS), (unsigned)n_ob),
                       dim3(CLUSTER_THREADS), 0, c->stream, w.parent, w.size, d_err, (int)n_a);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_cluster_stats(psa_ctx* c, const ClusterWork& w, int* d_origin, unsigned* d_part, int n_sizes, int64_t n_a, int64_t n_ob) {
    if (n_a == 0 || n_ob == 0) return PSA_OK;
    PSA_REQUIRE(shell_grid_check(1, n_a, n_ob) && n_sizes >= 1 && n_sizes <= CLUSTER_MAX_SIZES, "cluster stats pass outside its grid");
    hipLaunchKernelGGL(cluster_stats_kernel, dim3((unsigned)cluster_stat_groups(n_ob)), dim3(CLUSTER_THREADS), 0, c->stream, w.parent, w.size,
                       d_origin, d_part, n_sizes, (int)n_a, (int)n_ob, (int)cluster_stat_each(n_ob));
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
