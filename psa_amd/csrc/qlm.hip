// Kernels of the local order parameters that need the vectors q_lm themselves (psa_local_order, psa_debug_qlm; definition:
// include/psa_hip.h, host side: api_order.hip): the neighbour-averaged q-bar_l of Lechner and Dellago, the third-order
// invariants w_l and w-bar_l, and the solid-like bonds of ten Wolde, Ruiz-Montero and Frenkel, from the lists that the
// fraction pass (pair.hip) and the neighbour pass (angle.hip) leave -- per (origin, centre) the true neighbour count and up
// to 64 legs {d_x, d_y, d_z, tag}, the tag's low 28 bits the neighbour's row in the atom list.
//
// Two passes over the items of the angle pass, on one stream.
//
// qlm_sum_kernel.  A workgroup of four wavefronts takes an item; a wavefront takes a centre and lane b its leg b.  float64,
// every operation rounded once and none contracted (only __dmul_rn, __dadd_rn, __ddiv_rn, __dsqrt_rn):
//     x, y, z = (double) d_x, d_y, d_z;   r = sqrt(z z + (y y + x x));   u = (x / r, y / r, z / r)
//     c_0 = 1;   c_m = c_{m-1} (u_x + i u_y):   re = cr u_x + (-(ci u_y)),  im = cr u_y + ci u_x
//     Pi_mm = (2 m - 1)!!  (exact);   Pi_{m+1,m} = (2 m + 1)!! z;
//     Pi_lm = ((2 l - 1) (z Pi_{l-1,m}) + (-((l + m - 1) Pi_{l-2,m}))) / (l - m)
//     s = N_lm Pi_lm;   t_re = __double2ll_rn((s re) 2^40),  t_im = __double2ll_rn((s im) 2^40)
// N_lm = (-1)^m sqrt(1 / prod_{k = l-m+1 .. l+m} k) from the host's table (the Condon-Shortley phase is in it).  A 64-bit
// integer wave reduction per value; lane 0 stores Q_lm = sum_b t_lm(b), m = 0 .. l.  Nothing is accumulated across a loop
// and no array is indexed at run time: the recurrences carry two scalars, the column is an address.  A centre with more
// than 64 legs, with none or with a leg of length 0 gets zeros and the mark -1 in Im Q of its first column (0 otherwise:
// Y_l0 is real).
//
// local_order_kernel.  The same items; a wavefront takes a centre a.  Lane v (and v + 64) takes the value v of the row --
// (column, re | im) -- and walks the list in list order, adding q(b) = (Q(b) 2^-40) / n_b to q(a): q-bar = sum / (n + 1).
// Q(a) 2^-40 and q-bar go to the wavefront's LDS stage.  Per order: the sums of squares in ascending m (every lane the
// same), the 3j form with the dense table's entries dealt to the lanes in strides of 64 and a butterfly of __dadd_rn (a
// commutative operation: every lane ends with the same bits), the bond test with lane b on neighbour b.  The order of every
// sum is fixed by the list and the table, so a centre's result does not depend on the item, the block or the wavefront.
// The lanes 0, 1 and 2 count q-bar, w and w-bar with 32-bit integer LDS adds; the row leaves by plain stores and through hist_reduce.hip.  No global
// atomics, no float atomics.
#include "shell.h"

namespace psa {

namespace {

constexpr double LOCAL_ONE = (double)(1ll << LOCAL_SHIFT), LOCAL_EPS = 1.0 / LOCAL_ONE;
constexpr int    LOCAL_VALUES = 2 * LOCAL_MAX_COLUMNS;
constexpr int    LOCAL_TAG_MASK = (1 << ANGLE_SPECIES_SHIFT) - 1;

// Grid (items).  q[(origin of the block, centre)][column][re, im]
__global__ void __launch_bounds__(ANGLE_CENTRES)
qlm_sum_kernel(const int* __restrict__ count, const float4* __restrict__ list, const AngleItem* __restrict__ items,
               const double* __restrict__ norm, long long* __restrict__ q, const LocalLs ls, int n_a, int n_ob) {
    const AngleItem it = items[blockIdx.x];
    const int       wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    const int       V = 2 * ls.columns;
    SHELL_WALK_FIRST(it, wave, n_a, n_ob);
    int    n_next = more ? count[row] : 0;
    float4 e_next = more ? list[row * ANGLE_MAX_NEIGHBOURS + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    while (more) {
        const int     n = __builtin_amdgcn_readfirstlane(n_next);
        const float4  e = e_next;
        const int64_t cur = row;
        SHELL_WALK_NEXT(it, wave, n_a, n_ob, (n_next = count[row], e_next = list[row * ANGLE_MAX_NEIGHBOURS + lane]))
        long long*   out = q + cur * V;
        const bool   mine = lane < n;
        const double x = (double)e.x, y = (double)e.y, z = (double)e.z;
        const double r2 = __dadd_rn(__dmul_rn(z, z), __dadd_rn(__dmul_rn(y, y), __dmul_rn(x, x)));
        if (n > ANGLE_MAX_NEIGHBOURS || n == 0 || __any(mine && r2 == 0.0)) {      // left out: zeros and the mark
            for (int v = lane; v < V; v += 64) out[v] = v == 1 ? -1ll : 0ll;
            continue;
        }
        const double r = __dsqrt_rn(r2);
        const double ux = mine ? __ddiv_rn(x, r) : 0.0, uy = mine ? __ddiv_rn(y, r) : 0.0, uz = mine ? __ddiv_rn(z, r) : 1.0;
        double       cr = 1.0, cim = 0.0, pmm = 1.0;                               // (u_x + i u_y)^m, (2 m - 1)!!
        for (int m = 0; m <= ls.l_max; ++m) {
            if (m > 0) {
                const double nr = __dadd_rn(__dmul_rn(cr, ux), -__dmul_rn(cim, uy));
                const double ni = __dadd_rn(__dmul_rn(cr, uy), __dmul_rn(cim, ux));
                cr = nr, cim = ni;
                pmm = __dmul_rn(pmm, (double)(2 * m - 1));
            }
            double p2 = 0.0, p1 = 0.0;                                             // Pi_{l-2,m}, Pi_{l-1,m}
            int    base = 0;
            for (int l = 0; l <= ls.l_max; ++l) {
                if (l >= m) {
                    double p;
                    if (l == m) p = pmm;
                    else if (l == m + 1) p = __dmul_rn(__dmul_rn(pmm, (double)(2 * m + 1)), uz);
                    else p = __ddiv_rn(__dadd_rn(__dmul_rn((double)(2 * l - 1), __dmul_rn(uz, p1)), -__dmul_rn((double)(l + m - 1), p2)),
                                       (double)(l - m));
                    p2 = p1, p1 = p;
                }
                if (!(ls.mask >> l & 1u)) continue;
                if (l >= m) {
                    const double    s = __dmul_rn(norm[l * (ORDER_MAX_L + 1) + m], p1);
                    const long long tr = mine ? __double2ll_rn(__dmul_rn(__dmul_rn(s, cr), LOCAL_ONE)) : 0ll;
                    const long long ti = mine ? __double2ll_rn(__dmul_rn(__dmul_rn(s, cim), LOCAL_ONE)) : 0ll;
                    const long long sr = wave_sum(tr), si = wave_sum(ti);
                    if (lane == 0) out[2 * (base + m)] = sr, out[2 * (base + m) + 1] = si;
                }
                base += l + 1;
            }
        }
    }
}

// v_m of a staged vector (re, im pairs, m = 0 .. l): v_{-m} = (-1)^m conj v_m
__device__ inline void local_component(const double* v, int m, double* re, double* im) {
    const int    am = m < 0 ? -m : m;
    const double a = v[2 * am], b = v[2 * am + 1];
    const bool   flip = m < 0 && (am & 1);
    *re = flip ? -a : a;
    *im = (m < 0) != flip ? -b : b;
}

// Re(v_m1 v_m2 v_m3)
__device__ inline double local_triple(const double* v, int m1, int m2, int m3) {
    double ar, ai, br, bi, cr, ci;
    local_component(v, m1, &ar, &ai);
    local_component(v, m2, &br, &bi);
    local_component(v, m3, &cr, &ci);
    const double pr = __dadd_rn(__dmul_rn(ar, br), -__dmul_rn(ai, bi)), pi = __dadd_rn(__dmul_rn(ar, bi), __dmul_rn(ai, br));
    return __dadd_rn(__dmul_rn(pr, cr), -__dmul_rn(pi, ci));
}

// sum_{m = -l .. l} |v_m|^2 = |v_0|^2 + 2 sum_{m > 0} |v_m|^2, ascending m
__device__ inline double local_norm2(const double* v, int l) {
    double s = 0.0;
    for (int m = 0; m <= l; ++m) {
        const double t = __dadd_rn(__dmul_rn(v[2 * m], v[2 * m]), __dmul_rn(v[2 * m + 1], v[2 * m + 1]));
        s = __dadd_rn(s, m ? __dmul_rn(2.0, t) : t);
    }
    return s;
}

// Grid (items).  part[item][row]: the layout of local_row_words
__global__ void __launch_bounds__(ANGLE_CENTRES)
local_order_kernel(const int* __restrict__ count, const float4* __restrict__ list, const AngleItem* __restrict__ items,
                   const long long* __restrict__ q, const double* __restrict__ w3j, unsigned* __restrict__ part,
                   double* __restrict__ atoms_out, int* __restrict__ xi_out, const LocalLs ls, const LocalBins bn, int n_a, int n_ob) {
    extern __shared__ unsigned hist[];                                     // the row: the launch's dynamic LDS
    __shared__ double stage[ANGLE_CENTRES / 64][2][LOCAL_VALUES];          // per wavefront Q(a) 2^-40 and q-bar(a)
    const AngleItem it = items[blockIdx.x];
    const int       n_l = ls.n_l, V = 2 * ls.columns;
    const int       at_w = n_l * bn.n_q, at_wbar = at_w + n_l * bn.n_w, at_xi = at_wbar + n_l * bn.n_w;
    const int       at_out = at_xi + ANGLE_MAX_NEIGHBOURS + 1, at_wout = at_out + 4, words = at_wout + 4 * n_l;
    for (int i = threadIdx.x; i < words; i += ANGLE_CENTRES) hist[i] = 0u;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    double*   va = stage[wave][0];
    double*   vb = stage[wave][1];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // per atom (or null): q-bar^2, w, w-bar, each (n_ob, n_a, n_l), one behind the other
    const int64_t each = (int64_t)n_ob * n_a * n_l;
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
        const int64_t nrow = origin + (mine ? tag & LOCAL_TAG_MASK : 0);  // the neighbour's row, below (n_ob, n_a) by the neighbour pass
        int           out = n > ANGLE_MAX_NEIGHBOURS ? 0 : n == 0 ? 1 : -1;   // truncated, isolated: all or nothing
        if (out < 0 && q[cur * V + 1] != 0) out = 2;                       // undefined
        if (out < 0 && __any(mine && q[nrow * V + 1] != 0)) out = 3;       // incomplete: a neighbour without a vector
        if (out >= 0) {
            if (lane == 0) {
                atomicAdd(&hist[at_out + out], 1u);
                if (xi_out != nullptr) xi_out[cur] = -1;
            }
            if (atoms_out != nullptr && lane < 3 * n_l) atoms_out[(lane / n_l) * each + cur * n_l + lane % n_l] = nan;
            continue;
        }
        // the gather: lane v adds value v of every neighbour's row, in list order
        const int    v0 = lane, v1 = lane + 64;
        const double dn = (double)n;
        const double a0 = v0 < V ? __dmul_rn((double)q[cur * V + v0], LOCAL_EPS) : 0.0;
        const double a1 = v1 < V ? __dmul_rn((double)q[cur * V + v1], LOCAL_EPS) : 0.0;
        double       s0 = __ddiv_rn(a0, dn), s1 = __ddiv_rn(a1, dn);
        const int    jrow = (int)(nrow - origin);
        for (int b = 0; b < n; ++b) {
            const int64_t rb = origin + __shfl(jrow, b);
            const double  nb = (double)count[rb];
            if (v0 < V) s0 = __dadd_rn(s0, __ddiv_rn(__dmul_rn((double)q[rb * V + v0], LOCAL_EPS), nb));
            if (v1 < V) s1 = __dadd_rn(s1, __ddiv_rn(__dmul_rn((double)q[rb * V + v1], LOCAL_EPS), nb));
        }
        wave_sync();
        if (v0 < V) va[v0] = a0, vb[v0] = __ddiv_rn(s0, __dadd_rn(dn, 1.0));
        if (v1 < V) va[v1] = a1, vb[v1] = __ddiv_rn(s1, __dadd_rn(dn, 1.0));
        wave_sync();
        int xi = 0, base = 0, col = 0;
        for (int l = 2; l <= ls.l_max; l += 2) {
            if (!(ls.mask >> l & 1u)) continue;
            const double* qa = va + 2 * base;
            const double* qb = vb + 2 * base;
            const double  A = local_norm2(qa, l), Bar = local_norm2(qb, l);
            const int     side = 2 * l + 1;
            const double* tab = w3j + (int64_t)col * LOCAL_W3J_WORDS;
            double        wa = 0.0, wb = 0.0;
            for (int t = lane; t < side * side; t += 64) {
                const int m1 = t / side - l, m2 = t % side - l, m3 = -(m1 + m2);
                if (m3 < -l || m3 > l) continue;
                const double cf = tab[t];
                wa = __dadd_rn(wa, __dmul_rn(cf, local_triple(qa, m1, m2, m3)));
                wb = __dadd_rn(wb, __dmul_rn(cf, local_triple(qb, m1, m2, m3)));
            }
            wa = wave_dsum(wa), wb = wave_dsum(wb);
            if (l == ls.solid_l) {
                // lane b: D = Re sum_m Q_lm(a) conj Q_lm(b) and B = sum_m |Q_lm(b)|^2 over m = -l .. l, ascending |m|
                double D = 0.0, B = 0.0;
                if (mine) {
                    const long long* o = q + nrow * V + 2 * base;
                    for (int m = 0; m <= l; ++m) {
                        const double br = __dmul_rn((double)o[2 * m], LOCAL_EPS), bi = __dmul_rn((double)o[2 * m + 1], LOCAL_EPS);
                        const double d = __dadd_rn(__dmul_rn(qa[2 * m], br), __dmul_rn(qa[2 * m + 1], bi));
                        const double s = __dadd_rn(__dmul_rn(br, br), __dmul_rn(bi, bi));
                        D = __dadd_rn(D, m ? __dmul_rn(2.0, d) : d);
                        B = __dadd_rn(B, m ? __dmul_rn(2.0, s) : s);
                    }
                }
                const bool solid = mine && D > 0.0 && __dmul_rn(D, D) > __dmul_rn(bn.thr2, __dmul_rn(A, B));
                xi = __popcll(__ballot(solid));
            }
            // every lane holds the same values: lane 0 counts q-bar, lane 1 w, lane 2 w-bar, and each stores its own
            {
                const double rhs = __dmul_rn(Bar, (double)(bn.n_q * bn.n_q));
                int          left = 0, right = bn.n_q;                     // (double) left^2 <= rhs, and right^2 > rhs or right = n_q
                while (right - left > 1) {
                    const int mid = (left + right) >> 1;
                    if ((double)(mid * mid) <= rhs) left = mid; else right = mid;
                }
                const bool   bar = lane == 2;
                const double S = bar ? Bar : A, W = bar ? wb : wa;
                const double w = __ddiv_rn(W, __dmul_rn(S, __dsqrt_rn(S)));
                const double u = __dmul_rn(__dadd_rn(w, bn.w_range), bn.w_scale);
                int          slot = col * bn.n_q + left;                   // the counter of this lane's value
                if (lane != 0) {
                    const int which = bar ? 1 : 0;
                    slot = S == 0.0 ? at_wout + (2 * which + 1) * n_l + col
                         : u >= 0.0 && u < (double)bn.n_w ? (bar ? at_wbar : at_w) + col * bn.n_w + (int)u : at_wout + 2 * which * n_l + col;
                }
                if (lane < 3) {
                    atomicAdd(&hist[slot], 1u);
                    if (atoms_out != nullptr) atoms_out[lane * each + cur * n_l + col] = lane == 0 ? Bar : S == 0.0 ? nan : w;
                }
            }
            base += l + 1, ++col;
        }
        if (lane == 0) {
            atomicAdd(&hist[at_xi + xi], 1u);
            if (xi_out != nullptr) xi_out[cur] = xi;
        }
    }
    __syncthreads();
    unsigned* dst = part + (int64_t)blockIdx.x * words;
    for (int i = threadIdx.x; i < words; i += ANGLE_CENTRES) dst[i] = hist[i];
}

int local_ls_check(const LocalLs& ls) {
    const LocalLs o = shell_orders(ls.mask);
    PSA_REQUIRE(o.n_l >= 1 && o.n_l <= LOCAL_MAX_LS && o.n_l == ls.n_l && o.l_max == ls.l_max && o.l_max <= ORDER_MAX_L &&
                    o.columns == ls.columns && o.columns <= LOCAL_MAX_COLUMNS && !(ls.mask & 0xaaaaaaabu),
                "local order pass outside its orders");
    return PSA_OK;
}

}  // namespace

int launch_qlm_sum(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const double* d_norm,
                   long long* d_q, const LocalLs& ls, int64_t n_a, int64_t n_ob) {
    if (n_items == 0) return PSA_OK;
    PSA_TRY(local_ls_check(ls));
    PSA_REQUIRE(shell_grid_check(n_items, n_a, n_ob), "q_lm pass outside its grid");
    hipLaunchKernelGGL(qlm_sum_kernel, dim3((unsigned)n_items), dim3(ANGLE_CENTRES), 0, c->stream, d_count, static_cast<const float4*>(d_list),
                       static_cast<const AngleItem*>(d_items), d_norm, d_q, ls, (int)n_a, (int)n_ob);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

int launch_local_order(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const long long* d_q,
                       const double* d_w3j, unsigned* d_part, double* d_atoms, int* d_xi, const LocalLs& ls, const LocalBins& bins,
                       int64_t n_a, int64_t n_ob) {
    if (n_items == 0) return PSA_OK;
    PSA_TRY(local_ls_check(ls));
    PSA_REQUIRE(shell_grid_check(n_items, n_a, n_ob) && bins.n_q >= 1 && bins.n_q <= LOCAL_MAX_BINS && bins.n_w >= 1 && bins.n_w <= LOCAL_MAX_BINS && (ls.mask >> ls.solid_l & 1u),
                "local order pass outside its grid");
    hipLaunchKernelGGL(local_order_kernel, dim3((unsigned)n_items), dim3(ANGLE_CENTRES),
                       (size_t)local_row_words(ls.n_l, bins.n_q, bins.n_w) * sizeof(unsigned), c->stream, d_count,
                       static_cast<const float4*>(d_list), static_cast<const AngleItem*>(d_items), d_q, d_w3j, d_part, d_atoms, d_xi, ls,
                       bins, (int)n_a, (int)n_ob);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
