// What the passes over the neighbour lists share (angle.hip: angle_hist_kernel; order.hip: order_hist_kernel; qlm.hip:
// qlm_sum_kernel, local_order_kernel; cluster.hip: cluster_bonds_kernel, cluster_hook_kernel; persist.hip:
// persist_step_kernel; cna.hip: cna_signature_kernel; acna.hip: acna_signature_kernel): the walk of a wavefront over the
// centres of its item, the round of leg pairs within a centre, the wave reductions and the launchers' shared guard.  The
// lists are those the neighbour pass (angle.hip) leaves: per (origin, centre) the true neighbour count and up to 64 legs
// {d_x, d_y, d_z, tag}.  A new pass over them uses the walk and the leg-pair step from here.
#pragma once
#include "psa_ctx.h"

namespace psa {

// ---- the centre walk.  A workgroup of four wavefronts takes an item (AngleItem: centres [a_lo, a_lo + a_n) of one
// species, the origins slab, slab + n_os, ... below n_ob); wavefront `wave` takes the centres wave, wave + 4, ... of an
// origin, then those of the next origin of the slab.  SHELL_WALK_FIRST declares the walk's state in the kernel -- k, ci,
// `more` (there is a centre on its way) and `row`, its row in (n_ob, n_a) --, SHELL_WALK_NEXT moves it on and runs PREFETCH,
// the caller's loads of the next centre (every lane loads its slot of the list whether it is filled or not: the slots are
// there, the lanes at and beyond n are masked), which the caller places before it processes the current one.  A row is
// formed, and so loaded, only where `more` holds; the wrap to the slab's next origin happens once per origin.
// Macros, not functions: as a function (the state in a struct or by reference, the loads a callable or in an `if` of the
// caller) the advance changed the listing of every kernel that used it, and the angle and order passes measured slower
// (profiles/shell_refactor_isa.txt); as text it is the code the kernels had, instruction for instruction.
#define SHELL_WALK_FIRST(it, wave, n_a, n_ob)              \
    int     k = (it).slab, ci = (wave);                    \
    bool    more = k < (n_ob) && ci < (it).a_n;            \
    int64_t row = (int64_t)k * (n_a) + (it).a_lo + ci
#define SHELL_WALK_NEXT(it, wave, n_a, n_ob, PREFETCH)     \
    ci += ANGLE_CENTRES / 64;                              \
    if (ci >= (it).a_n) ci = (wave), k += (it).n_os;       \
    more = k < (n_ob) && ci < (it).a_n;                    \
    if (more) {                                            \
        row = (int64_t)k * (n_a) + (it).a_lo + ci;         \
        PREFETCH;                                          \
    }

// ---- the leg-pair step.  Lane j of a centre with n legs takes the pairs (j, j + m mod n), m = 1 .. n / 2: every unordered
// pair once.  float32, symmetric in the two legs bit for bit; every operation is rounded once but the square root under
// the cosine, which is the hardware's v_sqrt_f32 behind __fsqrt_rn: within one ulp.  (Which helper takes the leg by value
// and which by reference is not free either: this combination leaves both kernels' listings as they were, see
// profiles/shell_refactor_isa.txt.)
__device__ __forceinline__ float shell_r2(float4 e) { return __fmaf_rn(e.z, e.z, __fmaf_rn(e.y, e.y, __fmul_rn(e.x, e.x))); }

// the lane whose leg is this lane's partner in round m; a lane at or beyond n reads itself
__device__ __forceinline__ int shell_partner(int lane, int m, int n) {
    int src = lane + m;
    src = src >= n ? src - n : src;
    return lane < n ? src : lane;
}

// has this lane a pair of its own in round m?  (n even, m = n / 2: each pair once)
__device__ __forceinline__ bool shell_has_pair(int lane, int m, int n) { return lane < (2 * m == n ? m : n); }

// the partner's leg {d_x, d_y, d_z, r2} by cross-lane reads
__device__ __forceinline__ float4 shell_partner_leg(const float4& e, float r2, int src) {
    const float ox = __shfl(e.x, src), oy = __shfl(e.y, src), oz = __shfl(e.z, src), o2 = __shfl(r2, src);
    return make_float4(ox, oy, oz, o2);
}

// cos of the angle between the leg e (squared length r2) and the partner's o = {d_x, d_y, d_z, r2}, not clamped; not a
// number where a leg has length 0
__device__ __forceinline__ float shell_cos(float4 e, float r2, float4 o) {
    const float dot = __fmaf_rn(e.z, o.z, __fmaf_rn(e.y, o.y, __fmul_rn(e.x, o.x)));
    return __fdiv_rn(dot, __fsqrt_rn(__fmul_rn(r2, o.w)));
}

// ---- the solid-like bond test (psa_local_order's definition).  v: a centre's vector of one order staged as float64, Q 2^-40,
// (re, im) pairs for m = 0 .. l.  shell_norm2: sum_{m = -l .. l} |v_m|^2 = |v_0|^2 + 2 sum_{m > 0} |v_m|^2 in ascending m.
// shell_solid_bond: o the neighbour's row of the table of that order (int64); D = Re sum_m Q_lm(a) conj Q_lm(b) and
// B = sum_m |Q_lm(b)|^2 in ascending m, every operation rounded once, then D > 0 && D D > thr2 (A B), A = shell_norm2(v).
// (cluster.hip uses them; qlm.hip keeps its own text of the same operations)
constexpr double SHELL_Q_EPS = 1.0 / (double)(1ll << LOCAL_SHIFT);

__device__ __forceinline__ double shell_norm2(const double* v, int l) {
    double s = 0.0;
    for (int m = 0; m <= l; ++m) {
        const double t = __dadd_rn(__dmul_rn(v[2 * m], v[2 * m]), __dmul_rn(v[2 * m + 1], v[2 * m + 1]));
        s = __dadd_rn(s, m ? __dmul_rn(2.0, t) : t);
    }
    return s;
}

__device__ __forceinline__ bool shell_solid_bond(const double* v, const long long* o, int l, double A, double thr2) {
    double D = 0.0, B = 0.0;
    for (int m = 0; m <= l; ++m) {
        const double br = __dmul_rn((double)o[2 * m], SHELL_Q_EPS), bi = __dmul_rn((double)o[2 * m + 1], SHELL_Q_EPS);
        const double d = __dadd_rn(__dmul_rn(v[2 * m], br), __dmul_rn(v[2 * m + 1], bi));
        const double s = __dadd_rn(__dmul_rn(br, br), __dmul_rn(bi, bi));
        D = __dadd_rn(D, m ? __dmul_rn(2.0, d) : d);
        B = __dadd_rn(B, m ? __dmul_rn(2.0, s) : s);
    }
    return D > 0.0 && __dmul_rn(D, D) > __dmul_rn(thr2, __dmul_rn(A, B));
}

// ---- wave helpers
__device__ __forceinline__ long long wave_sum(long long s) {
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

__device__ __forceinline__ double wave_dsum(double s) {
    for (int o = 32; o >= 1; o >>= 1) s = __dadd_rn(s, __shfl_xor(s, o));
    return s;
}

// what one wavefront wrote to LDS is there for its other lanes, and no access moves across
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ---- host side: what the launchers of the four passes ask of their grid (items in x, one row per (origin, centre) with
// the row and the tag's list position in 28 bits, the origins of a block)
inline bool shell_grid_check(int64_t n_items, int64_t n_a, int64_t n_ob) {
    return n_items < (1ll << 31) && n_a < (1ll << ANGLE_SPECIES_SHIFT) && n_ob >= 1 && n_ob <= 65535;
}

// the orders of a mask recounted: how many, the largest, the sum of l + 1 (solid_l: 0)
inline LocalLs shell_orders(unsigned mask) {
    LocalLs o{0, 0, 0, 0, mask};
    for (int l = 0; l < 32; ++l)
        if (mask >> l & 1u) ++o.n_l, o.l_max = l, o.columns += l + 1;
    return o;
}

}  // namespace psa
