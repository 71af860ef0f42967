// Kernel of the Steinhardt bond-orientational order parameters (psa_bond_order; definition: include/psa_hip.h, host side:
// api_order.hip): q_l of the neighbour shell of every atom at every origin, from the lists that the fraction pass
// (pair.hip) and the neighbour pass (angle.hip) leave -- per (origin, centre) the true neighbour count and up to 64 legs
// {d_x, d_y, d_z, tag}.  By the addition theorem of the spherical harmonics, with n legs and theta_bc the angle between
// the legs b and c,
//     q_l^2 = 4 pi / (2 l + 1) sum_m |1/n sum_b Y_lm(d_b)|^2 = 1/n^2 (n + 2 sum_{b<c} P_l(cos theta_bc))
// so the pass needs no spherical harmonic and no frame: the pair loop of angle_hist_kernel with a Legendre recurrence on
// the cosine in place of the bisection.
//
// Arithmetic.  Per pair of legs, float32, every operation rounded once but the square root (v_sqrt_f32: within one ulp);
// r2 and cos are angle.hip's by construction: both kernels call shell.h's shell_r2 and shell_cos:
//     r2 = fma(d_z, d_z, fma(d_y, d_y, d_x d_x));  dot = fma(d_z(b), d_z(c), fma(d_y(b), d_y(c), d_x(b) d_x(c)))
//     cos = dot / sqrt(r2(b) r2(c)), clamped to [-1, 1]; a cos that is not a number makes the centre undefined
//     P_0 = 1;  P_1 = cos;  P_{k+1} = fma(A_k, cos P_k, -(B_k P_{k-1}))       k = 1 .. l_max - 1
//     A_k = float32((2 k + 1) / (k + 1)),  B_k = float32(k / (k + 1)), the quotients formed in float64
//     t_l = __float2ll_rn(P_l 2^24)
// symmetric in b <-> c bit for bit.  Per centre, 64-bit integers: X_l = n 2^24 + 2 sum_{b<c} t_l clamped to [0, n^2 2^24]
// (q_l^2 = X_l / (n^2 2^24)); the bin is the largest i < n_q with i^2 n^2 2^24 <= X_l n_q^2, by bisection in integers (both
// sides below 2^57).  Integer adds commute: X_l and the counts are the same bits whatever the order of the list, the
// blocking and the order of the atoms in a species.
//
// Tiling.  That of angle_hist_kernel: a workgroup of four wavefronts takes an item of the host's table (64 centres of one
// species, a slab of origins); a wavefront takes a centre, its lanes load the list once (issued while the centre before
// is processed) and lane j takes the pairs (j, j + m mod n), m = 1 .. n / 2, the partner's leg by cross-lane reads: the
// centre walk and the leg-pair step of shell.h, as in angle.hip.  A lane adds its t_l into one int64 accumulator per order
// asked for (a register per l = 1 .. 12, indexed statically; at most eight are in use); a 64-bit wave reduction; the lanes
// 0 .. n_l - 1 clamp, bin and count one order each with a 32-bit integer LDS add, and store X_l where the caller asks for
// it.  The histogram (n_l n_q <= 8192 words) and the three counters of the centres left out go to partials with plain
// stores and through hist_reduce.hip.  No global atomics, no float atomics.
#include "shell.h"

namespace psa {

namespace {

constexpr float order_a(int k) { return (float)((2.0 * k + 1.0) / (k + 1.0)); }
constexpr float order_b(int k) { return (float)((double)k / (k + 1.0)); }

// Grid (items).  part[item][row]: n_l n_q bins, then the truncated, the isolated and the undefined centres
__global__ void __launch_bounds__(ANGLE_CENTRES)
order_hist_kernel(const int* __restrict__ count, const float4* __restrict__ list, const AngleItem* __restrict__ items,
                  unsigned* __restrict__ part, long long* __restrict__ x, const OrderLs ls, int n_a, int n_ob, int n_q) {
    extern __shared__ unsigned hist[];                                     // the row: the launch's dynamic LDS
    const AngleItem it = items[blockIdx.x];
    const int       bins = ls.n_l * n_q, words = bins + 3;
    for (int i = threadIdx.x; i < words; i += ANGLE_CENTRES) hist[i] = 0u;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    // the wavefront's centres in turn, the next one's count and list on their way while this one is processed
    SHELL_WALK_FIRST(it, wave, n_a, n_ob);
    int    n_next = more ? count[row] : 0;
    float4 e_next = more ? list[row * ANGLE_MAX_NEIGHBOURS + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    while (more) {
        const int     n = __builtin_amdgcn_readfirstlane(n_next);
        const float4  e = e_next;
        const int64_t cur = row;
        SHELL_WALK_NEXT(it, wave, n_a, n_ob, (n_next = count[row], e_next = list[row * ANGLE_MAX_NEIGHBOURS + lane]))
        int       out = n > ANGLE_MAX_NEIGHBOURS ? 0 : n == 0 ? 1 : -1;    // truncated, isolated: all or nothing
        long long acc[ORDER_MAX_L] = {};
        if (out < 0) {
            const float r2 = shell_r2(e);
            bool        bad = false;
            for (int m = 1; 2 * m <= n; ++m) {
                const float4 o = shell_partner_leg(e, r2, shell_partner(lane, m, n));
                // the lanes without a pair in this round go along and add nothing
                const bool   mine = shell_has_pair(lane, m, n);
                float        cs = shell_cos(e, r2, o);
                bad = bad || (mine && cs != cs);                           // a coincident neighbour: the sums are dropped below
                cs = fminf(1.f, fmaxf(-1.f, cs));
                float pm = 1.f, p = cs;                                    // P_{k-1}, P_k
#pragma unroll
                for (int kk = 1; kk <= ORDER_MAX_L; ++kk) {
                    if (ls.mask >> kk & 1u) acc[kk - 1] += mine ? __float2ll_rn(__fmul_rn(p, (float)(1 << ORDER_SHIFT))) : 0ll;
                    if (kk >= ls.l_max) break;
                    const float pn = __fmaf_rn(order_a(kk), __fmul_rn(cs, p), -__fmul_rn(order_b(kk), pm));
                    pm = p, p = pn;
                }
            }
            if (__any(bad)) out = 2;                                       // undefined
        }
        if (out >= 0) {
            if (lane == 0) atomicAdd(&hist[bins + out], 1u);
            if (x != nullptr && lane < ls.n_l) x[cur * ls.n_l + lane] = -1;
            continue;
        }
        long long X = 0;                                                   // lane j: the sum of column j
        int       col = 0;
#pragma unroll
        for (int l = 1; l <= ORDER_MAX_L; ++l) {
            if (!(ls.mask >> l & 1u)) continue;
            long long s = acc[l - 1];                                      // (shell.h's wave_sum here costs 54 instructions: own loop)
            for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
            if (lane == col) X = s;
            ++col;
        }
        if (lane < ls.n_l) {
            const long long n2 = (long long)n * n << ORDER_SHIFT;
            X = min(max(((long long)n << ORDER_SHIFT) + 2 * X, 0ll), n2);
            const long long rhs = X * n_q * n_q;
            int             left = 0, right = n_q;                         // left^2 n2 <= rhs, and right^2 n2 > rhs or right = n_q
            while (right - left > 1) {
                const int mid = (left + right) >> 1;
                if ((long long)mid * mid * n2 <= rhs) left = mid; else right = mid;
            }
            atomicAdd(&hist[lane * n_q + left], 1u);
            if (x != nullptr) x[cur * ls.n_l + lane] = X;
        }
    }
    __syncthreads();
    unsigned* dst = part + (int64_t)blockIdx.x * words;
    for (int i = threadIdx.x; i < words; i += ANGLE_CENTRES) dst[i] = hist[i];
}

}  // namespace

int launch_order_hist(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, unsigned* d_part,
                      long long* d_x, const OrderLs& ls, int64_t n_a, int64_t n_ob, int32_t n_q) {
    if (n_items == 0) return PSA_OK;
    const LocalLs o = shell_orders(ls.mask);
    PSA_REQUIRE(shell_grid_check(n_items, n_a, n_ob) && n_q >= 1 && n_q <= ORDER_MAX_BINS && o.n_l >= 1 && o.n_l <= ORDER_MAX_LS &&
                    o.n_l == ls.n_l && o.l_max == ls.l_max && o.l_max <= ORDER_MAX_L && !(ls.mask & 1u), "order pass outside its grid");
    hipLaunchKernelGGL(order_hist_kernel, dim3((unsigned)n_items), dim3(ANGLE_CENTRES), (size_t)order_row_words(o.n_l, n_q) * sizeof(unsigned),
                       c->stream, d_count, static_cast<const float4*>(d_list), static_cast<const AngleItem*>(d_items), d_part, d_x, ls,
                       (int)n_a, (int)n_ob, (int)n_q);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
