// What the two contraction kernels of the mode projection share (modes.hip: one spectrum per k-vector; modes_welch.hip:
// the segment average): the work split and the walk over the n = 3 B rows of one (k, w) that fills the MT complex
// accumulators of a pass.
#pragma once
#include <hip/hip_runtime.h>

namespace psa {

constexpr int MODES_TW = 64;   // frequencies per workgroup tile: one per lane
constexpr int MODES_TK = 4;    // k-vectors per workgroup tile: one per wavefront

typedef float f32x2 __attribute__((ext_vector_type(2)));   // (re, im): one v_pk_fma_f32 per product

// acc[j] += sum_{b,c} cf[3 b + c][j] * rows[b stride_b + c stride_c], in the order of n = 3 b + c.  rows points at the
// lane's element of group 0, component 0; cf at the wavefront's coefficients [n][MT] of this pass (uniform: scalar loads);
// a lane with !in_range reads nothing and adds zeros.
template <int MT>
__device__ __forceinline__ void mode_rows(f32x2 (&acc)[MT], const float2* __restrict__ rows, size_t stride_b, size_t stride_c,
                                          const float2* __restrict__ cf, int B, bool in_range) {
    for (int b = 0; b < B; ++b) {
        const float2* row = rows + (size_t)b * stride_b;
        float2        s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = in_range ? row[(size_t)c * stride_c] : make_float2(0.f, 0.f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x2   xy = {s[c].x, s[c].y}, yx = {-s[c].y, s[c].x};
            const float2* e = cf + (size_t)(3 * b + c) * MT;
#pragma unroll
            for (int j = 0; j < MT; ++j) {              // (p + iq)(x + iy), p + iq = conj(eig)
                const float2 pq = e[j];
                acc[j] = __builtin_elementwise_fma(f32x2{pq.x, pq.x}, xy, acc[j]);
                acc[j] = __builtin_elementwise_fma(f32x2{pq.y, pq.y}, yx, acc[j]);
            }
        }
    }
}

}  // namespace psa
