// What the real-space kernels share (pair.hip: psa_pair_histogram; angle.hip: psa_angle_histogram; msd.hip:
// psa_van_hove_self; persist.hip: psa_bond_persistence; cna.hip: psa_common_neighbours; acna.hip:
// psa_adaptive_common_neighbours): the box as float32, the minimum-image displacement of two centred fractional coordinates
// and the radial bin of a squared length.  The chain, operation for operation, and its error bound are derived in the
// header of pair.hip; every caller goes through these functions, so what one of them counts below a radius is bit for bit
// what another one does.
#pragma once
#include <hip/hip_runtime.h>

namespace psa {

struct Box32 {
    float h[9];                                    // H (rows = box vectors) rounded to float32
    explicit Box32(const double* box) {
        for (int i = 0; i < 9; ++i) h[i] = (float)box[i];
    }
};

// d = mi(b - a) of two atoms' centred fractional coordinates, and r2 = |d|^2
struct MinImage {
    float dx, dy, dz, r2;
};
__device__ inline MinImage min_image(float ax, float ay, float az, float bx, float by, float bz, const Box32& B) {
    float e0 = __fsub_rn(bx, ax), e1 = __fsub_rn(by, ay), e2 = __fsub_rn(bz, az);
    e0 = __fsub_rn(e0, rintf(e0)), e1 = __fsub_rn(e1, rintf(e1)), e2 = __fsub_rn(e2, rintf(e2));
    MinImage m;
    m.dx = __fmaf_rn(e2, B.h[6], __fmaf_rn(e1, B.h[3], __fmul_rn(e0, B.h[0])));
    m.dy = __fmaf_rn(e2, B.h[7], __fmaf_rn(e1, B.h[4], __fmul_rn(e0, B.h[1])));
    m.dz = __fmaf_rn(e2, B.h[8], __fmaf_rn(e1, B.h[5], __fmul_rn(e0, B.h[2])));
    m.r2 = __fmaf_rn(m.dz, m.dz, __fmaf_rn(m.dy, m.dy, __fmul_rn(m.dx, m.dx)));
    return m;
}

// x = |d| / dr from r2 and inv_dr = float32(1 / dr); its bin of n_r, n_r the overflow counter (edge = (float)n_r; a
// value that is not finite: the overflow counter)
__device__ inline float radial_x(float r2, float inv_dr) { return __fmul_rn(__fsqrt_rn(r2), inv_dr); }
__device__ inline int   radial_bin(float r2, float inv_dr, float edge, int n_r) {
    const float x = radial_x(r2, inv_dr);
    return x < edge ? (int)floorf(x) : n_r;
}

}  // namespace psa
