// What the kernels on the box's reciprocal lattice share (lattice.hip: psa_lattice_spectra; self.hip: psa_self_spectra):
// the box inverse as a kernel argument, the fractional coordinate of an atom as float32 hi + lo, a table entry
// (cos, sin)(2 pi m s) formed directly from m, and the float32 complex product.  The arithmetic and its error bound
// (eps_lat) are derived in the header of lattice.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace psa {

struct LatBox {
    float hi[9], lo[9];                            // Hinv[c][j] as float32 hi + lo, row-major: c Cartesian, j axis
};

// a x b of two complex numbers (cos, sin)
__device__ __forceinline__ float2 lat_cmul(const float2 a, const float2 b) {
    return make_float2(__fmaf_rn(a.x, b.x, -__fmul_rn(a.y, b.y)), __fmaf_rn(a.x, b.y, __fmul_rn(a.y, b.x)));
}

// fractional coordinate j of one atom in turns, reduced to about [-1/2, 1/2], as hi + lo
__device__ __forceinline__ float2 lat_frac(const float x, const float y, const float z, const LatBox& b, const int j) {
    const float hx = b.hi[j], hy = b.hi[3 + j], hz = b.hi[6 + j];
    const float px = __fmul_rn(hx, x), py = __fmul_rn(hy, y), pz = __fmul_rn(hz, z);
    const float ex = __fmaf_rn(hx, x, -px), ey = __fmaf_rn(hy, y, -py), ez = __fmaf_rn(hz, z, -pz);
    const float fx = px - __builtin_rintf(px), fy = py - __builtin_rintf(py), fz = pz - __builtin_rintf(pz);
    float       t = fx + fy;
    float       bb = t - fx;
    const float err1 = (fx - (t - bb)) + (fy - bb);
    t -= __builtin_rintf(t);
    const float t2 = t + fz;
    bb = t2 - t;
    const float err2 = (t - (t2 - bb)) + (fz - bb);
    const float s_hi = t2 - __builtin_rintf(t2);
    float       lo = (ex + ey) + ez;
    lo = __fmaf_rn(b.lo[j], x, lo);
    lo = __fmaf_rn(b.lo[3 + j], y, lo);
    lo = __fmaf_rn(b.lo[6 + j], z, lo);
    return make_float2(s_hi, lo + (err1 + err2));
}

// (cos, sin)(2 pi m s), s = hi + lo
__device__ __forceinline__ float2 lat_entry(const float m, const float2 s) {
    const float p = __fmul_rn(m, s.x), e = __fmaf_rn(m, s.x, -p);
    const float g = p - __builtin_rintf(p);
    const float turns = g + __fmaf_rn(m, s.y, e);
    return make_float2(__builtin_amdgcn_cosf(turns), __builtin_amdgcn_sinf(turns));
}

}  // namespace psa
