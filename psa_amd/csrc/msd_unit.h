// What the kernels of the real-space self dynamics share on the device (msd.hip: moments and the van Hove histogram;
// overlap.hip: the self-overlap counts): one (lag, origin) sample of the displacement in the stated order, and the chunk
// table's entry.  The arithmetic is stated in msd.hip's header and in include/psa_hip.h.
#pragma once
#include <hip/hip_runtime.h>

namespace psa {

// One (lag, origin) unit of the moments and of the histogram: D, the squares and r2 in the stated order
struct MsdUnit {
    float qx, qy, qz, r2;
};
__device__ inline MsdUnit msd_unit(float bx, float by, float bz, float ax, float ay, float az) {
    const float dx = __fsub_rn(bx, ax), dy = __fsub_rn(by, ay), dz = __fsub_rn(bz, az);
    MsdUnit     q;
    q.qx = __fmul_rn(dx, dx), q.qy = __fmul_rn(dy, dy), q.qz = __fmul_rn(dz, dz);
    q.r2 = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, q.qx));
    return q;
}

// chunk table: per chunk its first atom of the block, one past its last, its group
struct MsdChunk {
    int a_lo, a_hi, group, pad;
};

}  // namespace psa
