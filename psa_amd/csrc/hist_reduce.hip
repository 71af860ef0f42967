// The integer reduce of the real-space histograms (psa_van_hove_self, psa_pair_histogram, psa_angle_histogram): the
// uint32 partial histograms that the workgroups of msd_hist, pair_hist and angle_hist wrote with plain stores, summed in
// uint64 into the call's accumulator.  For every output row (j, g), j < n_outer, g < n:
//     acc[(j n + g) cols + col] += factor[g] sum_r part[(r n_outer + j) cols + col],   r in [lo[g], hi[g])
// with the ranges and factors resolved by the host (HistRows): a group's chunks x origin slabs (msd, n_outer = its lags),
// the items of a species pair -- at tau = 0 those of (min, max) for both orders, doubled on the diagonal -- (pair), the
// items of a species (angle, cols = angle_row_words).  A lane per column, HIST_REDUCE_STRANDS strands of lanes each on
// every HIST_REDUCE_STRANDS-th row, their 64-bit sums added through LDS: integer adds, so any order gives the same bits.
// No atomics.
#include "psa_ctx.h"

namespace psa {

namespace {

constexpr int HIST_REDUCE_COLS = 32, HIST_REDUCE_STRANDS = 8;

// Grid (tiles of HIST_REDUCE_COLS columns, n, n_outer)
__global__ void __launch_bounds__(HIST_REDUCE_COLS * HIST_REDUCE_STRANDS)
hist_reduce_kernel(const unsigned* __restrict__ part, const HistRows rows, unsigned long long* __restrict__ acc, int64_t cols) {
    __shared__ unsigned long long strands[HIST_REDUCE_STRANDS][HIST_REDUCE_COLS];
    const int     lane = threadIdx.x % HIST_REDUCE_COLS, strand = threadIdx.x / HIST_REDUCE_COLS, g = blockIdx.y, j = blockIdx.z;
    const int64_t col = (int64_t)blockIdx.x * HIST_REDUCE_COLS + lane, n_outer = gridDim.z;
    unsigned long long sum = 0;
    if (col < cols)
        for (int64_t r = rows.lo[g] + strand; r < rows.hi[g]; r += HIST_REDUCE_STRANDS) sum += part[(r * n_outer + j) * cols + col];
    strands[strand][lane] = sum;
    __syncthreads();
    if (strand || col >= cols) return;
    for (int w = 1; w < HIST_REDUCE_STRANDS; ++w) sum += strands[w][lane];
    acc[((int64_t)j * gridDim.y + g) * cols + col] += (unsigned long long)rows.factor[g] * sum;
}

}  // namespace

int launch_hist_reduce(psa_ctx* c, const unsigned* d_part, const HistRows& rows, int32_t n, int64_t n_outer, int64_t cols,
                       unsigned long long* d_acc) {
    PSA_REQUIRE(n >= 1 && n <= HIST_REDUCE_MAX_ROWS && n_outer >= 1 && n_outer <= 65535 && cols >= 1 && cols < (1ll << 31),
                "integer reduce outside its grid");
    bool any = false;
    for (int g = 0; g < n; ++g) {
        PSA_REQUIRE(rows.lo[g] >= 0 && rows.factor[g] >= 1, "integer reduce: bad row range");
        any = any || rows.hi[g] > rows.lo[g];
    }
    if (!any) return PSA_OK;
    hipLaunchKernelGGL(hist_reduce_kernel, dim3((unsigned)((cols + HIST_REDUCE_COLS - 1) / HIST_REDUCE_COLS), (unsigned)n, (unsigned)n_outer),
                       dim3(HIST_REDUCE_COLS * HIST_REDUCE_STRANDS), 0, c->stream, d_part, rows, d_acc, cols);
    PSA_HIP_CHECK(hipGetLastError());
    return PSA_OK;
}

}  // namespace psa
