// The parameter-gradient slabs of the projection quantizers' backward (fsq.hip, lfq.hip) and the launch that adds them: every block of
// the backward stores ONE slab of its sums over its rows; the sums over all rows are formed here, in an order fixed by the slab count.
#pragma once
#include "common.h"

namespace {

// slab of one block (floats): [dW_in d*D][db_in d][dW_out D*d][db_out D], padded to a multiple of 4
__host__ __device__ inline int64_t proj_slab_floats(int dm, int d) { return ((int64_t)2 * d * dm + dm + d + 3) & ~(int64_t)3; }

// second launch: the slabs summed in an order fixed by their count, one thread per gradient element; accumulate: add to what the
// target holds
__global__ __launch_bounds__(256) void proj_slab_sum_kernel(const float* __restrict__ ws, int slabs, int dm, int d, int accumulate,
                                                            float* __restrict__ dw_in, float* __restrict__ db_in,
                                                            float* __restrict__ dw_out, float* __restrict__ db_out) {
    const int total = 2 * d * dm + dm + d;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t pitch = proj_slab_floats(dm, d);
    // four running sums over the block index (b % 4), combined at the end: a fixed order, and four times the loads in flight
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const float* src = ws + e;
    int b = 0;
#pragma unroll 4
    for (; b + 4 <= slabs; b += 4) {
        s0 += src[(b + 0) * pitch];
        s1 += src[(b + 1) * pitch];
        s2 += src[(b + 2) * pitch];
        s3 += src[(b + 3) * pitch];
    }
    for (; b < slabs; ++b) s0 += src[b * pitch];
    const float s = (s0 + s1) + (s2 + s3);
    float* dst;
    if (e < d * dm) dst = dw_in + e;
    else if (e < d * dm + d) dst = db_in + (e - d * dm);
    else if (e < 2 * d * dm + d) dst = dw_out + (e - d * dm - d);
    else dst = db_out + (e - 2 * d * dm - d);
    *dst = accumulate ? *dst + s : s;
}

}  // namespace
