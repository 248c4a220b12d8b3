// The l2 normalisation of the cosine quantizer (vq_cos.hip): ONE device function, so that the stand-alone normalise kernel, the
// codebook prepare step and the fused forward / backward kernels give the same bits for the same row.
//   ss = |x|^2 with the bits of vq.hip::row_sqnorm_kernel (lane l: fma chain over l, l + 64, ...; xor butterfly 32..1);
//   r = sqrt(ss), inv = 1 / max(r, eps), both correctly rounded (plain sqrtf and division: the build passes no flag that relaxes
//   them, and the _rn intrinsics of this toolchain map to the native approximations instead);  xn_j = x_j * inv.
#pragma once
#include "common.h"

constexpr float COS_EPS = 1e-12f;

// |row|^2 of one wavefront's row, the same value in every lane (the adds of a butterfly level commute)
__device__ __forceinline__ float cos_row_ss(const float* p, int d, int lane) {
    float acc = 0.0f;
    for (int k = lane; k < d; k += 64) acc = __fmaf_rn(p[k], p[k], acc);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off, 64));
    return acc;
}

// One wavefront normalises one row: returns inv, writes xn to out (may alias p: lane l reads and writes l, l + 64, ... only) and
// |xn|^2 -- the row_sqnorm bits of the normalised row -- to nn.
__device__ __forceinline__ float cos_nrm_row(const float* p, int d, int lane, float* out, float& nn) {
    const float ss = cos_row_ss(p, d, lane);
    const float inv = 1.0f / fmaxf(__builtin_sqrtf(ss), COS_EPS);
    float acc = 0.0f;
    for (int k = lane; k < d; k += 64) {
        const float xn = __fmul_rn(p[k], inv);
        out[k] = xn;
        acc = __fmaf_rn(xn, xn, acc);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off, 64));
    nn = acc;
    return inv;
}

// workspace of vqk_cos_prepare_f32: en[K][D] | |en|^2[K] | inv_e[K], every part 16-byte aligned
static inline int64_t cos_off_e2(int k, int d) { return (int64_t)k * d * 4; }
static inline int64_t cos_off_inv(int k, int d) { return cos_off_e2(k, d) + (((int64_t)k * 4 + 15) & ~(int64_t)15); }
static inline int64_t cos_ws_size(int k, int d) { return cos_off_inv(k, d) + (((int64_t)k * 4 + 15) & ~(int64_t)15); }
