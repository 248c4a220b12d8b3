// The 64 x 64 tile helpers of the flash-style kernels (attn.hip in fp32 and bf16, ibq.hip in fp32): a workgroup of 4 waves owns one
// 64-row tile, the inner dimension is walked in 64-wide chunks through LDS, and each wave owns one 32x32 tile of every 64x64 product.
// Held here once: the tile size AT and the LDS row pitch Pitch<T>, the register layout of a 32x32 accumulator (acc_row, acc_zero),
// a tile on its way from global memory to LDS (TileRegs, gload / lstore, and gload_b / lstore_b for the [k][col] operand) and the two
// products on a staged pair of tiles (mma_nt, mma_ab).  Pieces, not a framework: every kernel keeps its own LDS carve-up, barriers,
// accumulators and softmax between the calls.
// Written out elsewhere on purpose: patchgan.hip's mma_step has another tile shape (BK = 32, pitch 36 / 40), and the 4-MFMA groups
// of the ranking kernels stay in their files (vq_lookup.h says why).
#pragma once
#include "common.h"

namespace {

constexpr int AT = 64;           // tile rows (queries or keys) of a workgroup, and the d chunk

template <typename T> struct Pitch;
template <> struct Pitch<float> { static constexpr int LD = 68; };         // 272 B rows: 16-byte aligned, rows 4 banks apart
template <> struct Pitch<bf16_raw> { static constexpr int LD = 72; };      // 144 B rows

// row of a 32x32 accumulator register (the column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ void acc_zero(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.0f;
}

// One 64 x 64 operand tile on its way from global memory to LDS, held in registers in between: the loads of the NEXT step are
// issued before the MFMAs of the current one and land in LDS after them, so their latency runs under the matrix work.
template <typename T> struct TileRegs {
    static constexpr int NV = AT * AT * (int)sizeof(T) / 16 / 256;       // 16-byte pieces per thread: 4 (fp32) / 2 (bf16)
    vqk_u32x4 v[NV];
};

// regs <- src[row0 + r][c0 + c], rows past n are zeros (never read); lstore: dst[r][c] <- regs
template <typename T>
__device__ __forceinline__ void gload(TileRegs<T>& t, const T* __restrict__ src, int64_t ld, int row0, int n, int c0) {
    constexpr int V = 16 / (int)sizeof(T), VPR = AT / V;
#pragma unroll
    for (int j = 0; j < TileRegs<T>::NV; ++j) {
        const int i = threadIdx.x + 256 * j, r = i / VPR, v = i % VPR;
        vqk_u32x4 x = {0u, 0u, 0u, 0u};
        if (row0 + r < n) x = *reinterpret_cast<const vqk_u32x4*>(src + (int64_t)(row0 + r) * ld + c0 + v * V);
        t.v[j] = x;
    }
}
template <typename T> __device__ __forceinline__ void lstore(T* __restrict__ dst, const TileRegs<T>& t) {
    constexpr int V = 16 / (int)sizeof(T), VPR = AT / V, LD = Pitch<T>::LD;
#pragma unroll
    for (int j = 0; j < TileRegs<T>::NV; ++j) {
        const int i = threadIdx.x + 256 * j, r = i / VPR, v = i % VPR;
        *reinterpret_cast<vqk_u32x4*>(dst + r * LD + v * V) = t.v[j];
    }
}

// the [k][col] operand of the second products: as it is (fp32) or as the transposed image dst[c][r] (bf16; lanes walk r, so the
// 2-byte stores of a wave are consecutive)
__device__ __forceinline__ void gload_b(TileRegs<float>& t, const float* src, int64_t ld, int row0, int n, int c0) {
    gload<float>(t, src, ld, row0, n, c0);
}
__device__ __forceinline__ void lstore_b(float* dst, const TileRegs<float>& t) { lstore<float>(dst, t); }
__device__ __forceinline__ void gload_b(TileRegs<bf16_raw>& t, const bf16_raw* __restrict__ src, int64_t ld, int row0, int n, int c0) {
#pragma unroll
    for (int j = 0; j < TileRegs<bf16_raw>::NV; ++j) {
        const int i = threadIdx.x + 256 * j, r = i % AT, v = i / AT;
        vqk_u32x4 x = {0u, 0u, 0u, 0u};
        if (row0 + r < n) x = *reinterpret_cast<const vqk_u32x4*>(src + (int64_t)(row0 + r) * ld + c0 + v * 8);
        t.v[j] = x;
    }
}
__device__ __forceinline__ void lstore_b(bf16_raw* __restrict__ dst, const TileRegs<bf16_raw>& t) {
    constexpr int LD = Pitch<bf16_raw>::LD;
#pragma unroll
    for (int j = 0; j < TileRegs<bf16_raw>::NV; ++j) {
        const int i = threadIdx.x + 256 * j, r = i % AT, v = i / AT;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dst[(v * 8 + 2 * e) * LD + r] = (bf16_raw)(t.v[j][e] & 0xffffu);
            dst[(v * 8 + 2 * e + 1) * LD + r] = (bf16_raw)(t.v[j][e] >> 16);
        }
    }
}

// acc[i][j] += sum_k a[i][k] b[j][k], k < 64; a and b point at the first of the wave's 32 rows.  fp32: lane (r, h) reads k = 8s + 4h
// + 0..3 of its row as one 16-byte vector and feeds MFMA j of step s with element j -- the same k on both sides, which is all a
// sum over k needs.
__device__ __forceinline__ void mma_nt(f32x16& acc, const float* a, const float* b, int lane) {
    const float* pa = a + (lane & 31) * Pitch<float>::LD + 4 * (lane >> 5);
    const float* pb = b + (lane & 31) * Pitch<float>::LD + 4 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const f32x4 va = *reinterpret_cast<const f32x4*>(pa + 8 * s);
        const f32x4 vb = *reinterpret_cast<const f32x4*>(pb + 8 * s);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va[j], vb[j], acc, 0, 0, 0);
    }
}
__device__ __forceinline__ void mma_nt(f32x16& acc, const bf16_raw* a, const bf16_raw* b, int lane) {
    const bf16_raw* pa = a + (lane & 31) * Pitch<bf16_raw>::LD + 8 * (lane >> 5);
    const bf16_raw* pb = b + (lane & 31) * Pitch<bf16_raw>::LD + 8 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const bf16x8_t va = *reinterpret_cast<const bf16x8_t*>(pa + 16 * s);
        const bf16x8_t vb = *reinterpret_cast<const bf16x8_t*>(pb + 16 * s);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, vb, acc, 0, 0, 0);
    }
}
// acc[i][j] += sum_k a[i][k] b[k][col0 + j] with b as lstore_b left it
__device__ __forceinline__ void mma_ab(f32x16& acc, const float* a, const float* b, int col0, int lane) {
    constexpr int LD = Pitch<float>::LD;
    const float* pa = a + (lane & 31) * LD + 4 * (lane >> 5);
    const float* pb = b + 4 * (lane >> 5) * LD + col0 + (lane & 31);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const f32x4 va = *reinterpret_cast<const f32x4*>(pa + 8 * s);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va[j], pb[(8 * s + j) * LD], acc, 0, 0, 0);
    }
}
__device__ __forceinline__ void mma_ab(f32x16& acc, const bf16_raw* a, const bf16_raw* b, int col0, int lane) {
    mma_nt(acc, a, b + col0 * Pitch<bf16_raw>::LD, lane);
}

}  // namespace
