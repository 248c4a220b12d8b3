// The core the projection quantizers share (fsq.hip, lfq.hip, bsq.hip): u = W_in z + b_in, a code c per channel, q = W_out c + b_out,
// and the straight-through backward with its ordered parameter-gradient sums.  What only the two sign quantizers share (sigmoid /
// entropy, group tables, finish and decode kernels, host launchers) is sign_quant.h, on top of this file.
//
// Every kernel works a WAVE PER ROW.  Lane l owns the 16-byte chunks l, l + 64, ... of the row (4 fp32 channels each), so every global
// access of z / q / dq / dz is 16 bytes per lane (8 bytes for 4 packed bf16) and contiguous over the wave.  W_in [d][D] and W_out^T
// [d][D] sit in LDS in the same chunk order: a lane reads its own 16 bytes of every projection row, conflict-free.  The d projections
// of a row are partial dot products per lane + a butterfly over the wave (fixed order: every lane ends with the same bits).
// The backward's grid is (blocks over rows, 256-channel slices): a block owns ONE chunk per lane whatever D is; the cotangent
// g = W_out^T dq of a row needs the whole row of dq, which every slice reads.  The parameter gradients are sums over rows: per lane in
// registers over the rows of its wave (fixed by the grid), over the block's waves through LDS in wave order (each file's own pass),
// then ONE slab per block in the workspace -- plain stores, no atomics -- and a second launch that adds the slabs in an order fixed by
// their count.
//
// A quantizer's file supplies its channel bound kMaxD and chunks per lane kMaxChunks (the templates below unroll to exactly these), how
// channel j's code is obtained (a functor), the step from u to the code and from g to du, and its block reduction.  The loops over a
// lane's chunks stay in the kernels: the helpers below work on ONE chunk (moved in here, those loops changed the register allocation).
#pragma once
#include "common.h"

namespace {

constexpr int kProjWaves = 4;        // waves (= rows in flight) per block
constexpr int kProjThreads = 64 * kProjWaves;
constexpr int kProjSlice = 256;      // channels per backward block (one chunk per lane)

// W_in rows [c0, c0 + cn) -> wi [d][cn], W_out^T (all D channels) -> woT [d][dm]; scalar loads: the parameters need no alignment.
// The caller synchronises.
__device__ __forceinline__ void proj_stage_weights(const float* w_in, const float* w_out, int dm, int d, int c0, int cn, float* wi,
                                                   float* woT) {
    if (wi)
        for (int i = threadIdx.x; i < d * cn; i += kProjThreads) wi[i] = w_in[(i / cn) * dm + c0 + i % cn];
    if (woT)
        for (int i = threadIdx.x; i < d * dm; i += kProjThreads) woT[(i % d) * dm + i / d] = w_out[i];
}

template <int kMaxChunks>
__device__ __forceinline__ void proj_load_row(const float* z, int64_t row, int dm, int lane, float (&zc)[kMaxChunks][4]) {
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
        const int ch = (c * 64 + lane) * 4;
        if (ch < dm) Vec16<float>::load(z + row * dm + ch, zc[c]);
    }
}

template <typename Td> __device__ __forceinline__ void proj_load4(const Td* p, float (&o)[4]);
template <> __device__ __forceinline__ void proj_load4<float>(const float* p, float (&o)[4]) { Vec16<float>::load(p, o); }
template <> __device__ __forceinline__ void proj_load4<bf16_raw>(const bf16_raw* p, float (&o)[4]) {
    const u16x4 v = *reinterpret_cast<const u16x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = bf16_to_f32(v[i]);
}

__device__ __forceinline__ void proj_store_q(float* q, bf16_raw* q_lo, int64_t at, const float (&o)[4]) {
    if (q) Vec16<float>::store(q + at, o);
    if (q_lo) {
        typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
        const u32x2 v = {vqk_pack_bf16x2(o[0], o[1]), vqk_pack_bf16x2(o[2], o[3])};
        *reinterpret_cast<u32x2*>(q_lo + at) = v;
    }
}

// one 16-byte chunk (channels ch .. ch + 3) of a row against the d rows of an LDS matrix w [d][dm]: acc[j] += x . w[j], j ascending.
// Forward: x = z, w = W_in (the lane's partial projections); backward: x = dq, w = W_out^T (its partial cotangents g).
template <int kMaxD>
__device__ __forceinline__ void proj_dot_chunk(const float* w, int dm, int d, int ch, const float (&x)[4], float (&acc)[kMaxD]) {
#pragma unroll
    for (int j = 0; j < kMaxD; ++j)
        if (j < d) {
            const f32x4 wj = *reinterpret_cast<const f32x4*>(w + j * dm + ch);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j] = fmaf(x[i], wj[i], acc[j]);
        }
}

// 4 channels of q = b_out + sum_j W_out[:, j] c_j, j ascending, c_j = code(j): THE decode function -- forward and decode share it,
// same bits
template <int kMaxD, typename Code>
__device__ __forceinline__ void proj_q_chunk(const float* woT, int dm, int d, Code code, const float* b_out, int ch, float (&o)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = b_out[ch + i];
#pragma unroll
    for (int j = 0; j < kMaxD; ++j)
        if (j < d) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(woT + j * dm + ch);
            const float c = code(j);
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = fmaf(w[i], c, o[i]);
        }
}

// backward, one channel of one row on the lane's chunk: du = the gradient at u_j, cj = the channel's code, wi_j = W_in[j] at the chunk
__device__ __forceinline__ void proj_accumulate(const float* wi_j, float du, float cj, const float (&zo)[4], const float (&dqo)[4],
                                                float (&dzo)[4], float (&a_wi)[4], float (&a_wo)[4]) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(wi_j);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        dzo[i] = fmaf(w[i], du, dzo[i]);
        a_wi[i] = fmaf(du, zo[i], a_wi[i]);
        a_wo[i] = fmaf(dqo[i], cj, a_wo[i]);
    }
}

// backward, end of a row on the lane's chunk: dz out, the row's dq into the db_out sum
__device__ __forceinline__ void proj_finish_row(float* dz_at, const float (&dzo)[4], const float (&dqo)[4], float (&a_bo)[4]) {
    Vec16<float>::store(dz_at, dzo);
#pragma unroll
    for (int i = 0; i < 4; ++i) a_bo[i] += dqo[i];
}

// slab of one block (floats): [dW_in d*D][db_in d][dW_out D*d][db_out D], padded to a multiple of 4
__host__ __device__ inline int64_t proj_slab_floats(int dm, int d) { return ((int64_t)2 * d * dm + dm + d + 3) & ~(int64_t)3; }

// backward tail, wave 0 of a block: its sums into the block's slab at the lane's chunk ch (has: the chunk is inside D).  Returns where
// db_in [d] goes: how the channels' sums are spread over the lanes is the caller's.
template <int kMaxD>
__device__ __forceinline__ float* proj_store_slab(float* ws, int dm, int d, int ch, bool has, const float (&a_wi)[kMaxD][4],
                                                  const float (&a_wo)[kMaxD][4], const float (&a_bo)[4]) {
    float* slab = ws + (int64_t)blockIdx.x * proj_slab_floats(dm, d);
    float* s_bi = slab + d * dm;
    float* s_wo = s_bi + d;
    float* s_bo = s_wo + dm * d;
    if (has) {
#pragma unroll
        for (int j = 0; j < kMaxD; ++j)
            if (j < d) {
                Vec16<float>::store(slab + j * dm + ch, a_wi[j]);
#pragma unroll
                for (int i = 0; i < 4; ++i) s_wo[(ch + i) * d + j] = a_wo[j][i];
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) s_bo[ch + i] = a_bo[i];
    }
    return s_bi;
}

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

inline int proj_launch_slab_sum(const void* ws, int slabs, int dm, int d, int accumulate, float* dw_in, float* db_in, float* dw_out,
                                float* db_out, hipStream_t stream) {
    const int total = 2 * d * dm + dm + d;
    hipLaunchKernelGGL(proj_slab_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const float*>(ws), slabs, dm, d, accumulate, dw_in, db_in, dw_out, db_out);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

// ---- the transposing wave reduction (bsq.hip) ----
// kMaxD <= 32 per-lane partials in (padded to 32 with zeros), the 64-lane sum of channel j out on the lanes 2 j and 2 j + 1 -- the
// LANE MAP: lane l ends with channel l >> 1, both lanes of a pair with the same bits.  Five halving stages and a closing step, 32
// exchanges where kMaxD butterflies take 6 kMaxD.  A stage pairs lane l with lane l ^ m; of the n values both hold, the lane with bit m
// clear keeps the lower n / 2 channels and the other lane the upper n / 2, each adding the partner's partials of what it keeps:
//   stage 1: m = 32, 16 exchanges (v_permlane32_swap: the two lanes' values trade places in one instruction, no select)
//   stage 2: m = 16,  8 exchanges (v_permlane16_swap)
//   stage 3: m = 8,   4 exchanges (DPP row_ror:8)          stage 4: m = 4, 2 exchanges (__shfl_xor)
//   stage 5: m = 2,   1 exchange  (DPP quad_perm)          closing: m = 1, x + x(lane ^ 1): the two halves of the pair's sum
// so bit 5 of the lane selects bit 4 of the channel, ..., bit 1 selects bit 0.  Every addition is (what the lane kept) + (what its
// partner sent), the partner computing the same two terms the other way round: the order is fixed by the lane numbers alone, and float
// addition commutes, so both lanes of the closing pair hold the same bits.
template <int kCtrl> __device__ __forceinline__ float proj_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xf, 0xf, false));
}

// one stage on the lane bit m: t[0 .. n) -> t[0 .. n / 2); the value of lane ^ m through `xchg`
template <int kN, int kMask, typename X>
__device__ __forceinline__ void proj_tr_stage(float (&t)[32], int lane, X xchg) {
    const bool up = (lane & kMask) != 0;
#pragma unroll
    for (int i = 0; i < kN / 2; ++i) {
        const float keep = up ? t[i + kN / 2] : t[i], send = up ? t[i] : t[i + kN / 2];
        t[i] = keep + xchg(send);
    }
}

template <int kMaxD> __device__ __forceinline__ float proj_transpose_sum(const float (&acc)[kMaxD], int lane) {
    static_assert(kMaxD <= 32, "the transposing reduction serves up to 32 channels");
    float t[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) t[i] = i < kMaxD ? acc[i < kMaxD ? i : 0] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {       // lanes 0-31 end with [own t[i] | the upper lane's t[i]] in r[0] / r[1], lanes 32-63 with t[i + 16]
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(t[i]), __float_as_uint(t[i + 16]), false, false);
        t[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {        // the same between the 16-lane rows: even rows keep t[i], odd rows t[i + 8]
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(t[i]), __float_as_uint(t[i + 8]), false, false);
        t[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    proj_tr_stage<8, 8>(t, lane, [](float v) { return proj_dpp<0x128>(v); });            // row_ror:8
    proj_tr_stage<4, 4>(t, lane, [](float v) { return __shfl_xor(v, 4, 64); });
    proj_tr_stage<2, 2>(t, lane, [](float v) { return proj_dpp<0x4e>(v); });             // quad_perm:[2,3,0,1]
    return t[0] + proj_dpp<0xb1>(t[0]);                                                  // quad_perm:[1,0,3,2]
}

// the lane map and its inverse: the channel of a lane, and channel j of a value spread by that map, wave-uniform (j wave-uniform)
__device__ __forceinline__ int proj_tr_channel(int lane) { return lane >> 1; }
__device__ __forceinline__ float proj_tr_read(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 2 * j));
}
// a ballot over the map -> bit j = the predicate of channel j (taken on the even lane of the pair)
__device__ __forceinline__ unsigned proj_tr_bits(unsigned long long ballot) {
    unsigned long long x = ballot & 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
    x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return (unsigned)x;
}

}  // namespace
