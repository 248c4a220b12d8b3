// Finite scalar quantizer (Mentzer et al. 2023): u = W_in z + b_in, bounded = tanh(u + shift) * half_l - offset, r = rint(bounded),
// token = mixed-radix number of (r + half_width), q = W_out (r / half_width) + b_out.  No codebook, no search: one streaming pass.
//
// All three kernels work a WAVE PER ROW on the core of proj_quant.h (up to 8 projection channels, 4 chunks per lane: D <= 1024); after the
// butterfly every lane bounds, rounds and forms the token redundantly.
// The levels and what derives from them travel BY VALUE in the launch arguments (FsqP): nothing about them is read from memory.
#include "common.h"
#include "proj_quant.h"

#include <cmath>

namespace {

constexpr int kFsqMaxD = 8;          // projection channels
constexpr int kFsqMaxChunks = 4;     // 16-byte chunks per lane: D <= 4 * 64 * 4 = 1024
constexpr int kFsqAcc = 2 * kFsqMaxD * 4 + 4 + kFsqMaxD;     // backward accumulators per lane: dW_in, dW_out, db_out, db_in = 76

struct FsqP {
    int d;
    int lv[kFsqMaxD], hw[kFsqMaxD], basis[kFsqMaxD];
    float half_l[kFsqMaxD], offset[kFsqMaxD], shift[kFsqMaxD];
};

// one channel: tanh bound, round to nearest even, clamp to the level range (a NaN lands on the lowest level: the digit is in range
// whatever u holds).  Returns r (integer valued); t = the tanh the backward differentiates.
__device__ __forceinline__ float fsq_round(const FsqP& p, int j, float u, float& t) {
    t = tanhf(u + p.shift[j]);
    const float r = rintf(t * p.half_l[j] - p.offset[j]);
    return fminf(fmaxf(r, (float)-p.hw[j]), (float)(p.lv[j] - 1 - p.hw[j]));
}

__global__ __launch_bounds__(kProjThreads) void fsq_forward_kernel(const float* __restrict__ z, const float* __restrict__ w_in,
                                                                    const float* __restrict__ b_in, const float* __restrict__ w_out,
                                                                    const float* __restrict__ b_out, int64_t n, int dm, FsqP p,
                                                                    int64_t* __restrict__ idx, float* __restrict__ u_out,
                                                                    float* __restrict__ q, bf16_raw* __restrict__ q_lo,
                                                                    int32_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) float fsq_smem[];
    const int d = p.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool want_q = q || q_lo;
    float* wi = fsq_smem;
    float* woT = fsq_smem + d * dm;
    proj_stage_weights(w_in, w_out, dm, d, 0, dm, wi, want_q ? woT : nullptr);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    int64_t row = (int64_t)blockIdx.x * kProjWaves + wave;
    float zc[kFsqMaxChunks][4], zn[kFsqMaxChunks][4];
    if (row < n) proj_load_row(z, row, dm, lane, zc);
    for (; row < n; row += stride) {
        if (row + stride < n) proj_load_row(z, row + stride, dm, lane, zn);      // the next row is in flight under this one
        float acc[kFsqMaxD];
#pragma unroll
        for (int j = 0; j < kFsqMaxD; ++j) acc[j] = 0.f;
#pragma unroll
        for (int c = 0; c < kFsqMaxChunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) proj_dot_chunk(wi, dm, d, ch, zc[c], acc);
        }
        float cj[kFsqMaxD], uj[kFsqMaxD];
        int token = 0;
#pragma unroll
        for (int j = 0; j < kFsqMaxD; ++j) {
            cj[j] = 0.f; uj[j] = 0.f;
            if (j < d) {
                float t;
                uj[j] = wave_sum(acc[j]) + b_in[j];
                const float r = fsq_round(p, j, uj[j], t);
                cj[j] = r / (float)p.hw[j];
                token += ((int)r + p.hw[j]) * p.basis[j];
            }
        }
        if (lane == 0) {
            idx[row] = token;
            if (hist) atomicAdd(hist + token, 1);
        }
        if (u_out && lane < d) {
            float v = uj[0];
#pragma unroll
            for (int j = 1; j < kFsqMaxD; ++j) v = lane == j ? uj[j] : v;
            u_out[row * d + lane] = v;
        }
        if (want_q) {
#pragma unroll
            for (int c = 0; c < kFsqMaxChunks; ++c) {
                const int ch = (c * 64 + lane) * 4;
                if (ch < dm) {
                    float o[4];
                    proj_q_chunk<kFsqMaxD>(woT, dm, d, [&](int j) { return cj[j]; }, b_out, ch, o);
                    proj_store_q(q, q_lo, row * dm + ch, o);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < kFsqMaxChunks; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) zc[c][i] = zn[c][i];
    }
}

// token -> q: digits by integer arithmetic on the index (no table: an index outside [0, K) still yields in-range digits)
__global__ __launch_bounds__(kProjThreads) void fsq_decode_kernel(const int64_t* __restrict__ idx, const float* __restrict__ w_out,
                                                                   const float* __restrict__ b_out, int64_t n, int dm, FsqP p,
                                                                   float* __restrict__ q, bf16_raw* __restrict__ q_lo) {
    extern __shared__ __attribute__((aligned(16))) float fsq_smem[];
    const int d = p.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* woT = fsq_smem;
    proj_stage_weights(nullptr, w_out, dm, d, 0, dm, nullptr, woT);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    for (int64_t row = (int64_t)blockIdx.x * kProjWaves + wave; row < n; row += stride) {
        unsigned rem = (unsigned)idx[row];
        float cj[kFsqMaxD];
#pragma unroll
        for (int j = 0; j < kFsqMaxD; ++j) {
            cj[j] = 0.f;
            if (j < d) {
                const unsigned lv = (unsigned)p.lv[j];
                const int digit = (int)(rem % lv);
                rem /= lv;
                cj[j] = (float)(digit - p.hw[j]) / (float)p.hw[j];
            }
        }
#pragma unroll
        for (int c = 0; c < kFsqMaxChunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) {
                float o[4];
                proj_q_chunk<kFsqMaxD>(woT, dm, d, [&](int j) { return cj[j]; }, b_out, ch, o);
                proj_store_q(q, q_lo, row * dm + ch, o);
            }
        }
    }
}

// Backward.  grid = (blocks over rows, 256-channel slices), see proj_quant.h: 76 accumulators per lane whatever D is, the block's waves
// added through LDS in ONE pass over all of them.
template <typename Td>
__global__ __launch_bounds__(kProjThreads) void fsq_backward_kernel(const float* __restrict__ z, const float* __restrict__ u,
                                                                     const Td* __restrict__ dq, const float* __restrict__ w_in,
                                                                     const float* __restrict__ w_out, int64_t n, int dm, FsqP p,
                                                                     float* __restrict__ dz, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float fsq_smem[];
    const int d = p.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.y * kProjSlice;
    const int cn = dm - c0 < kProjSlice ? dm - c0 : kProjSlice;
    float* woT = fsq_smem;                       // [d][dm]
    float* wi = woT + d * dm;                    // [d][cn]
    float* red = wi + d * kProjSlice;            // [kFsqAcc][64]
    proj_stage_weights(w_in, w_out, dm, d, c0, cn, wi, woT);
    __syncthreads();
    const int own = lane * 4;                    // channel inside the slice
    const bool has = own < cn;
    const int nchunks = (dm + 255) / 256;
    float a_wi[kFsqMaxD][4], a_wo[kFsqMaxD][4], a_bo[4], a_bi[kFsqMaxD];
#pragma unroll
    for (int j = 0; j < kFsqMaxD; ++j) {
        a_bi[j] = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { a_wi[j][i] = 0.f; a_wo[j][i] = 0.f; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) a_bo[i] = 0.f;

    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    for (int64_t row = (int64_t)blockIdx.x * kProjWaves + wave; row < n; row += stride) {
        float g[kFsqMaxD], dqo[4] = {0.f, 0.f, 0.f, 0.f}, zo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kFsqMaxD; ++j) g[j] = 0.f;
        float ur[kFsqMaxD];
#pragma unroll
        for (int j = 0; j < kFsqMaxD; ++j) ur[j] = j < d ? u[row * d + j] : 0.f;
        if (has) Vec16<float>::load(z + row * dm + c0 + own, zo);
        for (int c = 0; c < nchunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) {
                float v[4];
                proj_load4<Td>(dq + row * dm + ch, v);
                if (c == (int)blockIdx.y) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) dqo[i] = v[i];
                }
                proj_dot_chunk(woT, dm, d, ch, v, g);
            }
        }
        float dzo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kFsqMaxD; ++j)
            if (j < d) {
                float t;
                const float hw = (float)p.hw[j];
                const float cj = fsq_round(p, j, ur[j], t) / hw;
                const float du = wave_sum(g[j]) / hw * p.half_l[j] * (1.f - t * t);      // straight-through: d r / d bounded = 1
                a_bi[j] += du;
                if (has) proj_accumulate(wi + j * cn + own, du, cj, zo, dqo, dzo, a_wi[j], a_wo[j]);
            }
        if (has) proj_finish_row(dz + row * dm + c0 + own, dzo, dqo, a_bo);
    }

    // the block's waves, added to wave 0 in wave order
    for (int w = 1; w < kProjWaves; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < kFsqMaxD; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    red[(j * 4 + i) * 64 + lane] = a_wi[j][i];
                    red[(32 + j * 4 + i) * 64 + lane] = a_wo[j][i];
                }
                red[(68 + j) * 64 + lane] = a_bi[j];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) red[(64 + i) * 64 + lane] = a_bo[i];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int j = 0; j < kFsqMaxD; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a_wi[j][i] += red[(j * 4 + i) * 64 + lane];
                    a_wo[j][i] += red[(32 + j * 4 + i) * 64 + lane];
                }
                a_bi[j] += red[(68 + j) * 64 + lane];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) a_bo[i] += red[(64 + i) * 64 + lane];
        }
    }
    if (wave != 0) return;
    float* s_bi = proj_store_slab(ws, dm, d, c0 + own, has, a_wi, a_wo, a_bo);
    if (blockIdx.y == 0 && lane == 0) {
#pragma unroll
        for (int j = 0; j < kFsqMaxD; ++j)
            if (j < d) s_bi[j] = a_bi[j];
    }
}

// levels (host) -> launch arguments; VQK_ERR_SHAPE for what the kernels do not serve
int fsq_params(int dm, int d, const int32_t* levels, FsqP& p) {
    VQK_REQUIRE(dm >= 4 && dm <= 4 * 64 * kFsqMaxChunks && (dm % 4) == 0 && d >= 1 && d <= kFsqMaxD, VQK_ERR_SHAPE);
    int64_t k = 1;
    p = FsqP{};
    p.d = d;
    for (int j = 0; j < kFsqMaxD; ++j) {
        const int lv = j < d ? levels[j] : 2;
        VQK_REQUIRE(lv >= 2, VQK_ERR_SHAPE);
        p.lv[j] = lv;
        p.hw[j] = lv / 2;
        p.basis[j] = j < d ? (int)k : 0;
        const double half_l = (lv - 1) * (1.0 + 1e-3) / 2.0, offset = (lv % 2 == 0) ? 0.5 : 0.0;
        p.half_l[j] = (float)half_l;
        p.offset[j] = (float)offset;
        p.shift[j] = (float)std::atanh(offset / half_l);
        if (j < d) k *= lv;
        VQK_REQUIRE(k < ((int64_t)1 << 31), VQK_ERR_SHAPE);
    }
    return VQK_OK;
}

int fsq_row_blocks(int64_t n, int rows_per_block, int cap) { return vqk_grid_1d(n, rows_per_block, cap); }
int fsq_backward_blocks(int64_t n) { return fsq_row_blocks(n, 4 * kProjWaves, 256); }      // a function of n only: the same sums every run

}  // namespace

extern "C" {

int vqk_fsq_forward(const float* z, const float* w_in, const float* b_in, const float* w_out, const float* b_out, int64_t n,
                    int dm, int d, const int32_t* levels, int64_t* idx, float* u, float* q, void* q_lo, int32_t* hist,
                    void* stream) {
    VQK_REQUIRE(levels, VQK_ERR_ARG);
    FsqP p;
    if (const int st = fsq_params(dm, d, levels, p)) return st;
    VQK_REQUIRE(n >= 0 && z && w_in && b_in && idx, VQK_ERR_ARG);
    VQK_REQUIRE(!(q || q_lo) || (w_out && b_out), VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(q) && vqk_aligned16(q_lo), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    const size_t lds = (size_t)((q || q_lo) ? 2 : 1) * d * dm * sizeof(float);
    hipLaunchKernelGGL(fsq_forward_kernel, dim3((unsigned)fsq_row_blocks(n, 4 * kProjWaves, 512)), dim3(kProjThreads), lds,
                       vqk_stream(stream), z, w_in, b_in, w_out, b_out, n, dm, p, idx, u, q, reinterpret_cast<bf16_raw*>(q_lo), hist);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_fsq_decode(const int64_t* idx, const float* w_out, const float* b_out, int64_t n, int dm, int d, const int32_t* levels,
                   float* q, void* q_lo, void* stream) {
    VQK_REQUIRE(levels, VQK_ERR_ARG);
    FsqP p;
    if (const int st = fsq_params(dm, d, levels, p)) return st;
    VQK_REQUIRE(n >= 0 && idx && w_out && b_out && (q || q_lo), VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(q) && vqk_aligned16(q_lo), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    hipLaunchKernelGGL(fsq_decode_kernel, dim3((unsigned)fsq_row_blocks(n, 4 * kProjWaves, 512)), dim3(kProjThreads),
                       (size_t)d * dm * sizeof(float), vqk_stream(stream), idx, w_out, b_out, n, dm, p, q,
                       reinterpret_cast<bf16_raw*>(q_lo));
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int64_t vqk_fsq_backward_ws_bytes(int64_t n, int dm, int d) {
    if (n < 0 || dm < 4 || dm > 4 * 64 * kFsqMaxChunks || (dm % 4) || d < 1 || d > kFsqMaxD) return VQK_ERR_SHAPE;
    return (int64_t)fsq_backward_blocks(n) * proj_slab_floats(dm, d) * (int64_t)sizeof(float);
}

int vqk_fsq_backward(const float* z, const float* u, const void* dq, int dq_dtype, const float* w_in, const float* w_out, int64_t n,
                     int dm, int d, const int32_t* levels, float* dz, float* dw_in, float* db_in, float* dw_out, float* db_out,
                     int accumulate, void* ws, int64_t ws_bytes, void* stream) {
    VQK_REQUIRE(levels, VQK_ERR_ARG);
    FsqP p;
    if (const int st = fsq_params(dm, d, levels, p)) return st;
    VQK_REQUIRE(n >= 0 && ws_bytes >= 0 && z && u && dq && w_in && w_out && dz && dw_in && db_in && dw_out && db_out && ws, VQK_ERR_ARG);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(dq) && vqk_aligned16(dz) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqk_fsq_backward_ws_bytes(n, dm, d), VQK_ERR_WORKSPACE);
    const int blocks = n > 0 ? fsq_backward_blocks(n) : 0;
    if (n > 0) {
        const dim3 grid((unsigned)blocks, (unsigned)((dm + kProjSlice - 1) / kProjSlice));
        const size_t lds = ((size_t)d * dm + (size_t)d * kProjSlice + (size_t)kFsqAcc * 64) * sizeof(float);
        float* wsf = reinterpret_cast<float*>(ws);
        if (dq_dtype == VQK_F32)
            hipLaunchKernelGGL(fsq_backward_kernel<float>, grid, dim3(kProjThreads), lds, vqk_stream(stream), z, u, (const float*)dq, w_in,
                               w_out, n, dm, p, dz, wsf);
        else
            hipLaunchKernelGGL(fsq_backward_kernel<bf16_raw>, grid, dim3(kProjThreads), lds, vqk_stream(stream), z, u,
                               (const bf16_raw*)dq, w_in, w_out, n, dm, p, dz, wsf);
        VQK_CHECK_LAUNCH();
    }
    return proj_launch_slab_sum(ws, blocks, dm, d, accumulate, dw_in, db_in, dw_out, db_out, vqk_stream(stream));
}

}  // extern "C"
