// The core the sign quantizers share (lfq.hip, bsq.hip) on top of proj_quant.h: c_j = +-s by the sign of channel j, token = the bit
// pattern, loss = beta commit + w (H_sample - gamma H_batch) with p_nj = sigmoid(a u_nj).  The softmax over the 2^d sign codes
// factorises into d sigmoids, so H_sample costs d terms per row, and the batch-average distribution is kept per GROUP of g consecutive
// bits (tables of 2^g entries): what is per group CODE runs on the lane whose id equals the code's low 6 bits, looping over the
// remaining 2^(g_s - 6) codes.  Every sum over rows is ordered: registers / wave-private LDS tables over the rows of a wave (fixed by
// the grid), the block's waves in wave order, one slab per block in the workspace, a second launch that adds the slabs in an order
// fixed by their count.  No fp32 atomics.
//
// Held here once: the limits, the parameter structs, the code functor, the stable sigmoid / entropy form, the group-table products
// (parametrised by the lane stride of the channel map: channel j on lane j in lfq.hip, on lane 2 j in bsq.hip), the forward's slab
// store and ordered slab sum, the finish and decode kernels, and the host side of the three launchers.  Pieces, not a framework: each
// kernel keeps its own barriers, LDS carve-up and accumulators and calls a piece between them.  A quantizer's file keeps its forward
// and backward kernel bodies -- channel layout, normalisation, the step from the projection to the code and from the cotangent to du
// -- and describes itself to the launchers with a SignKind.
// Written out in the files on purpose: lfq_forward_kernel's partial-projection loop (its comment has the figures), lfq_own, and the
// backward's two-pass reduction over the block's waves: as a helper here (accumulators by reference, the loops unchanged) it took
// lfq_backward_kernel from 232 to 234 VGPRs and bsq_backward_kernel from 231 to 233, for either cotangent type.
#pragma once
#include "common.h"
#include "proj_quant.h"

#include <cmath>

namespace {

constexpr int kSignMaxBits = 18;     // projection channels
constexpr int kSignMaxGroup = 10;    // bits per entropy group: tables of at most 1024 entries
constexpr int kSignMaxChunks = 2;    // 16-byte chunks per lane: D <= 2 * 64 * 4 = 512
constexpr int kSignMaxD = 4 * 64 * kSignMaxChunks;
constexpr int kSignRed = kSignMaxBits * 4 + 4;    // floats per lane of one block-reduction pass: 72 + (db_out 4 | db_in 1)
constexpr int kSignFinish = 1024;    // threads of the forward's finish launch
constexpr float kSignEps = 1e-10f;   // the epsilon of get_codebook_usage

struct SignP {
    int d, g, groups, pitch, tab;    // bits, bits per group, ceil(d / g), 1 << g, groups << g (floats of the group tables)
    float a, s;                      // logit of bit j = a u_j;  |c_j|
};

struct SignLossP {
    float c_commit, c_hs, c_hb;      // 2 beta / (N commit_d),  w a^2 / N,  w gamma a / N: the loss gradient at u without the cotangent
};

// what a quantizer's file tells the launchers about itself.  LFQ: a = 4 / tau, s = 1, commit a mean over rows AND channels (commit_d
// = d); BSQ: a = 4 s / tau, s = 1 / sqrt(d), commit a sum over channels and a mean over rows (commit_d = 1).  a_loss is a as the
// loss coefficients of the backward take it (in double)
struct SignKind {
    float a, s;
    double a_loss;
    int commit_d;
};

// the largest table over the served (d, g): d = 18, g = 10 -> 2 groups of 1024
constexpr int kSignMaxTab = 2 << kSignMaxGroup;
constexpr int kSignFwdLds = (2 * kSignMaxBits * kSignMaxD + kProjWaves * kSignMaxTab + 2 * kProjWaves) * 4;
constexpr int kSignBwdLds = (kSignMaxBits * kSignMaxD + kSignMaxBits * kProjSlice + kSignMaxTab + kSignRed * 64) * 4;

// channel j's code out of the token: bit j set: c_j = +s, else -s
struct SignCode {
    unsigned token;
    float s;
    __device__ __forceinline__ float operator()(int j) const { return ((token >> j) & 1u) ? s : -s; }
};

// one channel: p = sigmoid(x), pm = sigmoid(-x) (computed as such: e / (1 + e), never 1 - p), h = the binary entropy in the stable
// form log1p(exp(-|x|)) + |x| sigmoid(-|x|)
__device__ __forceinline__ void sign_sigmoid(float x, float& p, float& pm, float& h) {
    const float ax = fabsf(x), e = expf(-ax), den = 1.f + e;
    const float small = e / den, big = 1.f / den;      // sigmoid(-|x|), sigmoid(|x|)
    p = x >= 0.f ? big : small;
    pm = x >= 0.f ? small : big;
    h = log1pf(e) + ax * small;
}

// The codes of group s a lane owns are m = lane + 64 t: the product over the low (<= 6) bits depends on the lane, the product over the
// high bits on t alone.  p / pm hold channel j on lane kStride j.  Returns the low product (0 on a lane past the group's codes) and
// the high bits' probabilities, wave-uniform.
template <int kStride>
__device__ __forceinline__ float sign_group_low(float p, float pm, int base, int gs, int lane, float (&ph)[4], float (&pmh)[4]) {
    const int low = gs < 6 ? gs : 6;
    float prod = lane < (1 << low) ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (i < low) {
            const float pi = __shfl(p, kStride * (base + i), 64), pmi = __shfl(pm, kStride * (base + i), 64);
            prod *= ((lane >> i) & 1) ? pi : pmi;
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = 6 + i < gs ? base + 6 + i : 0;
        ph[i] = __shfl(p, kStride * j, 64);
        pmh[i] = __shfl(pm, kStride * j, 64);
    }
    return prod;
}

__device__ __forceinline__ float sign_group_high(const float (&ph)[4], const float (&pmh)[4], int gs, int t) {
    float prod = 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (6 + i < gs) prod *= ((t >> i) & 1) ? ph[i] : pmh[i];
    return prod;
}

// slab of one forward block (floats): [group tables p.tab][commit sum][sum_j h], padded to a multiple of 4
__host__ __device__ inline int64_t sign_fwd_slab_floats(int tab) { return ((int64_t)tab + 2 + 3) & ~(int64_t)3; }

// forward tail, after the barrier behind the waves' last table update and their two sums in red [waves][2]: the block's waves in wave
// order, one slab per block: plain stores, every element written
__device__ __forceinline__ void sign_store_fwd_slab(float* ws, const float* tabs, const float* red, int tab) {
    float* slab = ws + (int64_t)blockIdx.x * sign_fwd_slab_floats(tab);
    for (int i = threadIdx.x; i < tab; i += kProjThreads) {
        float s = tabs[i];
        for (int w = 1; w < kProjWaves; ++w) s += tabs[w * tab + i];
        slab[i] = s;
    }
    if (threadIdx.x < 2) {
        float s = red[threadIdx.x];
        for (int w = 1; w < kProjWaves; ++w) s += red[w * 2 + threadIdx.x];
        slab[tab + threadIdx.x] = s;
    }
}

// element e of every slab, added in an order fixed by the slab count: eight running sums over the slab index (b % 8), combined pairwise
__device__ __forceinline__ float sign_slab_column(const float* src, int slabs, int64_t pitch) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int b = 0;
    for (; b + 8 <= slabs; b += 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] += src[(b + i) * pitch];
    }
    for (; b < slabs; ++b) s[0] += src[b * pitch];
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// The forward's second launch, ONE block: Pbar = table sums / N, L = log(Pbar + eps) + Pbar / (Pbar + eps) for the backward, H_batch =
// -sum Pbar log(Pbar + eps) (a fixed tree over the threads), out = [loss, commit, H_sample, H_batch]; commit = the commitment sum /
// commit_div (N d or N).  An entry of a ragged last group's table past its 2^g_s codes holds 0 and adds -0 log(eps) = 0.
__global__ __launch_bounds__(kSignFinish) void sign_finish_kernel(const float* __restrict__ ws, int slabs, SignP p, float n_rows,
                                                                    float commit_div, float beta, float ratio, float gamma,
                                                                    float* __restrict__ out, float* __restrict__ ltab) {
    __shared__ float red[kSignFinish];
    __shared__ float sums[2];
    const int64_t pitch = sign_fwd_slab_floats(p.tab);
    float term = 0.f;
    for (int e = threadIdx.x; e < p.tab + 2; e += kSignFinish) {
        const float s = sign_slab_column(ws + e, slabs, pitch);
        if (e < p.tab) {
            const float pbar = s / n_rows, lg = logf(pbar + kSignEps);
            ltab[e] = lg + pbar / (pbar + kSignEps);
            term -= pbar * lg;
        } else {
            sums[e - p.tab] = s;
        }
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int off = kSignFinish / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float commit = sums[0] / commit_div, h_sample = sums[1] / n_rows, h_batch = red[0];
        out[0] = beta * commit + ratio * (h_sample - gamma * h_batch);
        out[1] = commit;
        out[2] = h_sample;
        out[3] = h_batch;
    }
}

// token -> q by bit arithmetic on the index (no table: any int64 yields a valid sign vector)
__global__ __launch_bounds__(kProjThreads) void sign_decode_kernel(const int64_t* __restrict__ idx, const float* __restrict__ w_out,
                                                                    const float* __restrict__ b_out, int64_t n, int dm, int d, float s,
                                                                    float* __restrict__ q, bf16_raw* __restrict__ q_lo) {
    extern __shared__ __attribute__((aligned(16))) float sign_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* woT = sign_smem;
    proj_stage_weights(nullptr, w_out, dm, d, 0, dm, nullptr, woT);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    for (int64_t row = (int64_t)blockIdx.x * kProjWaves + wave; row < n; row += stride) {
        const unsigned token = (unsigned)idx[row];
#pragma unroll
        for (int c = 0; c < kSignMaxChunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) {
                float o[4];
                proj_q_chunk<kSignMaxBits>(woT, dm, d, SignCode{token, s}, b_out, ch, o);
                proj_store_q(q, q_lo, row * dm + ch, o);
            }
        }
    }
}

// ---- the host side ----

// (D, bits, group bits, tau) -> launch arguments; VQK_ERR_SHAPE for what the kernels do not serve
inline int sign_params(int dm, int d, int g, float tau, const SignKind& kind, SignP& p) {
    VQK_REQUIRE(dm >= 4 && dm <= kSignMaxD && (dm % 4) == 0 && d >= 1 && d <= kSignMaxBits && g >= 1 && g <= kSignMaxGroup, VQK_ERR_SHAPE);
    VQK_REQUIRE(tau > 0.f, VQK_ERR_ARG);
    p.d = d;
    p.g = g;
    p.groups = (d + g - 1) / g;
    p.pitch = 1 << g;
    p.tab = p.groups << g;
    p.a = kind.a;
    p.s = kind.s;
    return VQK_OK;
}

// a function of n only: the same sums every run
inline int sign_blocks(int64_t n) { return vqk_grid_1d(n, 4 * kProjWaves, 256); }

inline int64_t sign_ws_bytes(int64_t n, int dm, int d, int g) {
    SignP p;
    if (n < 0) return VQK_ERR_SHAPE;
    if (const int st = sign_params(dm, d, g, 1.f, SignKind{}, p)) return st;
    const int64_t fwd = sign_fwd_slab_floats(p.tab), bwd = proj_slab_floats(dm, d);
    return (int64_t)sign_blocks(n) * (fwd > bwd ? fwd : bwd) * (int64_t)sizeof(float);
}

// `kernel` is the file's forward kernel; r...: what it takes between u and q (BSQ's 1 / |v| per row)
template <typename K, typename... R>
int sign_forward(K kernel, const SignKind& kind, const float* z, const float* w_in, const float* b_in, const float* w_out,
                 const float* b_out, int64_t n, int dm, int d, int g, float tau, float beta, float ratio, float gamma, int64_t* idx,
                 float* u, float* q, void* q_lo, int32_t* hist, float* out, float* ltab, void* ws, int64_t ws_bytes, void* stream,
                 R... r) {
    SignP p;
    if (const int st = sign_params(dm, d, g, tau, kind, p)) return st;
    VQK_REQUIRE(n >= 0 && ws_bytes >= 0 && z && w_in && b_in && idx, VQK_ERR_ARG);
    VQK_REQUIRE(!(q || q_lo) || (w_out && b_out), VQK_ERR_ARG);
    VQK_REQUIRE((out != nullptr) == (ltab != nullptr) && (out != nullptr) == (ws != nullptr), VQK_ERR_ARG);     // the loss: all three or none
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(q) && vqk_aligned16(q_lo) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(!ws || ws_bytes >= sign_ws_bytes(n, dm, d, g), VQK_ERR_WORKSPACE);
    const int blocks = n > 0 ? sign_blocks(n) : 0;
    hipStream_t st = vqk_stream(stream);
    if (n > 0) {
        static const hipError_t attr = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSignFwdLds);
        if (attr != hipSuccess) return VQK_ERR_LAUNCH;
        const size_t lds = ((size_t)((q || q_lo) ? 2 : 1) * d * dm + (ws ? (size_t)kProjWaves * p.tab + 2 * kProjWaves : 0)) * sizeof(float);
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kProjThreads), lds, st, z, w_in, b_in, w_out, b_out, n, dm, p, idx, u,
                           r..., q, reinterpret_cast<bf16_raw*>(q_lo), hist, reinterpret_cast<float*>(ws));
        VQK_CHECK_LAUNCH();
    }
    if (out) {
        const float n_rows = (float)(n > 0 ? n : 1);
        hipLaunchKernelGGL(sign_finish_kernel, dim3(1), dim3(kSignFinish), 0, st, reinterpret_cast<const float*>(ws), blocks, p, n_rows,
                           n_rows * (float)kind.commit_d, beta, ratio, gamma, out, ltab);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

inline int sign_decode(const SignKind& kind, const int64_t* idx, const float* w_out, const float* b_out, int64_t n, int dm, int d,
                       float* q, void* q_lo, void* stream) {
    SignP p;
    if (const int st = sign_params(dm, d, 1, 1.f, kind, p)) return st;
    VQK_REQUIRE(n >= 0 && idx && w_out && b_out && (q || q_lo), VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(q) && vqk_aligned16(q_lo), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    hipLaunchKernelGGL(sign_decode_kernel, dim3((unsigned)sign_blocks(n)), dim3(kProjThreads), (size_t)d * dm * sizeof(float),
                       vqk_stream(stream), idx, w_out, b_out, n, dm, d, p.s, q, reinterpret_cast<bf16_raw*>(q_lo));
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

// k32 / k16: the file's backward kernel for an fp32 / a bf16 cotangent; r...: what it takes between u and dq
template <typename K32, typename K16, typename... R>
int sign_backward(K32 k32, K16 k16, const SignKind& kind, const float* z, const float* u, const void* dq, int dq_dtype,
                  const float* w_in, const float* w_out, const float* ltab, const float* gscale_dev, int64_t n, int dm, int d, int g,
                  float tau, float beta, float ratio, float gamma, float* dz, float* dw_in, float* db_in, float* dw_out, float* db_out,
                  int accumulate, void* ws, int64_t ws_bytes, void* stream, R... r) {
    SignP p;
    if (const int st = sign_params(dm, d, g, tau, kind, p)) return st;
    VQK_REQUIRE(n >= 0 && ws_bytes >= 0 && z && u && (... && r) && dq && w_in && w_out && ltab && dz && dw_in && db_in && dw_out &&
                    db_out && ws, VQK_ERR_ARG);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(dq) && vqk_aligned16(dz) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= sign_ws_bytes(n, dm, d, g), VQK_ERR_WORKSPACE);
    const int blocks = n > 0 ? sign_blocks(n) : 0;
    hipStream_t st = vqk_stream(stream);
    if (n > 0) {
        const double nn = (double)n, a = kind.a_loss;
        const SignLossP lp = {(float)(2.0 * beta / (nn * kind.commit_d)), (float)((double)ratio * a * a / nn),
                              (float)((double)ratio * gamma * a / nn)};
        const dim3 grid((unsigned)blocks, (unsigned)((dm + kProjSlice - 1) / kProjSlice));
        const size_t lds = ((size_t)d * dm + (size_t)d * kProjSlice + (size_t)p.tab + (size_t)kSignRed * 64) * sizeof(float);
        float* wsf = reinterpret_cast<float*>(ws);
        if (dq_dtype == VQK_F32) {
            static const hipError_t attr = hipFuncSetAttribute((const void*)k32, hipFuncAttributeMaxDynamicSharedMemorySize, kSignBwdLds);
            if (attr != hipSuccess) return VQK_ERR_LAUNCH;
            hipLaunchKernelGGL(k32, grid, dim3(kProjThreads), lds, st, z, u, r..., (const float*)dq, w_in, w_out, ltab, gscale_dev, n, dm,
                               p, lp, dz, wsf);
        } else {
            static const hipError_t attr = hipFuncSetAttribute((const void*)k16, hipFuncAttributeMaxDynamicSharedMemorySize, kSignBwdLds);
            if (attr != hipSuccess) return VQK_ERR_LAUNCH;
            hipLaunchKernelGGL(k16, grid, dim3(kProjThreads), lds, st, z, u, r..., (const bf16_raw*)dq, w_in, w_out, ltab, gscale_dev, n,
                               dm, p, lp, dz, wsf);
        }
        VQK_CHECK_LAUNCH();
    }
    return proj_launch_slab_sum(ws, blocks, dm, d, accumulate, dw_in, db_in, dw_out, db_out, st);
}

}  // namespace
