// Lookup-free quantizer (Yu et al. 2023, MAGVIT-v2; Open-MAGVIT2): u = W_in z + b_in, c_j = sign(u_j) (+1 iff u_j > 0), token = the bit
// pattern of (u_j > 0) (first channel = bit 0), q = W_out c + b_out, loss = beta commit + w (H_sample - gamma H_batch) with
// p_nj = sigmoid(a u_nj), a = 4 / tau: the softmax over the 2^d sign codes factorises into d sigmoids, so H_sample costs d terms per
// row, and the batch-average distribution is kept per GROUP of g consecutive bits (tables of 2^g entries).  No codebook, no search.
//
// The kernels work a WAVE PER ROW on the core of proj_quant.h (up to 18 projection channels, 2 chunks per lane: D <= 512).
// What is per CHANNEL (sigmoid, entropy term, commitment term) runs once per row on lane j for channel j; what is per group CODE runs
// on the lane whose id equals the code's low 6 bits, looping over the remaining 2^(g_s - 6) codes.
// Every sum over rows is ordered: registers / wave-private LDS tables over the rows of a wave (fixed by the grid), the block's waves in
// wave order, one slab per block in the workspace, a second launch that adds the slabs in an order fixed by their count.  No fp32 atomics.
#include "common.h"
#include "proj_quant.h"

#include <cmath>

namespace {

constexpr int kLfqMaxBits = 18;      // projection channels
constexpr int kLfqMaxGroup = 10;     // bits per entropy group: tables of at most 1024 entries
constexpr int kLfqMaxChunks = 2;     // 16-byte chunks per lane: D <= 2 * 64 * 4 = 512
constexpr int kLfqMaxD = 4 * 64 * kLfqMaxChunks;
constexpr int kLfqRed = kLfqMaxBits * 4 + 4;      // floats per lane of one block-reduction pass: 72 + (db_out 4 | db_in 1)
constexpr int kLfqFinish = 1024;     // threads of the forward's finish launch
constexpr float kLfqEps = 1e-10f;    // the epsilon of get_codebook_usage

struct LfqP {
    int d, g, groups, pitch, tab;    // bits, bits per group, ceil(d / g), 1 << g, groups << g (floats of the group tables)
    float a;                         // 4 / tau: logit of bit j = a u_j
};

// the largest table over the served (d, g): d = 18, g = 10 -> 2 groups of 1024
constexpr int kLfqMaxTab = 2 << kLfqMaxGroup;
constexpr int kLfqFwdLds = (2 * kLfqMaxBits * kLfqMaxD + kProjWaves * kLfqMaxTab + 2 * kProjWaves) * 4;
constexpr int kLfqBwdLds = (kLfqMaxBits * kLfqMaxD + kLfqMaxBits * kProjSlice + kLfqMaxTab + kLfqRed * 64) * 4;

// channel j's code out of the token: bit j set: c_j = +1, else -1
struct LfqCode {
    unsigned token;
    __device__ __forceinline__ float operator()(int j) const { return ((token >> j) & 1u) ? 1.f : -1.f; }
};

// the value lane `lane` owns out of a wave-uniform register array (0 for lane >= d)
__device__ __forceinline__ float lfq_own(const float (&v)[kLfqMaxBits], int lane) {
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < kLfqMaxBits; ++j) r = lane == j ? v[j] : r;
    return r;
}

// one channel: p = sigmoid(x), pm = sigmoid(-x) (computed as such: e / (1 + e), never 1 - p), h = the binary entropy in the stable
// form log1p(exp(-|x|)) + |x| sigmoid(-|x|)
__device__ __forceinline__ void lfq_sigmoid(float x, float& p, float& pm, float& h) {
    const float ax = fabsf(x), e = expf(-ax), den = 1.f + e;
    const float small = e / den, big = 1.f / den;      // sigmoid(-|x|), sigmoid(|x|)
    p = x >= 0.f ? big : small;
    pm = x >= 0.f ? small : big;
    h = log1pf(e) + ax * small;
}

// The codes of group s a lane owns are m = lane + 64 t: the product over the low (<= 6) bits depends on the lane, the product over the
// high bits on t alone.  p / pm hold channel j on lane j.  Returns the low product (0 on a lane past the group's codes) and the high
// bits' probabilities, wave-uniform.
__device__ __forceinline__ float lfq_group_low(float p, float pm, int base, int gs, int lane, float (&ph)[4], float (&pmh)[4]) {
    const int low = gs < 6 ? gs : 6;
    float prod = lane < (1 << low) ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (i < low) {
            const float pi = __shfl(p, base + i, 64), pmi = __shfl(pm, base + i, 64);
            prod *= ((lane >> i) & 1) ? pi : pmi;
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = 6 + i < gs ? base + 6 + i : 0;
        ph[i] = __shfl(p, j, 64);
        pmh[i] = __shfl(pm, j, 64);
    }
    return prod;
}

__device__ __forceinline__ float lfq_group_high(const float (&ph)[4], const float (&pmh)[4], int gs, int t) {
    float prod = 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (6 + i < gs) prod *= ((t >> i) & 1) ? ph[i] : pmh[i];
    return prod;
}

// slab of one forward block (floats): [group tables p.tab][commit sum][sum_j h], padded to a multiple of 4
__host__ __device__ inline int64_t lfq_fwd_slab_floats(int tab) { return ((int64_t)tab + 2 + 3) & ~(int64_t)3; }

// Forward.  ws == nullptr: assignment only (no loss, no tables).
__global__ __launch_bounds__(kProjThreads) void lfq_forward_kernel(const float* __restrict__ z, const float* __restrict__ w_in,
                                                                    const float* __restrict__ b_in, const float* __restrict__ w_out,
                                                                    const float* __restrict__ b_out, int64_t n, int dm, LfqP p,
                                                                    int64_t* __restrict__ idx, float* __restrict__ u_out,
                                                                    float* __restrict__ q, bf16_raw* __restrict__ q_lo,
                                                                    int32_t* __restrict__ hist, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float lfq_smem[];
    const int d = p.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool want_q = q || q_lo;
    float* wi = lfq_smem;                                        // [d][dm]
    float* woT = wi + d * dm;                                    // [d][dm] when q is wanted
    float* tabs = woT + (want_q ? d * dm : 0);                   // [waves][p.tab] when the loss is wanted
    float* red = tabs + (ws ? kProjWaves * p.tab : 0);           // [waves][2]
    proj_stage_weights(w_in, w_out, dm, d, 0, dm, wi, want_q ? woT : nullptr);
    if (ws)
        for (int i = threadIdx.x; i < kProjWaves * p.tab; i += kProjThreads) tabs[i] = 0.f;
    __syncthreads();
    float* tab = tabs + wave * p.tab;                            // this wave's own tables: no other wave touches them before the end
    float a_commit = 0.f, a_h = 0.f;                             // lane j: channel j over the rows of this wave

    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    int64_t row = (int64_t)blockIdx.x * kProjWaves + wave;
    float zc[kLfqMaxChunks][4], zn[kLfqMaxChunks][4];
    if (row < n) proj_load_row(z, row, dm, lane, zc);
    for (; row < n; row += stride) {
        if (row + stride < n) proj_load_row(z, row + stride, dm, lane, zn);      // the next row is in flight under this one
        float uj[kLfqMaxBits];
#pragma unroll
        for (int j = 0; j < kLfqMaxBits; ++j) uj[j] = 0.f;
#pragma unroll
        for (int c = 0; c < kLfqMaxChunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) {
                // proj_dot_chunk, written out: through the helper this kernel is allocated 94 VGPRs instead of 98 and scheduled anew
#pragma unroll
                for (int j = 0; j < kLfqMaxBits; ++j)
                    if (j < d) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(wi + j * dm + ch);
#pragma unroll
                        for (int i = 0; i < 4; ++i) uj[j] = fmaf(zc[c][i], w[i], uj[j]);
                    }
            }
        }
        unsigned token = 0;
#pragma unroll
        for (int j = 0; j < kLfqMaxBits; ++j)
            if (j < d) {
                uj[j] = wave_sum(uj[j]) + b_in[j];
                token |= (uj[j] > 0.f ? 1u : 0u) << j;          // a zero or a NaN: bit clear, c = -1
            }
        if (lane == 0) {
            idx[row] = (int64_t)token;
            if (hist) atomicAdd(hist + token, 1);
        }
        const float mine = lfq_own(uj, lane);
        if (u_out && lane < d) u_out[row * d + lane] = mine;
        if (want_q) {
#pragma unroll
            for (int c = 0; c < kLfqMaxChunks; ++c) {
                const int ch = (c * 64 + lane) * 4;
                if (ch < dm) {
                    float o[4];
                    proj_q_chunk<kLfqMaxBits>(woT, dm, d, LfqCode{token}, b_out, ch, o);
                    proj_store_q(q, q_lo, row * dm + ch, o);
                }
            }
        }
        if (ws) {
            float pj, pmj, hj;
            lfq_sigmoid(p.a * mine, pj, pmj, hj);
            if (lane < d) {
                const float diff = mine - (mine > 0.f ? 1.f : -1.f);
                a_commit = fmaf(diff, diff, a_commit);
                a_h += hj;
            }
            for (int s = 0; s < p.groups; ++s) {
                const int base = s * p.g, gs = d - base < p.g ? d - base : p.g;
                float ph[4], pmh[4];
                const float low = lfq_group_low(pj, pmj, base, gs, lane, ph, pmh);
                const int nt = gs > 6 ? 1 << (gs - 6) : 1;
                if (lane < (1 << (gs < 6 ? gs : 6)))
                    for (int t = 0; t < nt; ++t) tab[s * p.pitch + t * 64 + lane] += low * lfq_group_high(ph, pmh, gs, t);
            }
        }
#pragma unroll
        for (int c = 0; c < kLfqMaxChunks; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) zc[c][i] = zn[c][i];
    }
    if (!ws) return;
    // the block's waves in wave order, one slab per block: plain stores, every element written
    const float c_sum = wave_sum(a_commit), h_sum = wave_sum(a_h);
    if (lane == 0) { red[wave * 2] = c_sum; red[wave * 2 + 1] = h_sum; }
    __syncthreads();
    float* slab = ws + (int64_t)blockIdx.x * lfq_fwd_slab_floats(p.tab);
    for (int i = threadIdx.x; i < p.tab; i += kProjThreads) {
        float s = tabs[i];
        for (int w = 1; w < kProjWaves; ++w) s += tabs[w * p.tab + i];
        slab[i] = s;
    }
    if (threadIdx.x < 2) {
        float s = red[threadIdx.x];
        for (int w = 1; w < kProjWaves; ++w) s += red[w * 2 + threadIdx.x];
        slab[p.tab + threadIdx.x] = s;
    }
}

// element e of every slab, added in an order fixed by the slab count: eight running sums over the slab index (b % 8), combined pairwise
__device__ __forceinline__ float lfq_slab_column(const float* src, int slabs, int64_t pitch) {
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
// -sum Pbar log(Pbar + eps) (a fixed tree over the threads), out = [loss, commit, H_sample, H_batch].  An entry of a ragged last group's
// table past its 2^g_s codes holds 0 and adds -0 log(eps) = 0.
__global__ __launch_bounds__(kLfqFinish) void lfq_finish_kernel(const float* __restrict__ ws, int slabs, LfqP p, float n_rows, float beta,
                                                                  float ratio, float gamma, float* __restrict__ out,
                                                                  float* __restrict__ ltab) {
    __shared__ float red[kLfqFinish];
    __shared__ float sums[2];
    const int64_t pitch = lfq_fwd_slab_floats(p.tab);
    float term = 0.f;
    for (int e = threadIdx.x; e < p.tab + 2; e += kLfqFinish) {
        const float s = lfq_slab_column(ws + e, slabs, pitch);
        if (e < p.tab) {
            const float pbar = s / n_rows, lg = logf(pbar + kLfqEps);
            ltab[e] = lg + pbar / (pbar + kLfqEps);
            term -= pbar * lg;
        } else {
            sums[e - p.tab] = s;
        }
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int off = kLfqFinish / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float commit = sums[0] / (n_rows * (float)p.d), h_sample = sums[1] / n_rows, h_batch = red[0];
        out[0] = beta * commit + ratio * (h_sample - gamma * h_batch);
        out[1] = commit;
        out[2] = h_sample;
        out[3] = h_batch;
    }
}

// token -> q by bit arithmetic on the index (no table: any int64 yields a valid sign vector)
__global__ __launch_bounds__(kProjThreads) void lfq_decode_kernel(const int64_t* __restrict__ idx, const float* __restrict__ w_out,
                                                                   const float* __restrict__ b_out, int64_t n, int dm, int d,
                                                                   float* __restrict__ q, bf16_raw* __restrict__ q_lo) {
    extern __shared__ __attribute__((aligned(16))) float lfq_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* woT = lfq_smem;
    proj_stage_weights(nullptr, w_out, dm, d, 0, dm, nullptr, woT);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    for (int64_t row = (int64_t)blockIdx.x * kProjWaves + wave; row < n; row += stride) {
        const unsigned token = (unsigned)idx[row];
#pragma unroll
        for (int c = 0; c < kLfqMaxChunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) {
                float o[4];
                proj_q_chunk<kLfqMaxBits>(woT, dm, d, LfqCode{token}, b_out, ch, o);
                proj_store_q(q, q_lo, row * dm + ch, o);
            }
        }
    }
}

struct LfqLossP {
    float c_commit, c_hs, c_hb;      // 2 beta / (N d),  w a^2 / N,  w gamma a / N: the loss gradient at u without the cotangent
};

// Backward.  grid = (blocks over rows, 256-channel slices), see proj_quant.h.  The gradient at u is straight-through from dq (g = W_out^T dq,
// no tanh) plus s * dloss/du, s = *gscale_dev:
//   dloss/du_nj = c_commit (u - c) - c_hs u p (1 - p) + c_hb sum_m L(m) P_n(m) (bit_j(m) - p_nj)   (m over the codes of j's group)
// The group sum is walked as in the forward: S = sum_m L P and S_j = sum_{m: bit_j(m)} L P per bit, then S_j - p_j S.
template <typename Td>
__global__ __launch_bounds__(kProjThreads) void lfq_backward_kernel(const float* __restrict__ z, const float* __restrict__ u,
                                                                     const Td* __restrict__ dq, const float* __restrict__ w_in,
                                                                     const float* __restrict__ w_out, const float* __restrict__ ltab,
                                                                     const float* __restrict__ gscale_dev, int64_t n, int dm, LfqP p,
                                                                     LfqLossP lp, float* __restrict__ dz, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float lfq_smem[];
    const int d = p.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.y * kProjSlice;
    const int cn = dm - c0 < kProjSlice ? dm - c0 : kProjSlice;
    float* woT = lfq_smem;                       // [d][dm]
    float* wi = woT + d * dm;                    // [d][cn]
    float* lt = wi + d * kProjSlice;             // [p.tab]
    float* red = lt + p.tab;                     // [kLfqRed][64]
    proj_stage_weights(w_in, w_out, dm, d, c0, cn, wi, woT);
    for (int i = threadIdx.x; i < p.tab; i += kProjThreads) lt[i] = ltab[i];
    __syncthreads();
    const float gs_loss = gscale_dev ? *gscale_dev : 1.f;
    const int own = lane * 4;                    // channel inside the slice
    const bool has = own < cn;
    const int nchunks = (dm + 255) / 256;
    float a_wi[kLfqMaxBits][4], a_wo[kLfqMaxBits][4], a_bo[4], a_bi = 0.f;      // a_bi: lane j holds channel j
#pragma unroll
    for (int j = 0; j < kLfqMaxBits; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { a_wi[j][i] = 0.f; a_wo[j][i] = 0.f; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) a_bo[i] = 0.f;

    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    for (int64_t row = (int64_t)blockIdx.x * kProjWaves + wave; row < n; row += stride) {
        float g[kLfqMaxBits], dqo[4] = {0.f, 0.f, 0.f, 0.f}, zo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kLfqMaxBits; ++j) g[j] = 0.f;
        const float mine = lane < d ? u[row * d + lane] : 0.f;
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
        // the loss gradient of channel `lane`, on lane `lane`
        float pj, pmj, hj;
        lfq_sigmoid(p.a * mine, pj, pmj, hj);
        float hb = 0.f;                          // sum_m L(m) P(m) (bit_j(m) - p_j) over the group of channel `lane`
        for (int s = 0; s < p.groups; ++s) {
            const int base = s * p.g, gs = d - base < p.g ? d - base : p.g;
            float ph[4], pmh[4];
            const float low = lfq_group_low(pj, pmj, base, gs, lane, ph, pmh);
            const int nt = gs > 6 ? 1 << (gs - 6) : 1;
            float all = 0.f, hi[4] = {0.f, 0.f, 0.f, 0.f};
            if (lane < (1 << (gs < 6 ? gs : 6)))
                for (int t = 0; t < nt; ++t) {
                    const float lpm = lt[s * p.pitch + t * 64 + lane] * (low * lfq_group_high(ph, pmh, gs, t));
                    all += lpm;
#pragma unroll
                    for (int i = 0; i < 4; ++i) hi[i] += ((t >> i) & 1) ? lpm : 0.f;
                }
            const float total = wave_sum(all);
            for (int i = 0; i < gs; ++i) {
                const float part = i < 6 ? (((lane >> i) & 1) ? all : 0.f) : (i == 6 ? hi[0] : i == 7 ? hi[1] : i == 8 ? hi[2] : hi[3]);
                const float set = wave_sum(part);
                if (lane == base + i) hb = set - pj * total;
            }
        }
        const float cj_mine = mine > 0.f ? 1.f : -1.f;
        const float lgrad = gs_loss * (lp.c_commit * (mine - cj_mine) - lp.c_hs * mine * (pj * pmj) + lp.c_hb * hb);
        float dzo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kLfqMaxBits; ++j)
            if (j < d) {
                const float du = wave_sum(g[j]) + __shfl(lgrad, j, 64);
                const float cj = __shfl(cj_mine, j, 64);
                if (lane == j) a_bi += du;
                if (has) proj_accumulate(wi + j * cn + own, du, cj, zo, dqo, dzo, a_wi[j], a_wo[j]);
            }
        if (has) proj_finish_row(dz + row * dm + c0 + own, dzo, dqo, a_bo);
    }

    // the block's waves, added to wave 0 in wave order; two passes through one buffer: (dW_in, db_out), then (dW_out, db_in)
    for (int pass = 0; pass < 2; ++pass)
        for (int w = 1; w < kProjWaves; ++w) {
            __syncthreads();
            if (wave == w) {
#pragma unroll
                for (int j = 0; j < kLfqMaxBits; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) red[(j * 4 + i) * 64 + lane] = pass == 0 ? a_wi[j][i] : a_wo[j][i];
#pragma unroll
                for (int i = 0; i < 4; ++i) red[(kLfqMaxBits * 4 + i) * 64 + lane] = pass == 0 ? a_bo[i] : a_bi;
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int j = 0; j < kLfqMaxBits; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = red[(j * 4 + i) * 64 + lane];
                        if (pass == 0) a_wi[j][i] += v; else a_wo[j][i] += v;
                    }
                if (pass == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) a_bo[i] += red[(kLfqMaxBits * 4 + i) * 64 + lane];
                } else {
                    a_bi += red[kLfqMaxBits * 4 * 64 + lane];
                }
            }
        }
    if (wave != 0) return;
    float* s_bi = proj_store_slab(ws, dm, d, c0 + own, has, a_wi, a_wo, a_bo);
    if (blockIdx.y == 0 && lane < d) s_bi[lane] = a_bi;
}

// (D, bits, group bits, tau) -> launch arguments; VQK_ERR_SHAPE for what the kernels do not serve
int lfq_params(int dm, int d, int g, float tau, LfqP& p) {
    VQK_REQUIRE(dm >= 4 && dm <= kLfqMaxD && (dm % 4) == 0 && d >= 1 && d <= kLfqMaxBits && g >= 1 && g <= kLfqMaxGroup, VQK_ERR_SHAPE);
    VQK_REQUIRE(tau > 0.f, VQK_ERR_ARG);
    p.d = d;
    p.g = g;
    p.groups = (d + g - 1) / g;
    p.pitch = 1 << g;
    p.tab = p.groups << g;
    p.a = 4.f / tau;
    return VQK_OK;
}

// a function of n only: the same sums every run
int lfq_blocks(int64_t n) { return vqk_grid_1d(n, 4 * kProjWaves, 256); }

}  // namespace

extern "C" {

int64_t vqk_lfq_ws_bytes(int64_t n, int dm, int d, int g) {
    LfqP p;
    if (n < 0) return VQK_ERR_SHAPE;
    if (const int st = lfq_params(dm, d, g, 1.f, p)) return st;
    const int64_t fwd = lfq_fwd_slab_floats(p.tab), bwd = proj_slab_floats(dm, d);
    return (int64_t)lfq_blocks(n) * (fwd > bwd ? fwd : bwd) * (int64_t)sizeof(float);
}

int vqk_lfq_forward(const float* z, const float* w_in, const float* b_in, const float* w_out, const float* b_out, int64_t n, int dm,
                    int d, int g, float tau, float beta, float ratio, float gamma, int64_t* idx, float* u, float* q, void* q_lo,
                    int32_t* hist, float* out, float* ltab, void* ws, int64_t ws_bytes, void* stream) {
    LfqP p;
    if (const int st = lfq_params(dm, d, g, tau, p)) return st;
    VQK_REQUIRE(n >= 0 && ws_bytes >= 0 && z && w_in && b_in && idx, VQK_ERR_ARG);
    VQK_REQUIRE(!(q || q_lo) || (w_out && b_out), VQK_ERR_ARG);
    VQK_REQUIRE((out != nullptr) == (ltab != nullptr) && (out != nullptr) == (ws != nullptr), VQK_ERR_ARG);     // the loss: all three or none
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(q) && vqk_aligned16(q_lo) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(!ws || ws_bytes >= vqk_lfq_ws_bytes(n, dm, d, g), VQK_ERR_WORKSPACE);
    const int blocks = n > 0 ? lfq_blocks(n) : 0;
    hipStream_t st = vqk_stream(stream);
    if (n > 0) {
        static const hipError_t attr = hipFuncSetAttribute((const void*)lfq_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                           kLfqFwdLds);
        if (attr != hipSuccess) return VQK_ERR_LAUNCH;
        const size_t lds = ((size_t)((q || q_lo) ? 2 : 1) * d * dm + (ws ? (size_t)kProjWaves * p.tab + 2 * kProjWaves : 0)) * sizeof(float);
        hipLaunchKernelGGL(lfq_forward_kernel, dim3((unsigned)blocks), dim3(kProjThreads), lds, st, z, w_in, b_in, w_out, b_out, n, dm, p,
                           idx, u, q, reinterpret_cast<bf16_raw*>(q_lo), hist, reinterpret_cast<float*>(ws));
        VQK_CHECK_LAUNCH();
    }
    if (out) {
        hipLaunchKernelGGL(lfq_finish_kernel, dim3(1), dim3(kLfqFinish), 0, st, reinterpret_cast<const float*>(ws), blocks, p,
                           (float)(n > 0 ? n : 1), beta, ratio, gamma, out, ltab);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

int vqk_lfq_decode(const int64_t* idx, const float* w_out, const float* b_out, int64_t n, int dm, int d, float* q, void* q_lo,
                   void* stream) {
    LfqP p;
    if (const int st = lfq_params(dm, d, 1, 1.f, p)) return st;
    VQK_REQUIRE(n >= 0 && idx && w_out && b_out && (q || q_lo), VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(q) && vqk_aligned16(q_lo), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    hipLaunchKernelGGL(lfq_decode_kernel, dim3((unsigned)lfq_blocks(n)), dim3(kProjThreads), (size_t)d * dm * sizeof(float),
                       vqk_stream(stream), idx, w_out, b_out, n, dm, d, q, reinterpret_cast<bf16_raw*>(q_lo));
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_lfq_backward(const float* z, const float* u, const void* dq, int dq_dtype, const float* w_in, const float* w_out,
                     const float* ltab, const float* gscale_dev, int64_t n, int dm, int d, int g, float tau, float beta, float ratio,
                     float gamma, float* dz, float* dw_in, float* db_in, float* dw_out, float* db_out, int accumulate, void* ws,
                     int64_t ws_bytes, void* stream) {
    LfqP p;
    if (const int st = lfq_params(dm, d, g, tau, p)) return st;
    VQK_REQUIRE(n >= 0 && ws_bytes >= 0 && z && u && dq && w_in && w_out && ltab && dz && dw_in && db_in && dw_out && db_out && ws,
                VQK_ERR_ARG);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(dq) && vqk_aligned16(dz) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqk_lfq_ws_bytes(n, dm, d, g), VQK_ERR_WORKSPACE);
    const int blocks = n > 0 ? lfq_blocks(n) : 0;
    hipStream_t st = vqk_stream(stream);
    if (n > 0) {
        const double nn = (double)n;
        const LfqLossP lp = {(float)(2.0 * beta / (nn * d)), (float)((double)ratio * p.a * p.a / nn),
                             (float)((double)ratio * gamma * p.a / nn)};
        const dim3 grid((unsigned)blocks, (unsigned)((dm + kProjSlice - 1) / kProjSlice));
        const size_t lds = ((size_t)d * dm + (size_t)d * kProjSlice + (size_t)p.tab + (size_t)kLfqRed * 64) * sizeof(float);
        float* wsf = reinterpret_cast<float*>(ws);
        if (dq_dtype == VQK_F32) {
            static const hipError_t attr = hipFuncSetAttribute((const void*)lfq_backward_kernel<float>,
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, kLfqBwdLds);
            if (attr != hipSuccess) return VQK_ERR_LAUNCH;
            hipLaunchKernelGGL(lfq_backward_kernel<float>, grid, dim3(kProjThreads), lds, st, z, u, (const float*)dq, w_in, w_out, ltab,
                               gscale_dev, n, dm, p, lp, dz, wsf);
        } else {
            static const hipError_t attr = hipFuncSetAttribute((const void*)lfq_backward_kernel<bf16_raw>,
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, kLfqBwdLds);
            if (attr != hipSuccess) return VQK_ERR_LAUNCH;
            hipLaunchKernelGGL(lfq_backward_kernel<bf16_raw>, grid, dim3(kProjThreads), lds, st, z, u, (const bf16_raw*)dq, w_in, w_out,
                               ltab, gscale_dev, n, dm, p, lp, dz, wsf);
        }
        VQK_CHECK_LAUNCH();
    }
    return proj_launch_slab_sum(ws, blocks, dm, d, accumulate, dw_in, db_in, dw_out, db_out, st);
}

}  // extern "C"
