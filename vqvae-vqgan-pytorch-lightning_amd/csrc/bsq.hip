// Binary spherical quantizer (Zhao, Xiong, Kraehenbuehl 2024, BSQ-ViT): v = W_in z + b_in, u = v / max(|v|, 1e-12) on the unit sphere,
// c_j = +s iff v_j > 0 else -s with s = 1 / sqrt(d), token = the bit pattern of (v_j > 0) (first channel = bit 0), q = W_out c + b_out,
// loss = beta commit + w (H_sample - gamma H_batch): commit = sum |u - c|^2 / N (< 2 whatever d is), p_nj = sigmoid(a u_nj), a = 4 s / tau
// -- the softmax over the 2^d corners factorises as in lfq.hip, and so do the group tables of the batch-average distribution.
//
// The kernels work a WAVE PER ROW on the core of proj_quant.h (up to 18 channels, 2 chunks per lane: D <= 512).  The d projections of a
// row go through the TRANSPOSING reduction of proj_quant.h: 32 exchanges leave channel j's sum on the lanes 2 j and 2 j + 1, where the
// per-channel work (normalisation, sigmoid, entropy, commitment, the gradient through the sphere) runs -- on the even lane of the pair,
// the "owner".  |v|^2 and u.e are one wave sum over the owners, the token is one ballot.  What is per group CODE runs on the lane whose
// id equals the code's low 6 bits, as in lfq.hip.  Every sum over rows is ordered: registers / wave-private LDS tables over the rows of
// a wave (fixed by the grid), the block's waves in wave order, one slab per block in the workspace, a second launch that adds the slabs
// in an order fixed by their count.  No fp32 atomics.
#include "common.h"
#include "proj_quant.h"

#include <cmath>

namespace {

constexpr int kBsqMaxBits = 18;      // projection channels
constexpr int kBsqMaxGroup = 10;     // bits per entropy group: tables of at most 1024 entries
constexpr int kBsqMaxChunks = 2;     // 16-byte chunks per lane: D <= 2 * 64 * 4 = 512
constexpr int kBsqMaxD = 4 * 64 * kBsqMaxChunks;
constexpr int kBsqRed = kBsqMaxBits * 4 + 4;      // floats per lane of one block-reduction pass: 72 + (db_out 4 | db_in 1)
constexpr int kBsqFinish = 1024;     // threads of the forward's finish launch
constexpr float kBsqEps = 1e-10f;    // the epsilon of the batch entropy
constexpr float kBsqNormEps = 1e-12f;

struct BsqP {
    int d, g, groups, pitch, tab;    // bits, bits per group, ceil(d / g), 1 << g, groups << g (floats of the group tables)
    float a, s;                      // 4 s / tau: logit of bit j = a u_j;  s = 1 / sqrt(d): |c_j|
};

constexpr int kBsqMaxTab = 2 << kBsqMaxGroup;     // the largest table over the served (d, g): d = 18, g = 10 -> 2 groups of 1024
constexpr int kBsqFwdLds = (2 * kBsqMaxBits * kBsqMaxD + kProjWaves * kBsqMaxTab + 2 * kProjWaves) * 4;
constexpr int kBsqBwdLds = (kBsqMaxBits * kBsqMaxD + kBsqMaxBits * kProjSlice + kBsqMaxTab + kBsqRed * 64) * 4;

// channel j's code out of the token: bit j set: c_j = +s, else -s
struct BsqCode {
    unsigned token;
    float s;
    __device__ __forceinline__ float operator()(int j) const { return ((token >> j) & 1u) ? s : -s; }
};

// one channel: p = sigmoid(x), pm = sigmoid(-x) (computed as such, never 1 - p), h = the binary entropy in the stable form
// log1p(exp(-|x|)) + |x| sigmoid(-|x|)
__device__ __forceinline__ void bsq_sigmoid(float x, float& p, float& pm, float& h) {
    const float ax = fabsf(x), e = expf(-ax), den = 1.f + e;
    const float small = e / den, big = 1.f / den;
    p = x >= 0.f ? big : small;
    pm = x >= 0.f ? small : big;
    h = log1pf(e) + ax * small;
}

// The codes of group s a lane owns are m = lane + 64 t: the product over the low (<= 6) bits depends on the lane, the product over the
// high bits on t alone.  p / pm hold channel j on the lanes of proj_transpose_sum's map.  Returns the low product (0 on a lane past the
// group's codes) and the high bits' probabilities, wave-uniform.
__device__ __forceinline__ float bsq_group_low(float p, float pm, int base, int gs, int lane, float (&ph)[4], float (&pmh)[4]) {
    const int low = gs < 6 ? gs : 6;
    float prod = lane < (1 << low) ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (i < low) {
            const float pi = __shfl(p, 2 * (base + i), 64), pmi = __shfl(pm, 2 * (base + i), 64);
            prod *= ((lane >> i) & 1) ? pi : pmi;
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = 6 + i < gs ? base + 6 + i : 0;
        ph[i] = __shfl(p, 2 * j, 64);
        pmh[i] = __shfl(pm, 2 * j, 64);
    }
    return prod;
}

__device__ __forceinline__ float bsq_group_high(const float (&ph)[4], const float (&pmh)[4], int gs, int t) {
    float prod = 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (6 + i < gs) prod *= ((t >> i) & 1) ? ph[i] : pmh[i];
    return prod;
}

// slab of one forward block (floats): [group tables p.tab][commit sum][sum_j h], padded to a multiple of 4
__host__ __device__ inline int64_t bsq_fwd_slab_floats(int tab) { return ((int64_t)tab + 2 + 3) & ~(int64_t)3; }

// Forward.  ws == nullptr: assignment only (no loss, no tables).
__global__ __launch_bounds__(kProjThreads) void bsq_forward_kernel(const float* __restrict__ z, const float* __restrict__ w_in,
                                                                    const float* __restrict__ b_in, const float* __restrict__ w_out,
                                                                    const float* __restrict__ b_out, int64_t n, int dm, BsqP p,
                                                                    int64_t* __restrict__ idx, float* __restrict__ u_out,
                                                                    float* __restrict__ r_out, float* __restrict__ q,
                                                                    bf16_raw* __restrict__ q_lo, int32_t* __restrict__ hist,
                                                                    float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float bsq_smem[];
    const int d = p.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mych = proj_tr_channel(lane);
    const bool own = mych < d, owner = own && !(lane & 1);      // the pair's lanes hold channel mych; the even one accounts for it
    const bool want_q = q || q_lo;
    float* wi = bsq_smem;                                        // [d][dm]
    float* woT = wi + d * dm;                                    // [d][dm] when q is wanted
    float* tabs = woT + (want_q ? d * dm : 0);                   // [waves][p.tab] when the loss is wanted
    float* red = tabs + (ws ? kProjWaves * p.tab : 0);           // [waves][2]
    proj_stage_weights(w_in, w_out, dm, d, 0, dm, wi, want_q ? woT : nullptr);
    if (ws)
        for (int i = threadIdx.x; i < kProjWaves * p.tab; i += kProjThreads) tabs[i] = 0.f;
    __syncthreads();
    float* tab = tabs + wave * p.tab;                            // this wave's own tables: no other wave touches them before the end
    float a_commit = 0.f, a_h = 0.f;                             // owner of channel j: channel j over the rows of this wave
    const float bias = own ? b_in[mych] : 0.f;

    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    int64_t row = (int64_t)blockIdx.x * kProjWaves + wave;
    float zc[kBsqMaxChunks][4], zn[kBsqMaxChunks][4];
    if (row < n) proj_load_row(z, row, dm, lane, zc);
    for (; row < n; row += stride) {
        if (row + stride < n) proj_load_row(z, row + stride, dm, lane, zn);      // the next row is in flight under this one
        float vj[kBsqMaxBits];
#pragma unroll
        for (int j = 0; j < kBsqMaxBits; ++j) vj[j] = 0.f;
#pragma unroll
        for (int c = 0; c < kBsqMaxChunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) proj_dot_chunk<kBsqMaxBits>(wi, dm, d, ch, zc[c], vj);
        }
        const float v = proj_transpose_sum<kBsqMaxBits>(vj, lane) + bias;         // channel mych
        const unsigned token = proj_tr_bits(__ballot(owner && v > 0.f));          // a zero or a NaN: bit clear, c = -s
        const float n2 = wave_sum(owner ? v * v : 0.f);
        const float r = 1.f / fmaxf(sqrtf(n2), kBsqNormEps);
        const float u = v * r;
        if (lane == 0) {
            idx[row] = (int64_t)token;
            if (hist) atomicAdd(hist + token, 1);
            if (r_out) r_out[row] = r;
        }
        if (u_out && owner) u_out[row * d + mych] = u;
        if (want_q) {
#pragma unroll
            for (int c = 0; c < kBsqMaxChunks; ++c) {
                const int ch = (c * 64 + lane) * 4;
                if (ch < dm) {
                    float o[4];
                    proj_q_chunk<kBsqMaxBits>(woT, dm, d, BsqCode{token, p.s}, b_out, ch, o);
                    proj_store_q(q, q_lo, row * dm + ch, o);
                }
            }
        }
        if (ws) {
            float pj, pmj, hj;
            bsq_sigmoid(p.a * u, pj, pmj, hj);
            if (owner) {
                const float diff = u - (v > 0.f ? p.s : -p.s);
                a_commit = fmaf(diff, diff, a_commit);
                a_h += hj;
            }
            for (int s = 0; s < p.groups; ++s) {
                const int base = s * p.g, gs = d - base < p.g ? d - base : p.g;
                float ph[4], pmh[4];
                const float low = bsq_group_low(pj, pmj, base, gs, lane, ph, pmh);
                const int nt = gs > 6 ? 1 << (gs - 6) : 1;
                if (lane < (1 << (gs < 6 ? gs : 6)))
                    for (int t = 0; t < nt; ++t) tab[s * p.pitch + t * 64 + lane] += low * bsq_group_high(ph, pmh, gs, t);
            }
        }
#pragma unroll
        for (int c = 0; c < kBsqMaxChunks; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) zc[c][i] = zn[c][i];
    }
    if (!ws) return;
    // the block's waves in wave order, one slab per block: plain stores, every element written
    const float c_sum = wave_sum(a_commit), h_sum = wave_sum(a_h);
    if (lane == 0) { red[wave * 2] = c_sum; red[wave * 2 + 1] = h_sum; }
    __syncthreads();
    float* slab = ws + (int64_t)blockIdx.x * bsq_fwd_slab_floats(p.tab);
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
__device__ __forceinline__ float bsq_slab_column(const float* src, int slabs, int64_t pitch) {
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
// -sum Pbar log(Pbar + eps) (a fixed tree over the threads), out = [loss, commit, H_sample, H_batch]; commit is a sum over channels and
// a mean over rows.  An entry of a ragged last group's table past its 2^g_s codes holds 0 and adds -0 log(eps) = 0.
__global__ __launch_bounds__(kBsqFinish) void bsq_finish_kernel(const float* __restrict__ ws, int slabs, BsqP p, float n_rows, float beta,
                                                                  float ratio, float gamma, float* __restrict__ out,
                                                                  float* __restrict__ ltab) {
    __shared__ float red[kBsqFinish];
    __shared__ float sums[2];
    const int64_t pitch = bsq_fwd_slab_floats(p.tab);
    float term = 0.f;
    for (int e = threadIdx.x; e < p.tab + 2; e += kBsqFinish) {
        const float s = bsq_slab_column(ws + e, slabs, pitch);
        if (e < p.tab) {
            const float pbar = s / n_rows, lg = logf(pbar + kBsqEps);
            ltab[e] = lg + pbar / (pbar + kBsqEps);
            term -= pbar * lg;
        } else {
            sums[e - p.tab] = s;
        }
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int off = kBsqFinish / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float commit = sums[0] / n_rows, h_sample = sums[1] / n_rows, h_batch = red[0];
        out[0] = beta * commit + ratio * (h_sample - gamma * h_batch);
        out[1] = commit;
        out[2] = h_sample;
        out[3] = h_batch;
    }
}

// token -> q by bit arithmetic on the index (no table: any int64 yields a valid corner)
__global__ __launch_bounds__(kProjThreads) void bsq_decode_kernel(const int64_t* __restrict__ idx, const float* __restrict__ w_out,
                                                                   const float* __restrict__ b_out, int64_t n, int dm, int d, float s,
                                                                   float* __restrict__ q, bf16_raw* __restrict__ q_lo) {
    extern __shared__ __attribute__((aligned(16))) float bsq_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* woT = bsq_smem;
    proj_stage_weights(nullptr, w_out, dm, d, 0, dm, nullptr, woT);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    for (int64_t row = (int64_t)blockIdx.x * kProjWaves + wave; row < n; row += stride) {
        const unsigned token = (unsigned)idx[row];
#pragma unroll
        for (int c = 0; c < kBsqMaxChunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) {
                float o[4];
                proj_q_chunk<kBsqMaxBits>(woT, dm, d, BsqCode{token, s}, b_out, ch, o);
                proj_store_q(q, q_lo, row * dm + ch, o);
            }
        }
    }
}

struct BsqLossP {
    float c_commit, c_hs, c_hb;      // 2 beta / N,  w a^2 / N,  w gamma a / N: the loss gradient at u without the cotangent
};

// Backward.  grid = (blocks over rows, 256-channel slices), see proj_quant.h.  The gradient at u is straight-through from dq (g = W_out^T
// dq, through the transposing reduction) plus gl * dloss/du, gl = *gscale_dev:
//   dloss/du_nj = c_commit (u - c) - c_hs u p (1 - p) + c_hb sum_m L(m) P_n(m) (bit_j(m) - p_nj)   (m over the codes of j's group)
// then through the normalisation: dv = (e - u (u.e)) r, u.e one wave sum over the owners.  dv_j sits on channel j's owner and is read
// wave-uniform for dz and the accumulators.
template <typename Td>
__global__ __launch_bounds__(kProjThreads) void bsq_backward_kernel(const float* __restrict__ z, const float* __restrict__ u,
                                                                     const float* __restrict__ rr, const Td* __restrict__ dq,
                                                                     const float* __restrict__ w_in, const float* __restrict__ w_out,
                                                                     const float* __restrict__ ltab, const float* __restrict__ gscale_dev,
                                                                     int64_t n, int dm, BsqP p, BsqLossP lp, float* __restrict__ dz,
                                                                     float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float bsq_smem[];
    const int d = p.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mych = proj_tr_channel(lane);
    const bool own = mych < d, owner = own && !(lane & 1);
    const int c0 = blockIdx.y * kProjSlice;
    const int cn = dm - c0 < kProjSlice ? dm - c0 : kProjSlice;
    float* woT = bsq_smem;                       // [d][dm]
    float* wi = woT + d * dm;                    // [d][cn]
    float* lt = wi + d * kProjSlice;             // [p.tab]
    float* red = lt + p.tab;                     // [kBsqRed][64]
    proj_stage_weights(w_in, w_out, dm, d, c0, cn, wi, woT);
    for (int i = threadIdx.x; i < p.tab; i += kProjThreads) lt[i] = ltab[i];
    __syncthreads();
    const float gs_loss = gscale_dev ? *gscale_dev : 1.f;
    const int ownc = lane * 4;                   // channel inside the slice
    const bool has = ownc < cn;
    const int nchunks = (dm + 255) / 256;
    float a_wi[kBsqMaxBits][4], a_wo[kBsqMaxBits][4], a_bo[4], a_bi = 0.f;      // a_bi: the owner of channel j holds channel j
#pragma unroll
    for (int j = 0; j < kBsqMaxBits; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { a_wi[j][i] = 0.f; a_wo[j][i] = 0.f; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) a_bo[i] = 0.f;

    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    for (int64_t row = (int64_t)blockIdx.x * kProjWaves + wave; row < n; row += stride) {
        float g[kBsqMaxBits], dqo[4] = {0.f, 0.f, 0.f, 0.f}, zo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kBsqMaxBits; ++j) g[j] = 0.f;
        const float mine = own ? u[row * d + mych] : 0.f;
        const float r = rr[row];
        if (has) Vec16<float>::load(z + row * dm + c0 + ownc, zo);
        for (int c = 0; c < nchunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) {
                float v[4];
                proj_load4<Td>(dq + row * dm + ch, v);
                if (c == (int)blockIdx.y) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) dqo[i] = v[i];
                }
                proj_dot_chunk<kBsqMaxBits>(woT, dm, d, ch, v, g);
            }
        }
        const float gj = proj_transpose_sum<kBsqMaxBits>(g, lane);               // channel mych of W_out^T dq
        // the loss gradient of channel mych
        float pj, pmj, hj;
        bsq_sigmoid(p.a * mine, pj, pmj, hj);
        const unsigned token = proj_tr_bits(__ballot(owner && mine > 0.f));
        float hb = 0.f;                          // sum_m L(m) P(m) (bit_j(m) - p_j) over the group of channel mych
        for (int s = 0; s < p.groups; ++s) {
            const int base = s * p.g, gs = d - base < p.g ? d - base : p.g;
            // sum_m P(m) (bit_j(m) - p_j) = 0, so L may be shifted by a constant: by L at the row's own code of this group, the code
            // that carries most of P.  A near-uniform Pbar (L almost constant) then leaves small terms instead of the difference of
            // large ones, and a saturated row has its one large term exactly zero.
            const float l0 = lt[s * p.pitch + (int)((token >> base) & ((1u << gs) - 1u))];
            float ph[4], pmh[4];
            const float low = bsq_group_low(pj, pmj, base, gs, lane, ph, pmh);
            const int nt = gs > 6 ? 1 << (gs - 6) : 1;
            float all = 0.f, hi[4] = {0.f, 0.f, 0.f, 0.f};
            if (lane < (1 << (gs < 6 ? gs : 6)))
                for (int t = 0; t < nt; ++t) {
                    const float lpm = (lt[s * p.pitch + t * 64 + lane] - l0) * (low * bsq_group_high(ph, pmh, gs, t));
                    all += lpm;
#pragma unroll
                    for (int i = 0; i < 4; ++i) hi[i] += ((t >> i) & 1) ? lpm : 0.f;
                }
            const float total = wave_sum(all);
            for (int i = 0; i < gs; ++i) {
                const float part = i < 6 ? (((lane >> i) & 1) ? all : 0.f) : (i == 6 ? hi[0] : i == 7 ? hi[1] : i == 8 ? hi[2] : hi[3]);
                const float set = wave_sum(part);
                if (mych == base + i) hb = set - pj * total;
            }
        }
        const float cj_mine = mine > 0.f ? p.s : -p.s;
        const float lgrad = gs_loss * (lp.c_commit * (mine - cj_mine) - lp.c_hs * mine * (pj * pmj) + lp.c_hb * hb);
        const float e = own ? gj + lgrad : 0.f;
        const float ue = wave_sum(owner ? mine * e : 0.f);
        const float dv = (e - mine * ue) * r;
        if (owner) a_bi += dv;
        const BsqCode code{token, p.s};
        float dzo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kBsqMaxBits; ++j)
            if (j < d) {
                const float du = proj_tr_read(dv, j);
                if (has) proj_accumulate(wi + j * cn + ownc, du, code(j), zo, dqo, dzo, a_wi[j], a_wo[j]);
            }
        if (has) proj_finish_row(dz + row * dm + c0 + ownc, dzo, dqo, a_bo);
    }

    // the block's waves, added to wave 0 in wave order; two passes through one buffer: (dW_in, db_out), then (dW_out, db_in)
    for (int pass = 0; pass < 2; ++pass)
        for (int w = 1; w < kProjWaves; ++w) {
            __syncthreads();
            if (wave == w) {
#pragma unroll
                for (int j = 0; j < kBsqMaxBits; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) red[(j * 4 + i) * 64 + lane] = pass == 0 ? a_wi[j][i] : a_wo[j][i];
#pragma unroll
                for (int i = 0; i < 4; ++i) red[(kBsqMaxBits * 4 + i) * 64 + lane] = pass == 0 ? a_bo[i] : a_bi;
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int j = 0; j < kBsqMaxBits; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = red[(j * 4 + i) * 64 + lane];
                        if (pass == 0) a_wi[j][i] += v; else a_wo[j][i] += v;
                    }
                if (pass == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) a_bo[i] += red[(kBsqMaxBits * 4 + i) * 64 + lane];
                } else {
                    a_bi += red[kBsqMaxBits * 4 * 64 + lane];
                }
            }
        }
    if (wave != 0) return;
    float* s_bi = proj_store_slab(ws, dm, d, c0 + ownc, has, a_wi, a_wo, a_bo);
    if (blockIdx.y == 0 && owner) s_bi[mych] = a_bi;
}

// (D, bits, group bits, tau) -> launch arguments; VQK_ERR_SHAPE for what the kernels do not serve
int bsq_params(int dm, int d, int g, float tau, BsqP& p) {
    VQK_REQUIRE(dm >= 4 && dm <= kBsqMaxD && (dm % 4) == 0 && d >= 1 && d <= kBsqMaxBits && g >= 1 && g <= kBsqMaxGroup, VQK_ERR_SHAPE);
    VQK_REQUIRE(tau > 0.f, VQK_ERR_ARG);
    p.d = d;
    p.g = g;
    p.groups = (d + g - 1) / g;
    p.pitch = 1 << g;
    p.tab = p.groups << g;
    const double s = 1.0 / std::sqrt((double)d);
    p.s = (float)s;
    p.a = (float)(4.0 * s / (double)tau);
    return VQK_OK;
}

// a function of n only: the same sums every run
int bsq_blocks(int64_t n) { return vqk_grid_1d(n, 4 * kProjWaves, 256); }

}  // namespace

extern "C" {

int64_t vqk_bsq_ws_bytes(int64_t n, int dm, int d, int g) {
    BsqP p;
    if (n < 0) return VQK_ERR_SHAPE;
    if (const int st = bsq_params(dm, d, g, 1.f, p)) return st;
    const int64_t fwd = bsq_fwd_slab_floats(p.tab), bwd = proj_slab_floats(dm, d);
    return (int64_t)bsq_blocks(n) * (fwd > bwd ? fwd : bwd) * (int64_t)sizeof(float);
}

int vqk_bsq_forward(const float* z, const float* w_in, const float* b_in, const float* w_out, const float* b_out, int64_t n, int dm,
                    int d, int g, float tau, float beta, float ratio, float gamma, int64_t* idx, float* u, float* r, float* q, void* q_lo,
                    int32_t* hist, float* out, float* ltab, void* ws, int64_t ws_bytes, void* stream) {
    BsqP p;
    if (const int st = bsq_params(dm, d, g, tau, p)) return st;
    VQK_REQUIRE(n >= 0 && ws_bytes >= 0 && z && w_in && b_in && idx, VQK_ERR_ARG);
    VQK_REQUIRE(!(q || q_lo) || (w_out && b_out), VQK_ERR_ARG);
    VQK_REQUIRE((out != nullptr) == (ltab != nullptr) && (out != nullptr) == (ws != nullptr), VQK_ERR_ARG);     // the loss: all three or none
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(q) && vqk_aligned16(q_lo) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(!ws || ws_bytes >= vqk_bsq_ws_bytes(n, dm, d, g), VQK_ERR_WORKSPACE);
    const int blocks = n > 0 ? bsq_blocks(n) : 0;
    hipStream_t st = vqk_stream(stream);
    if (n > 0) {
        static const hipError_t attr = hipFuncSetAttribute((const void*)bsq_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                           kBsqFwdLds);
        if (attr != hipSuccess) return VQK_ERR_LAUNCH;
        const size_t lds = ((size_t)((q || q_lo) ? 2 : 1) * d * dm + (ws ? (size_t)kProjWaves * p.tab + 2 * kProjWaves : 0)) * sizeof(float);
        hipLaunchKernelGGL(bsq_forward_kernel, dim3((unsigned)blocks), dim3(kProjThreads), lds, st, z, w_in, b_in, w_out, b_out, n, dm, p,
                           idx, u, r, q, reinterpret_cast<bf16_raw*>(q_lo), hist, reinterpret_cast<float*>(ws));
        VQK_CHECK_LAUNCH();
    }
    if (out) {
        hipLaunchKernelGGL(bsq_finish_kernel, dim3(1), dim3(kBsqFinish), 0, st, reinterpret_cast<const float*>(ws), blocks, p,
                           (float)(n > 0 ? n : 1), beta, ratio, gamma, out, ltab);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

int vqk_bsq_decode(const int64_t* idx, const float* w_out, const float* b_out, int64_t n, int dm, int d, float* q, void* q_lo,
                   void* stream) {
    BsqP p;
    if (const int st = bsq_params(dm, d, 1, 1.f, p)) return st;
    VQK_REQUIRE(n >= 0 && idx && w_out && b_out && (q || q_lo), VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(q) && vqk_aligned16(q_lo), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    hipLaunchKernelGGL(bsq_decode_kernel, dim3((unsigned)bsq_blocks(n)), dim3(kProjThreads), (size_t)d * dm * sizeof(float),
                       vqk_stream(stream), idx, w_out, b_out, n, dm, d, p.s, q, reinterpret_cast<bf16_raw*>(q_lo));
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_bsq_backward(const float* z, const float* u, const float* r, const void* dq, int dq_dtype, const float* w_in, const float* w_out,
                     const float* ltab, const float* gscale_dev, int64_t n, int dm, int d, int g, float tau, float beta, float ratio,
                     float gamma, float* dz, float* dw_in, float* db_in, float* dw_out, float* db_out, int accumulate, void* ws,
                     int64_t ws_bytes, void* stream) {
    BsqP p;
    if (const int st = bsq_params(dm, d, g, tau, p)) return st;
    VQK_REQUIRE(n >= 0 && ws_bytes >= 0 && z && u && r && dq && w_in && w_out && ltab && dz && dw_in && db_in && dw_out && db_out && ws,
                VQK_ERR_ARG);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(dq) && vqk_aligned16(dz) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqk_bsq_ws_bytes(n, dm, d, g), VQK_ERR_WORKSPACE);
    const int blocks = n > 0 ? bsq_blocks(n) : 0;
    hipStream_t st = vqk_stream(stream);
    if (n > 0) {
        const double nn = (double)n, a = 4.0 / (std::sqrt((double)d) * (double)tau);
        const BsqLossP lp = {(float)(2.0 * beta / nn), (float)((double)ratio * a * a / nn), (float)((double)ratio * gamma * a / nn)};
        const dim3 grid((unsigned)blocks, (unsigned)((dm + kProjSlice - 1) / kProjSlice));
        const size_t lds = ((size_t)d * dm + (size_t)d * kProjSlice + (size_t)p.tab + (size_t)kBsqRed * 64) * sizeof(float);
        float* wsf = reinterpret_cast<float*>(ws);
        if (dq_dtype == VQK_F32) {
            static const hipError_t attr = hipFuncSetAttribute((const void*)bsq_backward_kernel<float>,
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, kBsqBwdLds);
            if (attr != hipSuccess) return VQK_ERR_LAUNCH;
            hipLaunchKernelGGL(bsq_backward_kernel<float>, grid, dim3(kProjThreads), lds, st, z, u, r, (const float*)dq, w_in, w_out, ltab,
                               gscale_dev, n, dm, p, lp, dz, wsf);
        } else {
            static const hipError_t attr = hipFuncSetAttribute((const void*)bsq_backward_kernel<bf16_raw>,
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, kBsqBwdLds);
            if (attr != hipSuccess) return VQK_ERR_LAUNCH;
            hipLaunchKernelGGL(bsq_backward_kernel<bf16_raw>, grid, dim3(kProjThreads), lds, st, z, u, r, (const bf16_raw*)dq, w_in, w_out,
                               ltab, gscale_dev, n, dm, p, lp, dz, wsf);
        }
        VQK_CHECK_LAUNCH();
    }
    return proj_launch_slab_sum(ws, blocks, dm, d, accumulate, dw_in, db_in, dw_out, db_out, st);
}

}  // extern "C"
