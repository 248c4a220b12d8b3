// Index-backpropagation quantizer (IBQ; include/vqk.h: vqk_ibq_forward_f32 / vqk_ibq_backward_f32).
//
// The token of a latent row z_i is the argmax of the logits S_ij = (z_i . e_j) / T over the codebook e[K][D]; the one-hot that gathers
// the code is made differentiable with a straight-through estimator on P = softmax_j(S), so a step sends gradient to EVERY code and
// the encoder is trained through the logits.  The soft part is attention with Q = the latent rows and K = V = the codebook, and the
// kernels are the fp32 forms of csrc/attn.hip (on the same tile helpers, mfma_tile.h) with a query count that differs from the key
// count and an argmax carried beside the running maximum.  One workgroup = 4 waves = one 64-row tile:
//   forward : owns 64 latent rows, walks the codes in tiles of 64 (online softmax; m, l, lse, the argmax in fp32 / int32), then
//             gathers q = e[idx], sums |q - z|^2 of its rows and counts the tokens
//   rows    : G = g + s c2 (q - z), H = G + s beta c2 (q - z), delta = G . ebar, dz = -2 s c2 (q - z): one wave per row
//   dE      : owns 64 codes, walks the rows  (S^T and dP^T with the code on the tile row; dE = old + (1/T) dS^T z + Sel^T H, the 0/1
//             selection matrix Sel^T[code][row] = (idx[row] == code) built in LDS: the hard term is one more exact product)
//   dz      : owns 64 rows, walks the codes  (dz += (1/T) dS e)
// so every element of ebar, lse, dz and dE is summed by ONE workgroup in a fixed order: no float atomics, the same bits on every run
// and in every mode.  The sse sum is ordered as well (per-wave sums in row order, the block's four in wave order into the block's slot
// of ws, one finish block adds the slots in a fixed tree); hist uses int32 atomics.  All products are exact fp32
// (v_mfma_f32_32x32x2_f32), accumulation and statistics fp32; no N x K array is ever in memory.
// Shapes: D in {64, 128, 256}, ANY N >= 1 and ANY K >= 1 (n, k < 2^31): tail rows and tail codes are zeros in LDS, never read from
// or stored to memory; a tail code weighs exactly zero and its logit is -inf, so it can never win the argmax.
// The argmax-only mode (lse == NULL) runs the same logit arithmetic (same tiles, same MFMA order, same scaling) and skips the
// exponentials and the second product: the same tokens, bit for bit.
#include "common.h"
#include "mfma_tile.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int LD = Pitch<float>::LD;     // fp32 tile pitch
constexpr int TB = AT * LD;

static inline bool ibq_d_ok(int d) { return d == 64 || d == 128 || d == 256; }

struct IbqArgs {
    const float *z, *e;
    int64_t* idx_out;
    const int64_t* idx;
    float *lse, *ebar, *q32;
    bf16_raw* qlo;
    int32_t* hist;
    float* part;                 // forward: the blocks' sse slots
    const float *g, *h, *delta;  // backward: the row pass's G, H and delta
    float *dz, *de;
    int n, k;
    float inv_t;
};

constexpr int fwd_lds() { return (5 * TB + 2 * AT + 4) * 4; }     // 4 tiles, logits / P, alpha | 1 / l, the tokens, the waves' sse
constexpr int bwd_lds() { return 6 * TB * 4; }
constexpr int dz_lds() { return 5 * TB * 4; }

// ------------------------------------------------------------------------------------------------
// forward.  grid ceil(n / 64)
// ------------------------------------------------------------------------------------------------
template <int D, bool SOFT>
__global__ __launch_bounds__(256) void ibq_fwd_kernel(const IbqArgs a) {
    constexpr int NC = D / AT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* buf = reinterpret_cast<float*>(smem);                 // 4 operand tiles
    float* sS = buf + 4 * TB;                                    // scaled logits [64][LD], then P over them
    float* sRow = sS + TB;                                       // alpha, finally 1 / l
    int* sIdx = reinterpret_cast<int*>(sRow + AT);
    float* sWave = reinterpret_cast<float*>(sIdx + AT);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rh = wave >> 1, ch = wave & 1;
    const int n = a.n, k = a.k, q0 = blockIdx.x * AT;
    const float* zb = a.z;
    const float* eb = a.e;
    const int srow = tid >> 2, part = tid & 3;                   // softmax: 4 threads per latent row, 16 codes each

    f32x16 oacc[SOFT ? NC : 1];
#pragma unroll
    for (int c = 0; c < (SOFT ? NC : 1); ++c) acc_zero(oacc[c]);
    float m = -INFINITY, l = 0.0f;                               // the same in the 4 threads of a row
    int best = 0;

    TileRegs<float> ra, rb;                                             // the next step's tiles, in flight
    gload(ra, zb, D, q0, n, 0);
    gload(rb, eb, D, 0, k, 0);
    for (int k0 = 0; k0 < k; k0 += AT) {
        f32x16 s;
        acc_zero(s);
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // S = z e^T, chunk c in tile pair c & 1
            float* bq = buf + (2 * (c & 1)) * TB;
            float* bk = bq + TB;
            lstore(bq, ra);
            lstore(bk, rb);
            if (c + 1 < NC) {
                gload(ra, zb, D, q0, n, (c + 1) * AT);
                gload(rb, eb, D, k0, k, (c + 1) * AT);
            } else if (SOFT) {
                gload(ra, eb, D, k0, k, 0);
            } else if (k0 + AT < k) {
                gload(ra, zb, D, q0, n, 0);
                gload(rb, eb, D, k0 + AT, k, 0);
            }
            __syncthreads();
            mma_nt(s, bq + rh * 32 * LD, bk + ch * 32 * LD, lane);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sS[(rh * 32 + acc_row(r, lane)) * LD + ch * 32 + (lane & 31)] = s[r] * a.inv_t;
        __syncthreads();
        {
            float x[16];
            float mx = -INFINITY;
            int mi = INT_MAX;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int code = k0 + part * 16 + j;
                x[j] = (code < k) ? sS[srow * LD + part * 16 + j] : -INFINITY;      // a tail code can never win
                if (x[j] > mx) { mx = x[j]; mi = code; }                            // strict: the first maximum stays
            }
#pragma unroll
            for (int off = 1; off <= 2; off <<= 1) {
                const float ov = __shfl_xor(mx, off, 64);
                const int oi = __shfl_xor(mi, off, 64);
                if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
            }
            if (mx > m) best = mi;                               // strict over ascending tiles: the smallest index wins a tie
            const float mn = fmaxf(m, mx);                       // finite: code k0 is always valid
            if (SOFT) {
                const float alpha = expf(m - mn);
                float sum = 0.0f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const float p = (k0 + part * 16 + j < k) ? expf(x[j] - mn) : 0.0f;      // tail codes: exactly zero weight
                    sum += p;
                    sS[srow * LD + part * 16 + j] = p;
                }
                sum += __shfl_xor(sum, 1, 64);
                sum += __shfl_xor(sum, 2, 64);
                l = l * alpha + sum;
                if (part == 0) sRow[srow] = alpha;
            }
            m = mn;
        }
        if (SOFT) {
            __syncthreads();
            float al[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) al[r] = sRow[rh * 32 + acc_row(r, lane)];
#pragma unroll
            for (int c = 0; c < NC; ++c) {                       // ebar = alpha ebar + P e, chunk c in tile 2 + (c & 1)
                float* bv = buf + (2 + (c & 1)) * TB;
                lstore(bv, ra);
                if (c + 1 < NC) {
                    gload(ra, eb, D, k0, k, (c + 1) * AT);
                } else if (k0 + AT < k) {
                    gload(ra, zb, D, q0, n, 0);
                    gload(rb, eb, D, k0 + AT, k, 0);
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[c][r] *= al[r];
                mma_ab(oacc[c], sS + rh * 32 * LD, bv, ch * 32, lane);
            }
        }
        __syncthreads();                                         // the logits / P, alpha and the tiles are free again
    }
    if (part == 0) {
        sIdx[srow] = best;
        if (SOFT) sRow[srow] = 1.0f / l;
        if (q0 + srow < n) {
            a.idx_out[q0 + srow] = best;
            if (SOFT) a.lse[q0 + srow] = m + logf(l);
        }
    }
    __syncthreads();
    if (SOFT) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rh * 32 + acc_row(r, lane);
            if (q0 + row < n) {
                const float li = sRow[row];
#pragma unroll
                for (int c = 0; c < NC; ++c) a.ebar[(int64_t)(q0 + row) * D + c * AT + ch * 32 + (lane & 31)] = oacc[c][r] * li;
            }
        }
    }
    if (!a.q32 && !a.qlo && !a.part && !a.hist) return;          // (uniform over the grid)
    // the gather q = e[idx], the rows' |q - z|^2 and the token counts: wave w takes rows w, w + 4, ...
    float wsse = 0.0f;
    for (int r = wave; r < AT && q0 + r < n; r += 4) {
        const int64_t row = q0 + r;
        const int code = sIdx[r];
        float acc = 0.0f;
        if (a.q32 || a.qlo || a.part) {
            for (int c = lane * 4; c < D; c += 256) {
                const f32x4 qv = *reinterpret_cast<const f32x4*>(eb + (int64_t)code * D + c);
                if (a.q32) *reinterpret_cast<f32x4*>(a.q32 + row * D + c) = qv;
                if (a.qlo) {
                    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
                    const u32x2 o = {vqk_pack_bf16x2(qv[0], qv[1]), vqk_pack_bf16x2(qv[2], qv[3])};
                    *reinterpret_cast<u32x2*>(a.qlo + row * D + c) = o;
                }
                if (a.part) {
                    const f32x4 zv = *reinterpret_cast<const f32x4*>(zb + row * D + c);
#pragma unroll
                    for (int u = 0; u < 4; ++u) { const float df = qv[u] - zv[u]; acc = __fmaf_rn(df, df, acc); }
                }
            }
        }
        if (a.part) wsse = __fadd_rn(wsse, wave_sum(acc));
        if (a.hist && lane == 0) atomicAdd(a.hist + code, 1);
    }
    if (a.part) {
        if (lane == 0) sWave[wave] = wsse;
        __syncthreads();
        if (tid == 0) a.part[blockIdx.x] = __fadd_rn(__fadd_rn(__fadd_rn(sWave[0], sWave[1]), sWave[2]), sWave[3]);
    }
}

// sse[0] = the blocks' slots in a fixed order: thread t adds slots t, t + 256, ..., then a fixed tree over the threads
__global__ __launch_bounds__(256) void ibq_finish_kernel(const float* __restrict__ part, int blocks, float* __restrict__ sse) {
    __shared__ float sh[256];
    float s = 0.0f;
    for (int b = threadIdx.x; b < blocks; b += 256) s = __fadd_rn(s, part[b]);
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = __fadd_rn(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *sse = sh[0];
}

// ------------------------------------------------------------------------------------------------
// backward, row pass: one wave per row.  grid ceil(n / 4)
// ------------------------------------------------------------------------------------------------
template <typename TDQ> struct IbqDq;
template <> struct IbqDq<float> {
    __device__ static __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
};
template <> struct IbqDq<bf16_raw> {
    __device__ static __forceinline__ f32x4 ld4(const bf16_raw* p) {
        const u16x4 v = *reinterpret_cast<const u16x4*>(p);
        const f32x4 o = {bf16_to_f32(v[0]), bf16_to_f32(v[1]), bf16_to_f32(v[2]), bf16_to_f32(v[3])};
        return o;
    }
};

template <typename TDQ, bool HAS_DQ>
__global__ __launch_bounds__(256) void ibq_rows_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                       const int64_t* __restrict__ idx, const float* __restrict__ ebar,
                                                       const TDQ* __restrict__ dq, int n, int k, int d, float cz, float ce,
                                                       const float* __restrict__ gs, float* __restrict__ g, float* __restrict__ h,
                                                       float* __restrict__ delta, float* __restrict__ dz) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    if (gs) { const float sc = *gs; cz *= sc; ce *= sc; }
    const int64_t code = idx[row];
    const bool ok = code >= 0 && code < k;                       // a token outside [0, K): no hard terms, nothing read from e
    float dot = 0.0f;
    for (int c = lane * 4; c < d; c += 256) {
        const f32x4 zv = *reinterpret_cast<const f32x4*>(z + row * d + c);
        f32x4 df = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(e + code * d + c);
#pragma unroll
            for (int u = 0; u < 4; ++u) df[u] = __fsub_rn(qv[u], zv[u]);
        }
        f32x4 up = {0.f, 0.f, 0.f, 0.f};
        if (HAS_DQ) up = IbqDq<TDQ>::ld4(dq + row * d + c);
        const f32x4 eb = *reinterpret_cast<const f32x4*>(ebar + row * d + c);
        f32x4 gv, hv, dv;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            gv[u] = __fmaf_rn(ce, df[u], up[u]);
            hv[u] = __fmaf_rn(cz, df[u], gv[u]);
            dv[u] = __fmul_rn(-2.0f * ce, df[u]);
            dot = __fmaf_rn(gv[u], eb[u], dot);
        }
        *reinterpret_cast<f32x4*>(g + row * d + c) = gv;
        *reinterpret_cast<f32x4*>(h + row * d + c) = hv;
        *reinterpret_cast<f32x4*>(dz + row * d + c) = dv;
    }
    dot = wave_sum(dot);
    if (lane == 0) delta[row] = dot;
}

// ------------------------------------------------------------------------------------------------
// dE.  grid ceil(k / 64): the workgroup owns 64 codes; tiles are [code][row]
// ------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void ibq_de_kernel(const IbqArgs a) {
    constexpr int NC = D / AT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* buf = reinterpret_cast<float*>(smem);
    float* sSel = buf + 4 * TB;                                  // Sel^T [code][row], 0 / 1
    float* sDT = buf + 5 * TB;                                   // dS^T  [code][row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rh = wave >> 1, ch = wave & 1;
    const int n = a.n, k = a.k, k0 = blockIdx.x * AT;

    f32x16 soft[NC], hard[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { acc_zero(soft[c]); acc_zero(hard[c]); }

    TileRegs<float> ra, rb;
    gload(ra, a.e, D, k0, k, 0);
    gload(rb, a.z, D, 0, n, 0);
    for (int q0 = 0; q0 < n; q0 += AT) {
        f32x16 st, dpt;
        acc_zero(st);
        acc_zero(dpt);
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // S^T = e z^T in tiles 0, 1; dP^T = e G^T in tiles 2, 3
            lstore(buf, ra);
            lstore(buf + TB, rb);
            gload(rb, a.g, D, q0, n, c * AT);                    // (ra keeps the e chunk for tile 2)
            __syncthreads();
            mma_nt(st, buf + rh * 32 * LD, buf + TB + ch * 32 * LD, lane);
            lstore(buf + 2 * TB, ra);
            lstore(buf + 3 * TB, rb);
            if (c + 1 < NC) {
                gload(ra, a.e, D, k0, k, (c + 1) * AT);
                gload(rb, a.z, D, q0, n, (c + 1) * AT);
            } else {
                gload(ra, a.h, D, q0, n, 0);
                gload(rb, a.z, D, q0, n, 0);
            }
            __syncthreads();
            mma_nt(dpt, buf + 2 * TB + rh * 32 * LD, buf + 3 * TB + ch * 32 * LD, lane);
        }
        const int qi = q0 + ch * 32 + (lane & 31);
        const bool qok = qi < n;
        const float ls = qok ? a.lse[qi] : 0.0f, dl = qok ? a.delta[qi] : 0.0f;
        const int64_t tok = qok ? a.idx[qi] : (int64_t)-1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rh * 32 + acc_row(r, lane);
            const bool live = qok && k0 + row < k;
            const float p = live ? expf(st[r] * a.inv_t - ls) : 0.0f;
            sSel[row * LD + ch * 32 + (lane & 31)] = (live && tok == (int64_t)(k0 + row)) ? 1.0f : 0.0f;
            sDT[row * LD + ch * 32 + (lane & 31)] = p * (dpt[r] - dl);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // hard += Sel^T H, soft += dS^T z, chunk c in tile pair c & 1
            float* bg = buf + (2 * (c & 1)) * TB;
            float* bq = bg + TB;
            lstore(bg, ra);
            lstore(bq, rb);
            if (c + 1 < NC) {
                gload(ra, a.h, D, q0, n, (c + 1) * AT);
                gload(rb, a.z, D, q0, n, (c + 1) * AT);
            } else if (q0 + AT < n) {
                gload(ra, a.e, D, k0, k, 0);
                gload(rb, a.z, D, q0 + AT, n, 0);
            }
            __syncthreads();                                     // (chunk 0: Sel^T and dS^T are in LDS as well)
            mma_ab(hard[c], sSel + rh * 32 * LD, bg, ch * 32, lane);
            mma_ab(soft[c], sDT + rh * 32 * LD, bq, ch * 32, lane);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = k0 + rh * 32 + acc_row(r, lane);
        if (row < k) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float* p = a.de + (int64_t)row * D + c * AT + ch * 32 + (lane & 31);
                *p = __fadd_rn(*p, __fmaf_rn(soft[c][r], a.inv_t, hard[c][r]));      // old + sum: the target may hold values
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dz.  grid ceil(n / 64): the workgroup owns 64 rows; tiles are [row][code]
// ------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void ibq_dz_kernel(const IbqArgs a) {
    constexpr int NC = D / AT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* buf = reinterpret_cast<float*>(smem);
    float* sDS = buf + 4 * TB;                                   // dS [row][code]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rh = wave >> 1, ch = wave & 1;
    const int n = a.n, k = a.k, q0 = blockIdx.x * AT;

    float ls[16], dl[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qi = q0 + rh * 32 + acc_row(r, lane);
        ls[r] = qi < n ? a.lse[qi] : 0.0f;
        dl[r] = qi < n ? a.delta[qi] : 0.0f;
    }
    f32x16 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc_zero(acc[c]);

    TileRegs<float> ra, rb;
    gload(ra, a.z, D, q0, n, 0);
    gload(rb, a.e, D, 0, k, 0);
    for (int k0 = 0; k0 < k; k0 += AT) {
        f32x16 s, dp;
        acc_zero(s);
        acc_zero(dp);
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // S = z e^T in tiles 0, 1; dP = G e^T in tiles 2, 3
            lstore(buf, ra);
            lstore(buf + TB, rb);
            gload(ra, a.g, D, q0, n, c * AT);                    // (rb keeps the e chunk for tile 3)
            __syncthreads();
            mma_nt(s, buf + rh * 32 * LD, buf + TB + ch * 32 * LD, lane);
            lstore(buf + 2 * TB, ra);
            lstore(buf + 3 * TB, rb);
            if (c + 1 < NC) {
                gload(ra, a.z, D, q0, n, (c + 1) * AT);
                gload(rb, a.e, D, k0, k, (c + 1) * AT);
            } else {
                gload(ra, a.e, D, k0, k, 0);
            }
            __syncthreads();
            mma_nt(dp, buf + 2 * TB + rh * 32 * LD, buf + 3 * TB + ch * 32 * LD, lane);
        }
        const bool kok = k0 + ch * 32 + (lane & 31) < k;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rh * 32 + acc_row(r, lane);
            const float p = (kok && q0 + row < n) ? expf(s[r] * a.inv_t - ls[r]) : 0.0f;
            sDS[row * LD + ch * 32 + (lane & 31)] = p * (dp[r] - dl[r]);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // acc += dS e, chunk c in tile c & 1
            float* bk = buf + (c & 1) * TB;
            lstore(bk, ra);
            if (c + 1 < NC) {
                gload(ra, a.e, D, k0, k, (c + 1) * AT);
            } else if (k0 + AT < k) {
                gload(ra, a.z, D, q0, n, 0);
                gload(rb, a.e, D, k0 + AT, k, 0);
            }
            __syncthreads();                                     // (chunk 0: dS is in LDS as well)
            mma_ab(acc[c], sDS + rh * 32 * LD, bk, ch * 32, lane);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = q0 + rh * 32 + acc_row(r, lane);
        if (row < n) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float* p = a.dz + (int64_t)row * D + c * AT + ch * 32 + (lane & 31);
                *p = __fmaf_rn(acc[c][r], a.inv_t, *p);          // the row pass left -2 s c2 (q - z) there
            }
        }
    }
}

template <int D, bool SOFT> int launch_fwd(const IbqArgs& a, hipStream_t st) {
    static const hipError_t attr = hipFuncSetAttribute((const void*)ibq_fwd_kernel<D, SOFT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       fwd_lds());
    if (attr != hipSuccess) return VQK_ERR_LAUNCH;
    hipLaunchKernelGGL((ibq_fwd_kernel<D, SOFT>), dim3((unsigned)((a.n + AT - 1) / AT)), dim3(256), fwd_lds(), st, a);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}
template <int D> int launch_bwd(const IbqArgs& a, hipStream_t st) {
    static const hipError_t attr1 = hipFuncSetAttribute((const void*)ibq_de_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, bwd_lds());
    static const hipError_t attr2 = hipFuncSetAttribute((const void*)ibq_dz_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, dz_lds());
    if (attr1 != hipSuccess || attr2 != hipSuccess) return VQK_ERR_LAUNCH;
    if (a.de) hipLaunchKernelGGL((ibq_de_kernel<D>), dim3((unsigned)((a.k + AT - 1) / AT)), dim3(256), bwd_lds(), st, a);
    hipLaunchKernelGGL((ibq_dz_kernel<D>), dim3((unsigned)((a.n + AT - 1) / AT)), dim3(256), dz_lds(), st, a);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // namespace

extern "C" {

int64_t vqk_ibq_forward_ws_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31)) return VQK_ERR_SHAPE;
    return ((n + AT - 1) / AT + 1) * 4;
}

int vqk_ibq_forward_f32(const float* z, const float* e, int64_t n, int k, int d, float inv_t, int64_t* idx, float* lse, float* ebar,
                        float* q32, void* qlo, float* sse, int32_t* hist, void* ws, int64_t ws_bytes, void* stream) {
    VQK_REQUIRE(z && e && idx, VQK_ERR_ARG);
    VQK_REQUIRE((lse == nullptr) == (ebar == nullptr), VQK_ERR_ARG);
    VQK_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && k >= 1 && ibq_d_ok(d), VQK_ERR_SHAPE);
    VQK_REQUIRE(inv_t > 0.0f && inv_t < INFINITY, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(e) && (!ebar || vqk_aligned16(ebar)) && (!q32 || vqk_aligned16(q32)) &&
                    (reinterpret_cast<uintptr_t>(qlo) & 7u) == 0 && (!sse || vqk_aligned16(ws)), VQK_ERR_ALIGN);
    VQK_REQUIRE(!sse || (ws && ws_bytes >= vqk_ibq_forward_ws_bytes(n)), VQK_ERR_WORKSPACE);
    IbqArgs a = {};
    a.z = z; a.e = e; a.idx_out = idx; a.lse = lse; a.ebar = ebar; a.q32 = q32; a.qlo = reinterpret_cast<bf16_raw*>(qlo); a.hist = hist;
    a.part = sse ? reinterpret_cast<float*>(ws) : nullptr;
    a.n = (int)n; a.k = k; a.inv_t = inv_t;
    hipStream_t st = vqk_stream(stream);
    int rc;
    if (lse) rc = d == 64 ? launch_fwd<64, true>(a, st) : d == 128 ? launch_fwd<128, true>(a, st) : launch_fwd<256, true>(a, st);
    else rc = d == 64 ? launch_fwd<64, false>(a, st) : d == 128 ? launch_fwd<128, false>(a, st) : launch_fwd<256, false>(a, st);
    if (rc != VQK_OK) return rc;
    if (sse) {
        hipLaunchKernelGGL(ibq_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)a.part, (int)((n + AT - 1) / AT), sse);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

int64_t vqk_ibq_backward_ws_bytes(int64_t n, int d) {
    if (n < 0 || n >= ((int64_t)1 << 31) || !ibq_d_ok(d)) return VQK_ERR_SHAPE;
    return (2 * n * d + ((n + 3) & ~(int64_t)3)) * 4;
}

int vqk_ibq_backward_f32(const float* z, const float* e, const int64_t* idx, const float* lse, const float* ebar, const void* dq,
                         int dq_dtype, int64_t n, int k, int d, float inv_t, float cz, float ce, const float* gscale_dev, float* dz,
                         float* de, void* ws, int64_t ws_bytes, void* stream) {
    VQK_REQUIRE(z && e && idx && lse && ebar && dz, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && k >= 1 && ibq_d_ok(d), VQK_ERR_SHAPE);
    VQK_REQUIRE(inv_t > 0.0f && inv_t < INFINITY, VQK_ERR_ARG);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(e) && vqk_aligned16(ebar) && vqk_aligned16(dz) && vqk_aligned16(ws) &&
                    (!de || vqk_aligned16(de)) &&
                    (!dq || (dq_dtype == VQK_F32 ? vqk_aligned16(dq) : (reinterpret_cast<uintptr_t>(dq) & 7u) == 0)), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws && ws_bytes >= vqk_ibq_backward_ws_bytes(n, d), VQK_ERR_WORKSPACE);
    hipStream_t st = vqk_stream(stream);
    float* g = reinterpret_cast<float*>(ws);
    float* h = g + n * d;
    float* delta = h + n * d;
    const dim3 rgrid((unsigned)((n + 3) / 4));
#define IBQ_ROWS(T, Q) hipLaunchKernelGGL((ibq_rows_kernel<T, Q>), rgrid, dim3(256), 0, st, z, e, idx, ebar, (const T*)dq, (int)n, k, d, cz, \
                                          ce, gscale_dev, g, h, delta, dz)
    if (!dq) IBQ_ROWS(float, false); else if (dq_dtype == VQK_F32) IBQ_ROWS(float, true); else IBQ_ROWS(bf16_raw, true);
#undef IBQ_ROWS
    VQK_CHECK_LAUNCH();
    IbqArgs a = {};
    a.z = z; a.e = e; a.idx = idx; a.lse = const_cast<float*>(lse); a.g = g; a.h = h; a.delta = delta; a.dz = dz; a.de = de;
    a.n = (int)n; a.k = k; a.inv_t = inv_t;
    return d == 64 ? launch_bwd<64>(a, st) : d == 128 ? launch_bwd<128>(a, st) : launch_bwd<256>(a, st);
}

}  // extern "C"
