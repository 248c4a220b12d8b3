// Lookup-free quantizer (Yu et al. 2023, MAGVIT-v2; Open-MAGVIT2): u = W_in z + b_in, c_j = sign(u_j) (+1 iff u_j > 0), token = the bit
// pattern of (u_j > 0) (first channel = bit 0), q = W_out c + b_out, loss = beta commit + w (H_sample - gamma H_batch) with
// p_nj = sigmoid(a u_nj), a = 4 / tau: the softmax over the 2^d sign codes factorises into d sigmoids, so H_sample costs d terms per
// row, and the batch-average distribution is kept per GROUP of g consecutive bits (tables of 2^g entries).  No codebook, no search.
//
// The kernels work a WAVE PER ROW on the core of proj_quant.h (up to 18 projection channels, 2 chunks per lane: D <= 512) and on the
// sign-quantizer core of sign_quant.h (sigmoid / entropy, group tables, ordered slab sums, the finish and decode kernels, the host
// side); this file holds the forward and the backward kernel body.
// What is per CHANNEL (sigmoid, entropy term, commitment term) runs once per row on lane j for channel j; what is per group CODE runs
// on the lane whose id equals the code's low 6 bits, looping over the remaining 2^(g_s - 6) codes.
// Every sum over rows is ordered, see sign_quant.h.  No fp32 atomics.
#include "common.h"
#include "sign_quant.h"

namespace {

// the value lane `lane` owns out of a wave-uniform register array (0 for lane >= d)
__device__ __forceinline__ float lfq_own(const float (&v)[kSignMaxBits], int lane) {
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < kSignMaxBits; ++j) r = lane == j ? v[j] : r;
    return r;
}

// Forward.  ws == nullptr: assignment only (no loss, no tables).
__global__ __launch_bounds__(kProjThreads) void lfq_forward_kernel(const float* __restrict__ z, const float* __restrict__ w_in,
                                                                    const float* __restrict__ b_in, const float* __restrict__ w_out,
                                                                    const float* __restrict__ b_out, int64_t n, int dm, SignP p,
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
    float zc[kSignMaxChunks][4], zn[kSignMaxChunks][4];
    if (row < n) proj_load_row(z, row, dm, lane, zc);
    for (; row < n; row += stride) {
        if (row + stride < n) proj_load_row(z, row + stride, dm, lane, zn);      // the next row is in flight under this one
        float uj[kSignMaxBits];
#pragma unroll
        for (int j = 0; j < kSignMaxBits; ++j) uj[j] = 0.f;
#pragma unroll
        for (int c = 0; c < kSignMaxChunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) {
                // proj_dot_chunk, written out: through the helper this kernel is allocated 94 VGPRs instead of 98 and scheduled anew
#pragma unroll
                for (int j = 0; j < kSignMaxBits; ++j)
                    if (j < d) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(wi + j * dm + ch);
#pragma unroll
                        for (int i = 0; i < 4; ++i) uj[j] = fmaf(zc[c][i], w[i], uj[j]);
                    }
            }
        }
        unsigned token = 0;
#pragma unroll
        for (int j = 0; j < kSignMaxBits; ++j)
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
            for (int c = 0; c < kSignMaxChunks; ++c) {
                const int ch = (c * 64 + lane) * 4;
                if (ch < dm) {
                    float o[4];
                    proj_q_chunk<kSignMaxBits>(woT, dm, d, SignCode{token, p.s}, b_out, ch, o);
                    proj_store_q(q, q_lo, row * dm + ch, o);
                }
            }
        }
        if (ws) {
            float pj, pmj, hj;
            sign_sigmoid(p.a * mine, pj, pmj, hj);
            if (lane < d) {
                const float diff = mine - (mine > 0.f ? 1.f : -1.f);
                a_commit = fmaf(diff, diff, a_commit);
                a_h += hj;
            }
            for (int s = 0; s < p.groups; ++s) {
                const int base = s * p.g, gs = d - base < p.g ? d - base : p.g;
                float ph[4], pmh[4];
                const float low = sign_group_low<1>(pj, pmj, base, gs, lane, ph, pmh);
                const int nt = gs > 6 ? 1 << (gs - 6) : 1;
                if (lane < (1 << (gs < 6 ? gs : 6)))
                    for (int t = 0; t < nt; ++t) tab[s * p.pitch + t * 64 + lane] += low * sign_group_high(ph, pmh, gs, t);
            }
        }
#pragma unroll
        for (int c = 0; c < kSignMaxChunks; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) zc[c][i] = zn[c][i];
    }
    if (!ws) return;
    const float c_sum = wave_sum(a_commit), h_sum = wave_sum(a_h);
    if (lane == 0) { red[wave * 2] = c_sum; red[wave * 2 + 1] = h_sum; }
    __syncthreads();
    sign_store_fwd_slab(ws, tabs, red, p.tab);
}

// Backward.  grid = (blocks over rows, 256-channel slices), see proj_quant.h.  The gradient at u is straight-through from dq (g = W_out^T dq,
// no tanh) plus s * dloss/du, s = *gscale_dev:
//   dloss/du_nj = c_commit (u - c) - c_hs u p (1 - p) + c_hb sum_m L(m) P_n(m) (bit_j(m) - p_nj)   (m over the codes of j's group)
// The group sum is walked as in the forward: S = sum_m L P and S_j = sum_{m: bit_j(m)} L P per bit, then S_j - p_j S.
template <typename Td>
__global__ __launch_bounds__(kProjThreads) void lfq_backward_kernel(const float* __restrict__ z, const float* __restrict__ u,
                                                                     const Td* __restrict__ dq, const float* __restrict__ w_in,
                                                                     const float* __restrict__ w_out, const float* __restrict__ ltab,
                                                                     const float* __restrict__ gscale_dev, int64_t n, int dm, SignP p,
                                                                     SignLossP lp, float* __restrict__ dz, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float lfq_smem[];
    const int d = p.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.y * kProjSlice;
    const int cn = dm - c0 < kProjSlice ? dm - c0 : kProjSlice;
    float* woT = lfq_smem;                       // [d][dm]
    float* wi = woT + d * dm;                    // [d][cn]
    float* lt = wi + d * kProjSlice;             // [p.tab]
    float* red = lt + p.tab;                     // [kSignRed][64]
    proj_stage_weights(w_in, w_out, dm, d, c0, cn, wi, woT);
    for (int i = threadIdx.x; i < p.tab; i += kProjThreads) lt[i] = ltab[i];
    __syncthreads();
    const float gs_loss = gscale_dev ? *gscale_dev : 1.f;
    const int own = lane * 4;                    // channel inside the slice
    const bool has = own < cn;
    const int nchunks = (dm + 255) / 256;
    float a_wi[kSignMaxBits][4], a_wo[kSignMaxBits][4], a_bo[4], a_bi = 0.f;      // a_bi: lane j holds channel j
#pragma unroll
    for (int j = 0; j < kSignMaxBits; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { a_wi[j][i] = 0.f; a_wo[j][i] = 0.f; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) a_bo[i] = 0.f;

    const int64_t stride = (int64_t)gridDim.x * kProjWaves;
    for (int64_t row = (int64_t)blockIdx.x * kProjWaves + wave; row < n; row += stride) {
        float g[kSignMaxBits], dqo[4] = {0.f, 0.f, 0.f, 0.f}, zo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kSignMaxBits; ++j) g[j] = 0.f;
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
        sign_sigmoid(p.a * mine, pj, pmj, hj);
        float hb = 0.f;                          // sum_m L(m) P(m) (bit_j(m) - p_j) over the group of channel `lane`
        for (int s = 0; s < p.groups; ++s) {
            const int base = s * p.g, gs = d - base < p.g ? d - base : p.g;
            float ph[4], pmh[4];
            const float low = sign_group_low<1>(pj, pmj, base, gs, lane, ph, pmh);
            const int nt = gs > 6 ? 1 << (gs - 6) : 1;
            float all = 0.f, hi[4] = {0.f, 0.f, 0.f, 0.f};
            if (lane < (1 << (gs < 6 ? gs : 6)))
                for (int t = 0; t < nt; ++t) {
                    const float lpm = lt[s * p.pitch + t * 64 + lane] * (low * sign_group_high(ph, pmh, gs, t));
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
        for (int j = 0; j < kSignMaxBits; ++j)
            if (j < d) {
                const float du = wave_sum(g[j]) + __shfl(lgrad, j, 64);
                const float cj = __shfl(cj_mine, j, 64);
                if (lane == j) a_bi += du;
                if (has) proj_accumulate(wi + j * cn + own, du, cj, zo, dqo, dzo, a_wi[j], a_wo[j]);
            }
        if (has) proj_finish_row(dz + row * dm + c0 + own, dzo, dqo, a_bo);
    }

    // the block's waves, added to wave 0 in wave order; two passes through one buffer: (dW_in, db_out), then (dW_out, db_in).  Written
    // out here and in bsq.hip: as a helper of sign_quant.h it costs both backward kernels two more VGPRs (234 / 233 for 232 / 231)
    for (int pass = 0; pass < 2; ++pass)
        for (int w = 1; w < kProjWaves; ++w) {
            __syncthreads();
            if (wave == w) {
#pragma unroll
                for (int j = 0; j < kSignMaxBits; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) red[(j * 4 + i) * 64 + lane] = pass == 0 ? a_wi[j][i] : a_wo[j][i];
#pragma unroll
                for (int i = 0; i < 4; ++i) red[(kSignMaxBits * 4 + i) * 64 + lane] = pass == 0 ? a_bo[i] : a_bi;
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int j = 0; j < kSignMaxBits; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = red[(j * 4 + i) * 64 + lane];
                        if (pass == 0) a_wi[j][i] += v; else a_wo[j][i] += v;
                    }
                if (pass == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) a_bo[i] += red[(kSignMaxBits * 4 + i) * 64 + lane];
                } else {
                    a_bi += red[kSignMaxBits * 4 * 64 + lane];
                }
            }
        }
    if (wave != 0) return;
    float* s_bi = proj_store_slab(ws, dm, d, c0 + own, has, a_wi, a_wo, a_bo);
    if (blockIdx.y == 0 && lane < d) s_bi[lane] = a_bi;
}

// a = 4 / tau, codes +-1, commit a mean over rows and channels
SignKind lfq_kind(int d, float tau) {
    const float a = 4.f / tau;
    return {a, 1.f, (double)a, d};
}

}  // namespace

extern "C" {

int64_t vqk_lfq_ws_bytes(int64_t n, int dm, int d, int g) { return sign_ws_bytes(n, dm, d, g); }

int vqk_lfq_forward(const float* z, const float* w_in, const float* b_in, const float* w_out, const float* b_out, int64_t n, int dm,
                    int d, int g, float tau, float beta, float ratio, float gamma, int64_t* idx, float* u, float* q, void* q_lo,
                    int32_t* hist, float* out, float* ltab, void* ws, int64_t ws_bytes, void* stream) {
    return sign_forward(lfq_forward_kernel, lfq_kind(d, tau), z, w_in, b_in, w_out, b_out, n, dm, d, g, tau, beta, ratio, gamma, idx, u,
                        q, q_lo, hist, out, ltab, ws, ws_bytes, stream);
}

int vqk_lfq_decode(const int64_t* idx, const float* w_out, const float* b_out, int64_t n, int dm, int d, float* q, void* q_lo,
                   void* stream) {
    return sign_decode(lfq_kind(d, 1.f), idx, w_out, b_out, n, dm, d, q, q_lo, stream);
}

int vqk_lfq_backward(const float* z, const float* u, const void* dq, int dq_dtype, const float* w_in, const float* w_out,
                     const float* ltab, const float* gscale_dev, int64_t n, int dm, int d, int g, float tau, float beta, float ratio,
                     float gamma, float* dz, float* dw_in, float* db_in, float* dw_out, float* db_out, int accumulate, void* ws,
                     int64_t ws_bytes, void* stream) {
    return sign_backward(lfq_backward_kernel<float>, lfq_backward_kernel<bf16_raw>, lfq_kind(d, tau), z, u, dq, dq_dtype, w_in, w_out,
                         ltab, gscale_dev, n, dm, d, g, tau, beta, ratio, gamma, dz, dw_in, db_in, dw_out, db_out, accumulate, ws,
                         ws_bytes, stream);
}

}  // extern "C"
