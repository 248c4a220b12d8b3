// Binary spherical quantizer (Zhao, Xiong, Kraehenbuehl 2024, BSQ-ViT): v = W_in z + b_in, u = v / max(|v|, 1e-12) on the unit sphere,
// c_j = +s iff v_j > 0 else -s with s = 1 / sqrt(d), token = the bit pattern of (v_j > 0) (first channel = bit 0), q = W_out c + b_out,
// loss = beta commit + w (H_sample - gamma H_batch): commit = sum |u - c|^2 / N (< 2 whatever d is), p_nj = sigmoid(a u_nj), a = 4 s / tau
// -- the softmax over the 2^d corners factorises as in lfq.hip, and so do the group tables of the batch-average distribution.
//
// The kernels work a WAVE PER ROW on the core of proj_quant.h (up to 18 channels, 2 chunks per lane: D <= 512) and on the
// sign-quantizer core of sign_quant.h (sigmoid / entropy, group tables, ordered slab sums, the finish and decode kernels, the host
// side); this file holds the forward and the backward kernel body.  The d projections of a row go through the TRANSPOSING reduction
// of proj_quant.h: 32 exchanges leave channel j's sum on the lanes 2 j and 2 j + 1, where the per-channel work (normalisation,
// sigmoid, entropy, commitment, the gradient through the sphere) runs -- on the even lane of the pair, the "owner".  |v|^2 and u.e
// are one wave sum over the owners, the token is one ballot.  What is per group CODE runs on the lane whose id equals the code's low
// 6 bits, as in lfq.hip (sign_group_low with a lane stride of 2).  Every sum over rows is ordered, see sign_quant.h.  No fp32 atomics.
#include "common.h"
#include "sign_quant.h"

namespace {

constexpr float kBsqNormEps = 1e-12f;

// Forward.  ws == nullptr: assignment only (no loss, no tables).
__global__ __launch_bounds__(kProjThreads) void bsq_forward_kernel(const float* __restrict__ z, const float* __restrict__ w_in,
                                                                    const float* __restrict__ b_in, const float* __restrict__ w_out,
                                                                    const float* __restrict__ b_out, int64_t n, int dm, SignP p,
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
    float zc[kSignMaxChunks][4], zn[kSignMaxChunks][4];
    if (row < n) proj_load_row(z, row, dm, lane, zc);
    for (; row < n; row += stride) {
        if (row + stride < n) proj_load_row(z, row + stride, dm, lane, zn);      // the next row is in flight under this one
        float vj[kSignMaxBits];
#pragma unroll
        for (int j = 0; j < kSignMaxBits; ++j) vj[j] = 0.f;
#pragma unroll
        for (int c = 0; c < kSignMaxChunks; ++c) {
            const int ch = (c * 64 + lane) * 4;
            if (ch < dm) proj_dot_chunk<kSignMaxBits>(wi, dm, d, ch, zc[c], vj);
        }
        const float v = proj_transpose_sum<kSignMaxBits>(vj, lane) + bias;        // channel mych
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
            sign_sigmoid(p.a * u, pj, pmj, hj);
            if (owner) {
                const float diff = u - (v > 0.f ? p.s : -p.s);
                a_commit = fmaf(diff, diff, a_commit);
                a_h += hj;
            }
            for (int s = 0; s < p.groups; ++s) {
                const int base = s * p.g, gs = d - base < p.g ? d - base : p.g;
                float ph[4], pmh[4];
                const float low = sign_group_low<2>(pj, pmj, base, gs, lane, ph, pmh);
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
                                                                     int64_t n, int dm, SignP p, SignLossP lp, float* __restrict__ dz,
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
    float* red = lt + p.tab;                     // [kSignRed][64]
    proj_stage_weights(w_in, w_out, dm, d, c0, cn, wi, woT);
    for (int i = threadIdx.x; i < p.tab; i += kProjThreads) lt[i] = ltab[i];
    __syncthreads();
    const float gs_loss = gscale_dev ? *gscale_dev : 1.f;
    const int ownc = lane * 4;                   // channel inside the slice
    const bool has = ownc < cn;
    const int nchunks = (dm + 255) / 256;
    float a_wi[kSignMaxBits][4], a_wo[kSignMaxBits][4], a_bo[4], a_bi = 0.f;      // a_bi: the owner of channel j holds channel j
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
                proj_dot_chunk<kSignMaxBits>(woT, dm, d, ch, v, g);
            }
        }
        const float gj = proj_transpose_sum<kSignMaxBits>(g, lane);              // channel mych of W_out^T dq
        // the loss gradient of channel mych
        float pj, pmj, hj;
        sign_sigmoid(p.a * mine, pj, pmj, hj);
        const unsigned token = proj_tr_bits(__ballot(owner && mine > 0.f));
        float hb = 0.f;                          // sum_m L(m) P(m) (bit_j(m) - p_j) over the group of channel mych
        for (int s = 0; s < p.groups; ++s) {
            const int base = s * p.g, gs = d - base < p.g ? d - base : p.g;
            // sum_m P(m) (bit_j(m) - p_j) = 0, so L may be shifted by a constant: by L at the row's own code of this group, the code
            // that carries most of P.  A near-uniform Pbar (L almost constant) then leaves small terms instead of the difference of
            // large ones, and a saturated row has its one large term exactly zero.
            const float l0 = lt[s * p.pitch + (int)((token >> base) & ((1u << gs) - 1u))];
            float ph[4], pmh[4];
            const float low = sign_group_low<2>(pj, pmj, base, gs, lane, ph, pmh);
            const int nt = gs > 6 ? 1 << (gs - 6) : 1;
            float all = 0.f, hi[4] = {0.f, 0.f, 0.f, 0.f};
            if (lane < (1 << (gs < 6 ? gs : 6)))
                for (int t = 0; t < nt; ++t) {
                    const float lpm = (lt[s * p.pitch + t * 64 + lane] - l0) * (low * sign_group_high(ph, pmh, gs, t));
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
        const SignCode code{token, p.s};
        float dzo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kSignMaxBits; ++j)
            if (j < d) {
                const float du = proj_tr_read(dv, j);
                if (has) proj_accumulate(wi + j * cn + ownc, du, code(j), zo, dqo, dzo, a_wi[j], a_wo[j]);
            }
        if (has) proj_finish_row(dz + row * dm + c0 + ownc, dzo, dqo, a_bo);
    }

    // the block's waves, added to wave 0 in wave order; two passes through one buffer: (dW_in, db_out), then (dW_out, db_in); written
    // out as in lfq.hip (sign_quant.h has the figures)
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
    float* s_bi = proj_store_slab(ws, dm, d, c0 + ownc, has, a_wi, a_wo, a_bo);
    if (blockIdx.y == 0 && owner) s_bi[mych] = a_bi;
}

// s = 1 / sqrt(d), a = 4 s / tau, commit a sum over channels and a mean over rows
SignKind bsq_kind(int d, float tau) {
    const double s = 1.0 / std::sqrt((double)d);
    return {(float)(4.0 * s / (double)tau), (float)s, 4.0 / (std::sqrt((double)d) * (double)tau), 1};
}

}  // namespace

extern "C" {

int64_t vqk_bsq_ws_bytes(int64_t n, int dm, int d, int g) { return sign_ws_bytes(n, dm, d, g); }

int vqk_bsq_forward(const float* z, const float* w_in, const float* b_in, const float* w_out, const float* b_out, int64_t n, int dm,
                    int d, int g, float tau, float beta, float ratio, float gamma, int64_t* idx, float* u, float* r, float* q, void* q_lo,
                    int32_t* hist, float* out, float* ltab, void* ws, int64_t ws_bytes, void* stream) {
    return sign_forward(bsq_forward_kernel, bsq_kind(d, tau), z, w_in, b_in, w_out, b_out, n, dm, d, g, tau, beta, ratio, gamma, idx, u,
                        q, q_lo, hist, out, ltab, ws, ws_bytes, stream, r);
}

int vqk_bsq_decode(const int64_t* idx, const float* w_out, const float* b_out, int64_t n, int dm, int d, float* q, void* q_lo,
                   void* stream) {
    return sign_decode(bsq_kind(d, 1.f), idx, w_out, b_out, n, dm, d, q, q_lo, stream);
}

int vqk_bsq_backward(const float* z, const float* u, const float* r, const void* dq, int dq_dtype, const float* w_in, const float* w_out,
                     const float* ltab, const float* gscale_dev, int64_t n, int dm, int d, int g, float tau, float beta, float ratio,
                     float gamma, float* dz, float* dw_in, float* db_in, float* dw_out, float* db_out, int accumulate, void* ws,
                     int64_t ws_bytes, void* stream) {
    return sign_backward(bsq_backward_kernel<float>, bsq_backward_kernel<bf16_raw>, bsq_kind(d, tau), z, u, dq, dq_dtype, w_in, w_out,
                         ltab, gscale_dev, n, dm, d, g, tau, beta, ratio, gamma, dz, dw_in, db_in, dw_out, db_out, accumulate, ws,
                         ws_bytes, stream, r);
}

}  // extern "C"
