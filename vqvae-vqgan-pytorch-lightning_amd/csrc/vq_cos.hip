// ------------------------------------------------------------------------------------------------
// Cosine quantizer (Yu et al. 2022, ViT-VQGAN: the factorised, l2-normalised codebook): a low-dimensional latent (D = 8..64) and the
// codes are both l2-normalised before the lookup, so the Euclidean ranking is the cosine ranking, and the decoder sees the
// normalised code.
//   zn = nrm(z), en = nrm(e)  (vq_cos.h: one device function, the same bits everywhere);
//   k = argmin_k (|zn|^2 + |en_k|^2) - 2 zn.en_k  in the arithmetic of vq.hip::row_sqnorm_kernel / vq_assign_kernel, first minimum;
//   q = en[k];  sse = sum |q - zn|^2;  hist[k] += 1.
//
// PREPARE (once per codebook change): en[K][D], |en|^2[K] and inv_e[K] into the caller's workspace.
//
// FORWARD = one kernel.  A block owns 32 rows: they are staged in LDS, normalised there (one wavefront per row, cos_nrm_row), and
// ranked against en streamed from L2 with the MFMA sequence, k order and comparisons of vq_assign_kernel (every wave walks a quarter
// of the 32-code tiles with a lane-local running (min, argmin); no N x K matrix); the epilogue gathers en[k], writes q as fp32 and /
// or bf16, adds |q - zn|^2 to the block's partial of sse (one atomic per block; deterministic mode: the partials go through the
// ordered-sum workspace and a second, one-thread launch adds them in block order) and counts hist with in-block duplicates first.
// The kernel evaluates the fp32 expression sequence of vqk_l2norm_rows_f32 + vqk_row_sqnorm_f32 + vqk_vq_assign_f32 on the same
// values: it equals that staged formulation bit for bit.
//
// BACKWARD re-normalises z with the same function (the same bits; nothing but idx is saved).  With s the upstream loss gradient:
//   g = dq + s cz (zn - q);  dz = (g - zn (zn.g)) inv_z  (evaluated in float64 from z: the projection cancels);
//   de[k] += s ce inv_e[k] (en_k (en_k.S_k) - S_k),  S_k = sum_{rows: idx = k} zn  (the per-row term en_k (en_k.zn) - zn is linear).
// Default: the rows of a 32-row block that share a code are summed through an LDS tile, projected once and sent as ONE coalesced
// fp32 atomic row per distinct (code, block) -- CHAINS of vq_lookup.h (the walk itself is written out here: d <= 64 on a 64-pitch
// tile with a projection before the atomic).  Deterministic mode: the per-row terms go to the caller's workspace and one block per
// code adds its rows in row order -- ORDERED SCAN of vq_lookup.h.  The block partial of sse, its ordered sum and the decode kernel
// (the residual quantizer's at depth 1) are that header's too.
// ------------------------------------------------------------------------------------------------
#include "vq_cos.h"
#include "vq_lookup.h"

namespace {

// one wavefront per row, any d % 4 == 0: xn (and optionally inv and |xn|^2)
__global__ __launch_bounds__(256) void cos_l2norm_kernel(const float* __restrict__ x, int64_t rows, int d, float* __restrict__ xn,
                                                         float* __restrict__ inv, float* __restrict__ nn) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float nn_v;
    const float iv = cos_nrm_row(x + row * d, d, lane, xn + row * d, nn_v);
    if (lane == 0) {
        if (inv) inv[row] = iv;
        if (nn) nn[row] = nn_v;
    }
}

// thread-local part of sum |q - zn|^2 (the fused epilogue and the staged path's deterministic sum share it)
__device__ __forceinline__ float cos_sse_acc(float local, const f32x4 ev, const f32x4 zv) {
#pragma unroll
    for (int t = 0; t < 4; ++t) { const float u = __fsub_rn(ev[t], zv[t]); local = __fmaf_rn(u, u, local); }
    return local;
}

// the block's partial: waves by butterfly, then (w0 + w1) + (w2 + w3); to the ordered-sum workspace or one atomic
__device__ __forceinline__ void cos_block_sse(float local, float* part, float* __restrict__ sse, float* __restrict__ sse_part) {
    lk_wave_part(local, part, threadIdx.x & 63, threadIdx.x >> 6);
    __syncthreads();
    if (threadIdx.x == 0) lk_sse_emit(part, sse, sse_part, blockIdx.x);
}

template <int D>
__global__ __launch_bounds__(256) void cos_forward_kernel(const float* __restrict__ z, const float* __restrict__ en,
                                                          const float* __restrict__ e2, int64_t n, int k, int64_t* __restrict__ idx,
                                                          float* __restrict__ q32, bf16_raw* __restrict__ q_lo,
                                                          float* __restrict__ sse, float* __restrict__ sse_part,
                                                          int32_t* __restrict__ hist) {
    constexpr int LD = D + 4, VPR = D / 4;
    __shared__ __attribute__((aligned(16))) float zt[32 * LD];  // the block's rows, normalised in place (rows past n: row n - 1)
    __shared__ float z2_s[32];
    __shared__ float red_d[128];
    __shared__ int red_i[128];
    __shared__ int fin[32];
    __shared__ float part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * 32;

    for (int v = tid; v < 32 * VPR; v += 256) {
        const int r = v / VPR, c = v - r * VPR;
        int64_t src = n0 + r; if (src >= n) src = n - 1;
        *reinterpret_cast<f32x4*>(zt + r * LD + 4 * c) = *reinterpret_cast<const f32x4*>(z + src * D + 4 * c);
    }
    __syncthreads();
    for (int i = 0; i < 8; ++i) {
        const int r = wave * 8 + i;
        float nn;
        cos_nrm_row(zt + r * LD, D, lane, zt + r * LD, nn);
        if (lane == 0) z2_s[r] = nn;
    }
    __syncthreads();

    // ranking: vq_assign_kernel<0> on (zn, en) -- A = codes, B = rows; lane (j, half) owns row j and 16 codes of the tile
    const int j = lane & 31, half = lane >> 5;
    const float zz = z2_s[j];
    const float* zb = zt + j * LD + 4 * half;
    const int tiles = k >> 5;
    const int per_wave = (tiles + 3) >> 2;
    const int t_begin = wave * per_wave;
    const int t_end = min(tiles, t_begin + per_wave);
    // the row's fragments are the same for every tile: registers.  The code fragments and |en|^2 of tile t + 1 are loaded before
    // the MFMAs of tile t (one wave per SIMD at N = 8192: nothing else hides the L2 latency)
    constexpr int NF = D / 8;
    f32x4 b[NF], a_cur[NF], a_nxt[NF], e2_cur[4], e2_nxt[4];
#pragma unroll
    for (int m = 0; m < NF; ++m) b[m] = *reinterpret_cast<const f32x4*>(zb + 8 * m);
    if (t_begin < t_end) {
        const float* ea = en + (int64_t)(t_begin * 32 + j) * D + 4 * half;
#pragma unroll
        for (int m = 0; m < NF; ++m) a_cur[m] = *reinterpret_cast<const f32x4*>(ea + 8 * m);
#pragma unroll
        for (int g = 0; g < 4; ++g) e2_cur[g] = *reinterpret_cast<const f32x4*>(e2 + t_begin * 32 + 8 * g + 4 * half);
    }
    float best = INFINITY;
    int best_i = 0x7fffffff;
    for (int t = t_begin; t < t_end; ++t) {
        if (t + 1 < t_end) {
            const float* ea = en + (int64_t)((t + 1) * 32 + j) * D + 4 * half;
#pragma unroll
            for (int m = 0; m < NF; ++m) a_nxt[m] = *reinterpret_cast<const f32x4*>(ea + 8 * m);
#pragma unroll
            for (int g = 0; g < 4; ++g) e2_nxt[g] = *reinterpret_cast<const f32x4*>(e2 + (t + 1) * 32 + 8 * g + 4 * half);
        }
        f32x16 acc = {0};
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[m][0], b[m][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[m][1], b[m][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[m][2], b[m][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[m][3], b[m][3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int code = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;       // = e2_cur[r >> 2][r & 3]
            const float ab2 = 2.0f * acc[r];
            const float dist = __fsub_rn(__fadd_rn(zz, e2_cur[r >> 2][r & 3]), ab2);
            if (dist < best) { best = dist; best_i = code; }
        }
#pragma unroll
        for (int m = 0; m < NF; ++m) a_cur[m] = a_nxt[m];
#pragma unroll
        for (int g = 0; g < 4; ++g) e2_cur[g] = e2_nxt[g];
    }
    {
        const float od = __shfl_xor(best, 32, 64);
        const int oi = __shfl_xor(best_i, 32, 64);
        if (od < best || (od == best && oi < best_i)) { best = od; best_i = oi; }
    }
    if (half == 0) { red_d[wave * 32 + j] = best; red_i[wave * 32 + j] = best_i; }
    __syncthreads();
    if (tid < 32) {
        float bd = red_d[tid]; int bi = red_i[tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float od = red_d[w * 32 + tid]; const int oi = red_i[w * 32 + tid];
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        if (bi == 0x7fffffff) bi = 0;
        fin[tid] = bi;
        if (n0 + tid < n) idx[n0 + tid] = (int64_t)bi;
    }
    __syncthreads();

    // epilogue: q = en[k] as fp32 and / or bf16, |q - zn|^2
    if (q32 || q_lo || sse) {
        float local = 0.0f;
        for (int v = tid; v < 32 * VPR; v += 256) {
            const int r = v / VPR, c = (v - r * VPR) * 4;
            if (n0 + r >= n) continue;
            const f32x4 ev = *reinterpret_cast<const f32x4*>(en + (int64_t)fin[r] * D + c);
            const f32x4 zv = *reinterpret_cast<const f32x4*>(zt + r * LD + c);
            const int64_t o = (n0 + r) * D + c;
            if (q32) *reinterpret_cast<f32x4*>(q32 + o) = ev;
            if (q_lo) {
                const u16x4 ob = {f32_to_bf16(ev[0]), f32_to_bf16(ev[1]), f32_to_bf16(ev[2]), f32_to_bf16(ev[3])};
                *reinterpret_cast<u16x4*>(q_lo + o) = ob;
            }
            local = cos_sse_acc(local, ev, zv);
        }
        if (sse) cos_block_sse(local, part, sse, sse_part);
    }
    // histogram: duplicates inside the block are counted first
    if (hist && tid < 32 && n0 + tid < n) {
        const int code = fin[tid];
        int count = 0;
        bool leader = true;
        for (int u = 0; u < 32; ++u) {
            const bool same = (n0 + u < n) && fin[u] == code;
            count += same ? 1 : 0;
            if (same && u < tid) leader = false;
        }
        if (leader) atomicAdd(hist + code, count);
    }
}

// sum |q - zn|^2 over materialised rows with the fused epilogue's thread mapping and block partials (the staged formulation in
// deterministic mode: the same bits as the fused kernel)
__global__ __launch_bounds__(256) void cos_sse_kernel(const float* __restrict__ zn, const float* __restrict__ q, int64_t n, int d,
                                                      float* __restrict__ sse, float* __restrict__ sse_part) {
    __shared__ float part[4];
    const int vpr = d >> 2;
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    float local = 0.0f;
    for (int v = threadIdx.x; v < 32 * vpr; v += 256) {
        const int r = v / vpr, c = (v - r * vpr) * 4;
        if (n0 + r >= n) continue;
        const int64_t o = (n0 + r) * d + c;
        local = cos_sse_acc(local, *reinterpret_cast<const f32x4*>(q + o), *reinterpret_cast<const f32x4*>(zn + o));
    }
    cos_block_sse(local, part, sse, sse_part);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// block = 32 rows, wave w: rows 8 w .. 8 w + 7, lane = column (d <= 64).
// DE: 0 no codebook gradient, 1 LDS chains + atomics, 2 the per-row terms to contrib[N][d] (deterministic mode).
// A token outside [0, K) (never written by the forward) is treated as a zero code without a gradient.
template <typename TDQ, bool HAS_DQ, int DE>
__global__ __launch_bounds__(256) void cos_backward_kernel(const float* __restrict__ z, const float* __restrict__ en,
                                                           const float* __restrict__ inv_e, const int64_t* __restrict__ idx,
                                                           const TDQ* __restrict__ dq, int64_t n, int k, int d, float cz, float ce,
                                                           const float* __restrict__ gs, float* __restrict__ dz,
                                                           float* __restrict__ de, float* __restrict__ contrib) {
    __shared__ float tile[DE != 0 ? 32 * 64 : 1];                // zn of the block's rows
    __shared__ int code_s[32], next_s[32], first_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    if (gs) { const float sc = *gs; cz *= sc; ce *= sc; }
    const bool on = lane < d;
    if (tid < 32) {
        const int64_t c = n0 + tid < n ? idx[n0 + tid] : -1;
        code_s[tid] = (c >= 0 && c < k) ? (int)c : -1;
    }
    __syncthreads();
    for (int i = 0; i < 8; ++i) {
        const int r = wave * 8 + i;
        const int64_t row = n0 + r;
        if (row >= n) break;                                     // wave-uniform
        const int code = code_s[r];
        const float qv = (on && code >= 0) ? en[(int64_t)code * d + lane] : 0.0f;
        // dz in float64 from z itself: the projection g - zn (zn.g) cancels, and zn rounded to fp32 would leave 1e-7 |g| in it
        const double xd = on ? (double)z[row * d + lane] : 0.0;
        const double invd = 1.0 / fmax(sqrt(wave_sum_f64(xd * xd)), (double)COS_EPS);
        const double znd = xd * invd;
        double g = 0.0;
        if (HAS_DQ && on) g = (double)Elem<TDQ>::ld(dq + row * d + lane);
        g = fma((double)cz, znd - (double)qv, g);
        const double dot = wave_sum_f64(znd * g);
        if (on) dz[row * d + lane] = (float)((g - znd * dot) * invd);
        if (DE != 0) {
            // the codebook term works on the forward's zn (the same bits)
            float* tr = tile + r * 64;
            float nn;
            cos_nrm_row(z + row * d, d, lane, tr, nn);
            if (DE == 2) {
                // the row's term en_k (en_k.zn) - zn (en_k = q)
                const float znv = on ? tr[lane] : 0.0f;
                const float eq = wave_sum(qv * znv);
                if (on) contrib[row * d + lane] = code >= 0 ? __fmaf_rn(qv, eq, -znv) : 0.0f;
            }
        }
    }
    if constexpr (DE == 1) {
        __syncthreads();
        if (tid < 32) lk_build_chains(code_s, first_s, next_s, tid);
        __syncthreads();
        // wave w: heads w, w + 4, ...; ONE projected, coalesced fp32 atomic row per distinct code of the block
        for (int r = wave; r < 32; r += 4) {
            const int code = code_s[r];
            if (code < 0 || first_s[r] != r) continue;           // wave-uniform
            float s = 0.0f;
            for (int m = r; m >= 0; m = next_s[m]) s += on ? tile[m * 64 + lane] : 0.0f;
            const float ev = on ? en[(int64_t)code * d + lane] : 0.0f;
            const float dot = wave_sum(ev * s);
            if (on) atomicAdd(de + (int64_t)code * d + lane, ce * inv_e[code] * __fmaf_rn(ev, dot, -s));
        }
    }
}

// Deterministic codebook gradient: one block per code scans idx[N] in chunks of 256 (a wave's matches as one ballot mask, the four
// masks through LDS); thread c < d adds column c of the matching rows of contrib, lowest row first.
__global__ __launch_bounds__(256) void cos_code_grad_ordered_kernel(const float* __restrict__ contrib, const int64_t* __restrict__ idx,
                                                                    int64_t rows, int d, float ce, const float* __restrict__ gs,
                                                                    const float* __restrict__ inv_e, float* __restrict__ de) {
    __shared__ unsigned long long masks[4];
    const int64_t code = blockIdx.x;
    const int tid = threadIdx.x;
    if (gs) ce *= *gs;
    float acc = 0.f;
    lk_ordered_scan(idx, rows, code, masks, tid < d, [&](int64_t r) { acc += contrib[r * d + tid]; });
    if (tid < d) de[code * d + tid] += ce * inv_e[code] * acc;
}

static inline bool cos_fused_d(int d) { return d == 8 || d == 16 || d == 32 || d == 64; }

}  // namespace

extern "C" {

int vqk_l2norm_rows_f32(const float* x, int64_t rows, int d, float* xn, float* inv, void* stream) {
    VQK_REQUIRE(x && xn, VQK_ERR_ARG);
    VQK_REQUIRE(rows >= 0 && d > 0 && (d % 4) == 0, VQK_ERR_SHAPE);
    if (rows == 0) return VQK_OK;
    hipLaunchKernelGGL(cos_l2norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, vqk_stream(stream), x, rows, d, xn, inv,
                       (float*)nullptr);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int64_t vqk_cos_ws_bytes(int k, int d) {
    if (k <= 0 || k >= (1 << 26) || d <= 0 || (d % 4) != 0) return VQK_ERR_SHAPE;
    return cos_ws_size(k, d);
}

int vqk_cos_prepare_f32(const float* e, int k, int d, void* ws, int64_t ws_bytes, void* stream) {
    VQK_REQUIRE(e && ws, VQK_ERR_ARG);
    VQK_REQUIRE(k > 0 && k < (1 << 26) && d > 0 && (d % 4) == 0, VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= cos_ws_size(k, d), VQK_ERR_WORKSPACE);
    char* w = reinterpret_cast<char*>(ws);
    hipLaunchKernelGGL(cos_l2norm_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, vqk_stream(stream), e, (int64_t)k, d,
                       reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + cos_off_inv(k, d)),
                       reinterpret_cast<float*>(w + cos_off_e2(k, d)));
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_cos_forward_f32(const float* z, const void* ws, int64_t ws_bytes, int64_t n, int k, int d, int64_t* idx, float* q, void* q_lo,
                        float* sse, int32_t* hist, void* stream) {
    VQK_REQUIRE(z && ws && idx, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0 && k < (1 << 26) && (k % 32) == 0 && cos_fused_d(d), VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(ws) && (!q || vqk_aligned16(q)) && (!q_lo || (reinterpret_cast<uintptr_t>(q_lo) & 7u) == 0),
                VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= cos_ws_size(k, d), VQK_ERR_WORKSPACE);
    if (n == 0) return VQK_OK;
    const char* w = reinterpret_cast<const char*>(ws);
    const float* en = reinterpret_cast<const float*>(w);
    const float* e2 = reinterpret_cast<const float*>(w + cos_off_e2(k, d));
    const dim3 grid((unsigned)((n + 31) / 32));
    hipStream_t st = vqk_stream(stream);
    LK_SSE_PART(sse_part, sse, grid.x)
#define COS_LAUNCH(DD) hipLaunchKernelGGL((cos_forward_kernel<DD>), grid, dim3(256), 0, st, z, en, e2, n, k, idx, q, \
                                          reinterpret_cast<bf16_raw*>(q_lo), sse, sse_part, hist)
    if (d == 8) COS_LAUNCH(8); else if (d == 16) COS_LAUNCH(16); else if (d == 32) COS_LAUNCH(32); else COS_LAUNCH(64);
#undef COS_LAUNCH
    VQK_CHECK_LAUNCH();
    if (sse_part) {
        hipLaunchKernelGGL(lk_sse_ordered_kernel<float>, dim3(1), dim3(64), 0, st, (const float*)sse_part, (int)grid.x, 1, sse);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

int vqk_cos_sse_f32(const float* zn, const float* q, int64_t n, int d, float* sse, void* stream) {
    VQK_REQUIRE(zn && q && sse, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && d > 0 && (d % 4) == 0, VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(zn) && vqk_aligned16(q), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    const dim3 grid((unsigned)((n + 31) / 32));
    hipStream_t st = vqk_stream(stream);
    LK_SSE_PART(sse_part, true, grid.x)
    hipLaunchKernelGGL(cos_sse_kernel, grid, dim3(256), 0, st, zn, q, n, d, sse, sse_part);
    VQK_CHECK_LAUNCH();
    if (sse_part) {
        hipLaunchKernelGGL(lk_sse_ordered_kernel<float>, dim3(1), dim3(64), 0, st, (const float*)sse_part, (int)grid.x, 1, sse);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

int vqk_cos_decode_f32(const int64_t* idx, const void* ws, int64_t ws_bytes, int64_t n, int k, int d, float* q, void* q_lo,
                       void* stream) {
    VQK_REQUIRE(idx && ws && (q || q_lo), VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0 && k < (1 << 26) && d > 0 && (d % 4) == 0, VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(ws) && (!q || vqk_aligned16(q)) && (!q_lo || (reinterpret_cast<uintptr_t>(q_lo) & 7u) == 0), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= cos_ws_size(k, d), VQK_ERR_WORKSPACE);
    if (n == 0) return VQK_OK;
    hipLaunchKernelGGL(lk_decode_kernel<false>, dim3(vqk_grid_1d(n * (d / 4), 256)), dim3(256), 0, vqk_stream(stream), idx,
                       reinterpret_cast<const float*>(ws), n, k, d, 1, q, reinterpret_cast<bf16_raw*>(q_lo));
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int64_t vqk_cos_backward_ws_bytes(int64_t n, int d) {
    if (n < 0 || !cos_fused_d(d)) return VQK_ERR_SHAPE;
    return (n > 0 ? n : 1) * (int64_t)d * 4;
}

int vqk_cos_backward_f32(const float* z, const void* ws, const int64_t* idx, const void* dq, int dq_dtype, int64_t n, int k, int d,
                         float cz, float ce, const float* gscale_dev, float* dz, float* de, void* ws2, int64_t ws2_bytes,
                         void* stream) {
    VQK_REQUIRE(z && ws && idx && dz, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0 && k < (1 << 26) && cos_fused_d(d), VQK_ERR_SHAPE);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(vqk_aligned16(ws), VQK_ERR_ALIGN);
    const bool ordered = de && vqkd::det_state().on;             // the per-row terms go through ws2
    if (ordered) VQK_REQUIRE(ws2 && ws2_bytes >= vqk_cos_backward_ws_bytes(n, d), VQK_ERR_WORKSPACE);
    if (n == 0) return VQK_OK;
    const char* w = reinterpret_cast<const char*>(ws);
    const float* en = reinterpret_cast<const float*>(w);
    const float* inv_e = reinterpret_cast<const float*>(w + cos_off_inv(k, d));
    const dim3 grid((unsigned)((n + 31) / 32));
    hipStream_t st = vqk_stream(stream);
    float* contrib = ordered ? reinterpret_cast<float*>(ws2) : nullptr;
#define CSB(T, Q, E) hipLaunchKernelGGL((cos_backward_kernel<T, Q, E>), grid, dim3(256), 0, st, z, en, inv_e, idx, (const T*)dq, n, k, d, \
                                       cz, ce, gscale_dev, dz, de, contrib)
    LK_DISPATCH_DQ_DE(CSB, dq, dq_dtype, !de ? 0 : !ordered ? 1 : 2);
#undef CSB
    VQK_CHECK_LAUNCH();
    if (ordered) {
        hipLaunchKernelGGL(cos_code_grad_ordered_kernel, dim3((unsigned)k), dim3(256), 0, st, (const float*)contrib, idx, n, d, ce,
                           gscale_dev, inv_e, de);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

}  // extern "C"
