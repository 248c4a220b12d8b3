// ------------------------------------------------------------------------------------------------
// SimVQ (Zhu et al. 2024, "Addressing representation collapse in vector quantized models with one linear layer"): the code table
// c[K][D] is FROZEN at its random start and one D x D linear layer (w[D][D] in nn.Linear orientation, bias b[D]) is learned; the
// effective codebook is  E = c w^T + b.  The lookup against E is the standard quantizer's (vq.hip / vq_filter.hip, assoc 0); this
// file holds the two pieces that are new:
//
// PROJECTION  E[k][i] = sum_j c[k][j] w[i][j] + b[i]  in exact fp32 products and fp32 accumulation (v_mfma_f32_32x32x2_f32).
//   Block = D / 32 wavefronts (2 D threads).  Wave v owns the output columns i in [32 v, 32 v + 32): its rows of w stay in registers
//   for the whole kernel as MFMA A fragments (lane (j, half): w[32 v + j][8 m + 4 half .. + 4), m < D / 8).  The block walks code
//   tiles of 8192 / D codes (32 KB of c, read once with coalesced 16-byte loads into a [codes][D + 4] LDS tile); per 32 codes a wave
//   runs D / 2 MFMAs whose B fragments are 16-byte LDS reads of the same columns, adds the bias and writes E with one 16-byte store per
//   (code, four columns).  The order of the sum over j is  for m: for t < 4: (j = 8 m + t, j = 8 m + 4 + t)  -- fixed for a given D.
//
// BACKWARD, straight-through:  dz = fma(s cz, z - q, dq)  (the expression and bits of vq.hip::vq_backward_kernel),
//   g_r = s ce (q_r - z_r);  dw[i][j] += sum_r g_r[i] c[idx_r][j];  db[i] += sum_r g_r[i];  c receives nothing.  A [K][D] codebook
//   gradient is never formed: the sum over rows is a gather-GEMM of 2 N D^2 FLOP.
//   Launch 1: at most 256 blocks of D / 32 wavefronts; block b walks rows [b R, (b + 1) R) in chunks of 32, ascending, R a function
//   of n alone (simvq_rows_per_block).  Per chunk it stages g and the gathered rows of c in two [32][D + 32] LDS tiles (writing dz on
//   the way, 16-byte loads and stores), then wave v accumulates the 32 x D strip i in [32 v, 32 v + 32) of g^T c_gathered in D / 32
//   accumulator tiles (16 MFMA steps of two rows each per tile) and thread i < D adds column i of g, row by row.  The D x D partial and
//   the D column sums go to the block's own slice of ws.
//   Launch 2: one thread per element of dw and db adds the slices in block order and then does ONE read-modify-write of the target,
//   which may be a view of the optimizer's gradient arena that already holds values.  No float atomics: the same inputs give the same
//   bits in every run and in every mode, so there is no deterministic-mode twin.
//   A token outside [0, K) is a zero code: q = 0 in dz, nothing read from e or c, nothing added to dw or db.
// ------------------------------------------------------------------------------------------------
#include "common.h"

namespace {

constexpr int SIMVQ_MAX_BLOCKS = 256;

static inline bool simvq_d_ok(int d) { return d == 64 || d == 128 || d == 256; }

// rows per block of the backward: whole chunks of 32 rows, at least two, and as many as keep the grid at or below 256 blocks
static inline int64_t simvq_rows_per_block(int64_t n) {
    const int64_t chunks = (n + 31) / 32;
    int64_t cpb = (chunks + SIMVQ_MAX_BLOCKS - 1) / SIMVQ_MAX_BLOCKS;
    if (cpb < 2) cpb = 2;
    return cpb * 32;
}
static inline int64_t simvq_blocks(int64_t n) {
    const int64_t rpb = simvq_rows_per_block(n);
    return (n + rpb - 1) / rpb;
}

template <int D>
__global__ __launch_bounds__(2 * D) void simvq_project_kernel(const float* __restrict__ c, const float* __restrict__ w,
                                                              const float* __restrict__ bias, int k, float* __restrict__ e) {
    constexpr int LD = D + 4, VPR = D / 4, CT = 8192 / D, NF = D / 8, NT = 2 * D;
    __shared__ __attribute__((aligned(16))) float ct[CT * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int i0 = 32 * wave;

    f32x4 a[NF];                                                 // w[i0 + j][8 m + 4 half .. + 4): the A fragments of every code tile
    {
        const float* wr = w + (int64_t)(i0 + j) * D + 4 * half;
#pragma unroll
        for (int m = 0; m < NF; ++m) a[m] = *reinterpret_cast<const f32x4*>(wr + 8 * m);
    }
    f32x4 bv[4];                                                 // bias[i0 + 8 u + 4 half .. + 4): the columns of acc[4 u .. 4 u + 3]
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        bv[u] = bias ? *reinterpret_cast<const f32x4*>(bias + i0 + 8 * u + 4 * half) : zero;
    }

    const int tiles = (k + CT - 1) / CT;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int k0 = t * CT;
        const int codes = min(CT, k - k0);                       // a multiple of 32
        for (int v = tid; v < codes * VPR; v += NT) {
            const int r = v / VPR, cc = (v - r * VPR) * 4;
            *reinterpret_cast<f32x4*>(ct + r * LD + cc) = *reinterpret_cast<const f32x4*>(c + (int64_t)(k0 + r) * D + cc);
        }
        __syncthreads();
        for (int s = 0; s < codes; s += 32) {
            const float* cb = ct + (s + j) * LD + 4 * half;
            f32x16 acc = {0};
#pragma unroll
            for (int m = 0; m < NF; ++m) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(cb + 8 * m);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][0], b[0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][1], b[1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][2], b[2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][3], b[3], acc, 0, 0, 0);
            }
            // acc[r] = E[k0 + s + j][i0 + (r & 3) + 8 (r >> 2) + 4 half]
            float* er = e + (int64_t)(k0 + s + j) * D + i0 + 4 * half;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                f32x4 o = {acc[4 * u], acc[4 * u + 1], acc[4 * u + 2], acc[4 * u + 3]};
                if (bias) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = __fadd_rn(o[q], bv[u][q]);
                }
                *reinterpret_cast<f32x4*>(er + 8 * u) = o;
            }
        }
        __syncthreads();
    }
}

template <typename TDQ> struct SimvqDq;
template <> struct SimvqDq<float> {
    __device__ static __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
};
template <> struct SimvqDq<bf16_raw> {
    __device__ static __forceinline__ f32x4 ld4(const bf16_raw* p) {
        const u16x4 v = *reinterpret_cast<const u16x4*>(p);
        const f32x4 o = {bf16_to_f32(v[0]), bf16_to_f32(v[1]), bf16_to_f32(v[2]), bf16_to_f32(v[3])};
        return o;
    }
};

template <int D, typename TDQ, bool HAS_DQ>
__global__ __launch_bounds__(2 * D) void simvq_backward_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                               const float* __restrict__ c, const int64_t* __restrict__ idx,
                                                               const TDQ* __restrict__ dq, int64_t n, int k, int64_t rows_per_block,
                                                               float cz, float ce, const float* __restrict__ gs, float* __restrict__ dz,
                                                               float* __restrict__ ws) {
    constexpr int LD = D + 32, VPR = D / 4, T = D / 32, NT = 2 * D;
    __shared__ __attribute__((aligned(16))) float g_s[32 * LD];  // g of the chunk's rows (zero: past the range, token out of range)
    __shared__ __attribute__((aligned(16))) float c_s[32 * LD];  // c[idx] of the same rows (zero likewise)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    if (gs) { const float sc = *gs; cz *= sc; ce *= sc; }
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r_end = min(n, r_begin + rows_per_block);

    f32x16 acc[T];
#pragma unroll
    for (int jt = 0; jt < T; ++jt) acc[jt] = (f32x16){0};
    float colsum = 0.0f;

    for (int64_t r0 = r_begin; r0 < r_end; r0 += 32) {
        for (int v = tid; v < 32 * VPR; v += NT) {
            const int r = v / VPR, cc = (v - r * VPR) * 4;
            const int64_t row = r0 + r;
            f32x4 gv = {0.f, 0.f, 0.f, 0.f}, cv = {0.f, 0.f, 0.f, 0.f};
            if (row < r_end) {
                const int64_t code = idx[row];
                const bool ok = code >= 0 && code < k;
                const f32x4 zv = *reinterpret_cast<const f32x4*>(z + row * D + cc);
                f32x4 qv = {0.f, 0.f, 0.f, 0.f};
                if (ok) {
                    qv = *reinterpret_cast<const f32x4*>(e + code * D + cc);
                    cv = *reinterpret_cast<const f32x4*>(c + code * D + cc);
                }
                f32x4 up = {0.f, 0.f, 0.f, 0.f};
                if (HAS_DQ) up = SimvqDq<TDQ>::ld4(dq + row * D + cc);
                f32x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    o[q] = __fmaf_rn(cz, zv[q] - qv[q], up[q]);
                    gv[q] = ok ? __fmul_rn(ce, __fsub_rn(qv[q], zv[q])) : 0.0f;
                }
                *reinterpret_cast<f32x4*>(dz + row * D + cc) = o;
            }
            *reinterpret_cast<f32x4*>(g_s + r * LD + cc) = gv;
            *reinterpret_cast<f32x4*>(c_s + r * LD + cc) = cv;
        }
        __syncthreads();
        if (tid < D) {
#pragma unroll 8
            for (int r = 0; r < 32; ++r) colsum = __fadd_rn(colsum, g_s[r * LD + tid]);
        }
        // A[m = i][k = row] = g[row][32 wave + m], B[k = row][n = col] = c_gathered[row][32 jt + n]; two rows per MFMA
#pragma unroll 4
        for (int t = 0; t < 16; ++t) {
            const int ro = (2 * t + half) * LD + j;
            const float av = g_s[ro + 32 * wave];
#pragma unroll
            for (int jt = 0; jt < T; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, c_s[ro + 32 * jt], acc[jt], 0, 0, 0);
        }
        __syncthreads();
    }

    constexpr int64_t SLICE = (int64_t)D * D + D;
    float* out = ws + (int64_t)blockIdx.x * SLICE;
#pragma unroll
    for (int jt = 0; jt < T; ++jt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
            out[i * D + 32 * jt + j] = acc[jt][r];
        }
    }
    if (tid < D) out[D * D + tid] = colsum;
}

// element el of (dw | db): the slices in block order, then one read-modify-write of the target
__global__ __launch_bounds__(256) void simvq_reduce_kernel(const float* __restrict__ ws, int blocks, int d, float* __restrict__ dw,
                                                           float* __restrict__ db) {
    const int dd = d * d, total = dd + d;
    const int el = blockIdx.x * 256 + threadIdx.x;
    if (el >= total) return;
    float s = ws[el];
    for (int b = 1; b < blocks; ++b) s = __fadd_rn(s, ws[(int64_t)b * total + el]);
    if (el < dd) dw[el] = __fadd_rn(dw[el], s);
    else if (db) db[el - dd] = __fadd_rn(db[el - dd], s);
}

// hist[idx[r]] += 1 (integer atomics: any order gives the same counts); a token outside [0, K) counts nowhere
__global__ __launch_bounds__(256) void simvq_hist_kernel(const int64_t* __restrict__ idx, int64_t n, int k, int32_t* __restrict__ hist) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int64_t code = idx[r];
        if (code >= 0 && code < k) atomicAdd(hist + code, 1);
    }
}

}  // namespace

extern "C" {

int vqk_simvq_project_f32(const float* c, const float* w, const float* bias, int k, int d, float* e, void* stream) {
    VQK_REQUIRE(c && w && e, VQK_ERR_ARG);
    VQK_REQUIRE(simvq_d_ok(d) && k > 0 && (k % 32) == 0 && k < (1 << 26), VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(c) && vqk_aligned16(w) && vqk_aligned16(e) && (!bias || vqk_aligned16(bias)), VQK_ERR_ALIGN);
    const int ct = 8192 / d;
    const int tiles = (k + ct - 1) / ct;
    const dim3 grid((unsigned)(tiles < 512 ? tiles : 512));
    hipStream_t st = vqk_stream(stream);
    if (d == 64) hipLaunchKernelGGL(simvq_project_kernel<64>, grid, dim3(128), 0, st, c, w, bias, k, e);
    else if (d == 128) hipLaunchKernelGGL(simvq_project_kernel<128>, grid, dim3(256), 0, st, c, w, bias, k, e);
    else hipLaunchKernelGGL(simvq_project_kernel<256>, grid, dim3(512), 0, st, c, w, bias, k, e);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_simvq_hist_i32(const int64_t* idx, int64_t n, int k, int32_t* hist, void* stream) {
    VQK_REQUIRE(idx && hist, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0, VQK_ERR_SHAPE);
    if (n == 0) return VQK_OK;
    hipLaunchKernelGGL(simvq_hist_kernel, dim3(vqk_grid_1d(n, 256)), dim3(256), 0, vqk_stream(stream), idx, n, k, hist);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int64_t vqk_simvq_backward_ws_bytes(int64_t n, int d) {
    if (n < 0 || n >= ((int64_t)1 << 31) || !simvq_d_ok(d)) return VQK_ERR_SHAPE;
    const int64_t blocks = n > 0 ? simvq_blocks(n) : 1;
    return blocks * ((int64_t)d * d + d) * 4;
}

int vqk_simvq_backward_f32(const float* z, const float* e, const float* c, const int64_t* idx, const void* dq, int dq_dtype, int64_t n,
                           int k, int d, float cz, float ce, const float* gscale_dev, float* dz, float* dw, float* db, void* ws,
                           int64_t ws_bytes, void* stream) {
    VQK_REQUIRE(z && e && c && idx && dz && dw, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && k > 0 && k < (1 << 26) && simvq_d_ok(d), VQK_ERR_SHAPE);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(e) && vqk_aligned16(c) && vqk_aligned16(dz) && vqk_aligned16(ws) &&
                (!dq || (dq_dtype == VQK_F32 ? vqk_aligned16(dq) : (reinterpret_cast<uintptr_t>(dq) & 7u) == 0)), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws && ws_bytes >= vqk_simvq_backward_ws_bytes(n, d), VQK_ERR_WORKSPACE);
    if (n == 0) return VQK_OK;
    const int64_t rpb = simvq_rows_per_block(n);
    const int blocks = (int)simvq_blocks(n);
    hipStream_t st = vqk_stream(stream);
    float* wsf = reinterpret_cast<float*>(ws);
#define SVB_D(DD, T, Q) hipLaunchKernelGGL((simvq_backward_kernel<DD, T, Q>), dim3((unsigned)blocks), dim3(2 * DD), 0, st, z, e, c, idx, \
                                           (const T*)dq, n, k, rpb, cz, ce, gscale_dev, dz, wsf)
#define SVB(T, Q) do { if (d == 64) SVB_D(64, T, Q); else if (d == 128) SVB_D(128, T, Q); else SVB_D(256, T, Q); } while (0)
    if (!dq) SVB(float, false); else if (dq_dtype == VQK_F32) SVB(float, true); else SVB(bf16_raw, true);
#undef SVB
#undef SVB_D
    VQK_CHECK_LAUNCH();
    hipLaunchKernelGGL(simvq_reduce_kernel, dim3((unsigned)((d * d + d + 255) / 256)), dim3(256), 0, st, (const float*)wsf, blocks, d,
                       dw, db);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // extern "C"
