// Self-attention core o = softmax(scale Q K^T) V and its backward (include/vqk.h: vqk_attn_fwd / vqk_attn_bwd).
//
// Operands are [B][N][ld] rows with the head's d channels at column head * d; every operand has its own row stride ld, so the
// three slices of one [B][N][3C] tensor are read in place.  One workgroup = 4 waves = one 64-row tile of one (batch, head):
//   forward : owns 64 queries, walks the keys in tiles of 64 (online softmax, running maximum; m, l, lse in fp32)
//   dK / dV : owns 64 keys, walks the queries      (S^T and dP^T with the key on the tile row: dV = P^T dO, dK = dS^T Q)
//   dQ      : owns 64 queries, walks the keys      (dQ = dS K)
// so every output element is summed by ONE workgroup in a fixed order: no atomics, the same bits on every run.
// The head dimension is walked in 64-wide chunks through LDS; each wave owns one 32x32 tile of every 64x64 product, and the
// output accumulators (D / 64 tiles per wave and output) stay in registers over the whole walk.
// fp32 storage: exact fp32 products on v_mfma_f32_32x32x2_f32; bf16 storage: v_mfma_f32_32x32x16_bf16, fp32 accumulation, P and
// dS rounded to bf16 only as MFMA operands.  A [k][col] operand (V, dO, Q, K of the second products) is read by columns in fp32
// and staged transposed in bf16, so the bf16 form only ever reads [row][k] fragments.
// The tile helpers (tile size AT, LDS pitch, accumulator layout, global -> register -> LDS staging, the two MFMA products) are
// mfma_tile.h's, shared with ibq.hip.
#include "common.h"
#include "mfma_tile.h"

#include <math.h>

namespace {

constexpr int SLD = 68;          // fp32 logit tile pitch

struct AttnArgs {
    const void *q, *k, *v, *o, *dout;
    void *out, *dq, *dk, *dv;
    float* lse;
    float* delta;
    int n, heads;
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    float scale;
};

template <typename T> __device__ __forceinline__ const T* head_base(const void* p, int64_t ld, int n, int d) {
    return reinterpret_cast<const T*>(p) + (int64_t)blockIdx.z * n * ld + (int64_t)blockIdx.y * d;
}

template <typename T> constexpr int fwd_lds() { return 4 * AT * Pitch<T>::LD * (int)sizeof(T) + AT * SLD * 4 + (sizeof(T) == 2 ? AT * Pitch<T>::LD * 2 : 0) + AT * 4; }
template <typename T> constexpr int dkv_lds() { return 6 * AT * Pitch<T>::LD * (int)sizeof(T); }
template <typename T> constexpr int dq_lds() { return 5 * AT * Pitch<T>::LD * (int)sizeof(T); }

// ------------------------------------------------------------------------------------------------
// forward.  grid (ceil(n / 64), heads, B)
// ------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const AttnArgs a) {
    constexpr int LD = Pitch<T>::LD, NC = D / AT, TB = AT * LD;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* buf = reinterpret_cast<T*>(smem);                         // 4 operand tiles
    float* sS = reinterpret_cast<float*>(buf + 4 * TB);          // scaled logits [64][SLD]
    T* sP = sizeof(T) == 2 ? reinterpret_cast<T*>(sS + AT * SLD) : reinterpret_cast<T*>(sS);     // fp32: P over its own logits
    float* sRow = reinterpret_cast<float*>(smem + fwd_lds<T>() - AT * 4);                        // alpha, finally 1 / l
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rh = wave >> 1, ch = wave & 1;
    const int n = a.n, q0 = blockIdx.x * AT;
    const T* qb = head_base<T>(a.q, a.ldq, n, D);
    const T* kb = head_base<T>(a.k, a.ldk, n, D);
    const T* vb = head_base<T>(a.v, a.ldv, n, D);
    const int srow = tid >> 2, part = tid & 3;                   // softmax: 4 threads per query row, 16 keys each

    f32x16 oacc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc_zero(oacc[c]);
    float m = -INFINITY, l = 0.0f;                               // the same in the 4 threads of a row

    TileRegs<T> ra, rb;                                          // the next step's tiles, in flight
    gload<T>(ra, qb, a.ldq, q0, n, 0);
    gload<T>(rb, kb, a.ldk, 0, n, 0);
    for (int k0 = 0; k0 < n; k0 += AT) {
        f32x16 s;
        acc_zero(s);
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // S = Q K^T, chunk c in tile pair c & 1
            T* bq = buf + (2 * (c & 1)) * TB;
            T* bk = bq + TB;
            lstore<T>(bq, ra);
            lstore<T>(bk, rb);
            if (c + 1 < NC) {
                gload<T>(ra, qb, a.ldq, q0, n, (c + 1) * AT);
                gload<T>(rb, kb, a.ldk, k0, n, (c + 1) * AT);
            } else {
                gload_b(ra, vb, a.ldv, k0, n, 0);
            }
            __syncthreads();
            mma_nt(s, bq + rh * 32 * LD, bk + ch * 32 * LD, lane);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sS[(rh * 32 + acc_row(r, lane)) * SLD + ch * 32 + (lane & 31)] = s[r] * a.scale;
        __syncthreads();
        {
            float x[16];
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                x[j] = (k0 + part * 16 + j < n) ? sS[srow * SLD + part * 16 + j] : -INFINITY;
                mx = fmaxf(mx, x[j]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            const float mn = fmaxf(m, mx);                       // finite: key k0 is always valid
            const float alpha = expf(m - mn);
            float sum = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float p = (k0 + part * 16 + j < n) ? expf(x[j] - mn) : 0.0f;      // tail keys: exactly zero weight
                sum += p;
                Elem<T>::st(sP + srow * LD + part * 16 + j, p);
            }
            sum += __shfl_xor(sum, 1, 64);
            sum += __shfl_xor(sum, 2, 64);
            l = l * alpha + sum;
            m = mn;
            if (part == 0) sRow[srow] = alpha;
        }
        __syncthreads();
        float al[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) al[r] = sRow[rh * 32 + acc_row(r, lane)];
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // O = alpha O + P V, chunk c in tile 2 + (c & 1)
            T* bv = buf + (2 + (c & 1)) * TB;
            lstore_b(bv, ra);
            if (c + 1 < NC) {
                gload_b(ra, vb, a.ldv, k0, n, (c + 1) * AT);
            } else if (k0 + AT < n) {
                gload<T>(ra, qb, a.ldq, q0, n, 0);
                gload<T>(rb, kb, a.ldk, k0 + AT, n, 0);
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[c][r] *= al[r];
            mma_ab(oacc[c], sP + rh * 32 * LD, bv, ch * 32, lane);
        }
        __syncthreads();                                         // P, alpha and the tiles are free again
    }
    if (part == 0) {
        sRow[srow] = 1.0f / l;
        if (q0 + srow < n) a.lse[((int64_t)blockIdx.z * a.heads + blockIdx.y) * n + q0 + srow] = m + logf(l);
    }
    __syncthreads();
    T* ob = reinterpret_cast<T*>(a.out) + (int64_t)blockIdx.z * n * a.ldo + (int64_t)blockIdx.y * D;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = rh * 32 + acc_row(r, lane);
        if (q0 + row < n) {
            const float li = sRow[row];
#pragma unroll
            for (int c = 0; c < NC; ++c) Elem<T>::st(ob + (int64_t)(q0 + row) * a.ldo + c * AT + ch * 32 + (lane & 31), oacc[c][r] * li);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// delta[b][h][i] = sum_c do[b][i][h d + c] o[b][i][h d + c]: one wave per row, a fixed order.  grid (ceil(n / 4), heads, B)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void attn_delta_kernel(const AttnArgs a, int d) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const T* o = head_base<T>(a.o, a.ldo, a.n, d) + (int64_t)i * a.ldo;
    const T* g = head_base<T>(a.dout, a.lddo, a.n, d) + (int64_t)i * a.lddo;
    float s = 0.0f;
    for (int c = lane; c < d; c += 64) s += Elem<T>::ld(o + c) * Elem<T>::ld(g + c);
    s = wave_sum(s);
    if (lane == 0) a.delta[((int64_t)blockIdx.z * a.heads + blockIdx.y) * a.n + i] = s;
}

// ------------------------------------------------------------------------------------------------
// dK, dV.  grid (ceil(n / 64), heads, B): the workgroup owns 64 keys; tiles are [key][query]
// ------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_dkv_kernel(const AttnArgs a) {
    constexpr int LD = Pitch<T>::LD, NC = D / AT, TB = AT * LD;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* buf = reinterpret_cast<T*>(smem);
    T* sPT = buf + 4 * TB;                                        // P^T  [key][query]
    T* sDT = buf + 5 * TB;                                        // dS^T [key][query]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rh = wave >> 1, ch = wave & 1;
    const int n = a.n, k0 = blockIdx.x * AT;
    const T* qb = head_base<T>(a.q, a.ldq, n, D);
    const T* kb = head_base<T>(a.k, a.ldk, n, D);
    const T* vb = head_base<T>(a.v, a.ldv, n, D);
    const T* gb = head_base<T>(a.dout, a.lddo, n, D);
    const float* lse = a.lse + ((int64_t)blockIdx.z * a.heads + blockIdx.y) * n;
    const float* delta = a.delta + ((int64_t)blockIdx.z * a.heads + blockIdx.y) * n;

    f32x16 dk[NC], dv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { acc_zero(dk[c]); acc_zero(dv[c]); }

    TileRegs<T> ra, rb;
    gload<T>(ra, kb, a.ldk, k0, n, 0);
    gload<T>(rb, qb, a.ldq, 0, n, 0);
    for (int q0 = 0; q0 < n; q0 += AT) {
        f32x16 st, dpt;
        acc_zero(st);
        acc_zero(dpt);
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // S^T = K Q^T in tiles 0, 1; dP^T = V dO^T in tiles 2, 3
            lstore<T>(buf, ra);
            lstore<T>(buf + TB, rb);
            gload<T>(ra, vb, a.ldv, k0, n, c * AT);
            gload<T>(rb, gb, a.lddo, q0, n, c * AT);
            __syncthreads();
            mma_nt(st, buf + rh * 32 * LD, buf + TB + ch * 32 * LD, lane);
            lstore<T>(buf + 2 * TB, ra);
            lstore<T>(buf + 3 * TB, rb);
            if (c + 1 < NC) {
                gload<T>(ra, kb, a.ldk, k0, n, (c + 1) * AT);
                gload<T>(rb, qb, a.ldq, q0, n, (c + 1) * AT);
            } else {
                gload_b(ra, gb, a.lddo, q0, n, 0);
                gload_b(rb, qb, a.ldq, q0, n, 0);
            }
            __syncthreads();
            mma_nt(dpt, buf + 2 * TB + rh * 32 * LD, buf + 3 * TB + ch * 32 * LD, lane);
        }
        const int qi = q0 + ch * 32 + (lane & 31);
        const bool qok = qi < n;
        const float ls = qok ? lse[qi] : 0.0f, dl = qok ? delta[qi] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rh * 32 + acc_row(r, lane);
            const float p = (qok && k0 + row < n) ? expf(st[r] * a.scale - ls) : 0.0f;
            Elem<T>::st(sPT + row * LD + ch * 32 + (lane & 31), p);
            Elem<T>::st(sDT + row * LD + ch * 32 + (lane & 31), p * (dpt[r] - dl));
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // dV += P^T dO, dK += dS^T Q, chunk c in tile pair c & 1
            T* bg = buf + (2 * (c & 1)) * TB;
            T* bq = bg + TB;
            lstore_b(bg, ra);
            lstore_b(bq, rb);
            if (c + 1 < NC) {
                gload_b(ra, gb, a.lddo, q0, n, (c + 1) * AT);
                gload_b(rb, qb, a.ldq, q0, n, (c + 1) * AT);
            } else if (q0 + AT < n) {
                gload<T>(ra, kb, a.ldk, k0, n, 0);
                gload<T>(rb, qb, a.ldq, q0 + AT, n, 0);
            }
            __syncthreads();                                     // (chunk 0: P^T and dS^T are in LDS as well)
            mma_ab(dv[c], sPT + rh * 32 * LD, bg, ch * 32, lane);
            mma_ab(dk[c], sDT + rh * 32 * LD, bq, ch * 32, lane);
        }
        __syncthreads();
    }
    T* dkb = reinterpret_cast<T*>(a.dk) + (int64_t)blockIdx.z * n * a.lddk + (int64_t)blockIdx.y * D;
    T* dvb = reinterpret_cast<T*>(a.dv) + (int64_t)blockIdx.z * n * a.lddv + (int64_t)blockIdx.y * D;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = k0 + rh * 32 + acc_row(r, lane);
        if (row < n) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int col = c * AT + ch * 32 + (lane & 31);
                Elem<T>::st(dkb + (int64_t)row * a.lddk + col, dk[c][r] * a.scale);
                Elem<T>::st(dvb + (int64_t)row * a.lddv + col, dv[c][r]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dQ.  grid (ceil(n / 64), heads, B): the workgroup owns 64 queries; tiles are [query][key]
// ------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_dq_kernel(const AttnArgs a) {
    constexpr int LD = Pitch<T>::LD, NC = D / AT, TB = AT * LD;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* buf = reinterpret_cast<T*>(smem);
    T* sDS = buf + 4 * TB;                                        // dS [query][key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rh = wave >> 1, ch = wave & 1;
    const int n = a.n, q0 = blockIdx.x * AT;
    const T* qb = head_base<T>(a.q, a.ldq, n, D);
    const T* kb = head_base<T>(a.k, a.ldk, n, D);
    const T* vb = head_base<T>(a.v, a.ldv, n, D);
    const T* gb = head_base<T>(a.dout, a.lddo, n, D);
    const float* lse = a.lse + ((int64_t)blockIdx.z * a.heads + blockIdx.y) * n;
    const float* delta = a.delta + ((int64_t)blockIdx.z * a.heads + blockIdx.y) * n;

    float ls[16], dl[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qi = q0 + rh * 32 + acc_row(r, lane);
        ls[r] = qi < n ? lse[qi] : 0.0f;
        dl[r] = qi < n ? delta[qi] : 0.0f;
    }
    f32x16 dq[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc_zero(dq[c]);

    TileRegs<T> ra, rb;
    gload<T>(ra, qb, a.ldq, q0, n, 0);
    gload<T>(rb, kb, a.ldk, 0, n, 0);
    for (int k0 = 0; k0 < n; k0 += AT) {
        f32x16 s, dp;
        acc_zero(s);
        acc_zero(dp);
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // S = Q K^T in tiles 0, 1; dP = dO V^T in tiles 2, 3
            lstore<T>(buf, ra);
            lstore<T>(buf + TB, rb);
            gload<T>(ra, gb, a.lddo, q0, n, c * AT);
            gload<T>(rb, vb, a.ldv, k0, n, c * AT);
            __syncthreads();
            mma_nt(s, buf + rh * 32 * LD, buf + TB + ch * 32 * LD, lane);
            lstore<T>(buf + 2 * TB, ra);
            lstore<T>(buf + 3 * TB, rb);
            if (c + 1 < NC) {
                gload<T>(ra, qb, a.ldq, q0, n, (c + 1) * AT);
                gload<T>(rb, kb, a.ldk, k0, n, (c + 1) * AT);
            } else {
                gload_b(ra, kb, a.ldk, k0, n, 0);
            }
            __syncthreads();
            mma_nt(dp, buf + 2 * TB + rh * 32 * LD, buf + 3 * TB + ch * 32 * LD, lane);
        }
        const bool kok = k0 + ch * 32 + (lane & 31) < n;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rh * 32 + acc_row(r, lane);
            const float p = (kok && q0 + row < n) ? expf(s[r] * a.scale - ls[r]) : 0.0f;
            Elem<T>::st(sDS + row * LD + ch * 32 + (lane & 31), p * (dp[r] - dl[r]));
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {                           // dQ += dS K, chunk c in tile c & 1
            T* bk = buf + (c & 1) * TB;
            lstore_b(bk, ra);
            if (c + 1 < NC) {
                gload_b(ra, kb, a.ldk, k0, n, (c + 1) * AT);
            } else if (k0 + AT < n) {
                gload<T>(ra, qb, a.ldq, q0, n, 0);
                gload<T>(rb, kb, a.ldk, k0 + AT, n, 0);
            }
            __syncthreads();                                     // (chunk 0: dS is in LDS as well)
            mma_ab(dq[c], sDS + rh * 32 * LD, bk, ch * 32, lane);
        }
        __syncthreads();
    }
    T* dqb = reinterpret_cast<T*>(a.dq) + (int64_t)blockIdx.z * n * a.lddq + (int64_t)blockIdx.y * D;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = q0 + rh * 32 + acc_row(r, lane);
        if (row < n) {
#pragma unroll
            for (int c = 0; c < NC; ++c) Elem<T>::st(dqb + (int64_t)row * a.lddq + c * AT + ch * 32 + (lane & 31), dq[c][r] * a.scale);
        }
    }
}

template <typename T, int D> int launch_fwd(const AttnArgs& a, dim3 grid, hipStream_t st) {
    static const hipError_t attr = hipFuncSetAttribute((const void*)attn_fwd_kernel<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       fwd_lds<T>());
    if (attr != hipSuccess) return VQK_ERR_LAUNCH;
    hipLaunchKernelGGL((attn_fwd_kernel<T, D>), grid, dim3(256), fwd_lds<T>(), st, a);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}
template <typename T, int D> int launch_bwd(const AttnArgs& a, dim3 grid, hipStream_t st) {
    static const hipError_t attr1 = hipFuncSetAttribute((const void*)attn_dkv_kernel<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        dkv_lds<T>());
    static const hipError_t attr2 = hipFuncSetAttribute((const void*)attn_dq_kernel<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        dq_lds<T>());
    if (attr1 != hipSuccess || attr2 != hipSuccess) return VQK_ERR_LAUNCH;
    hipLaunchKernelGGL((attn_delta_kernel<T>), dim3((unsigned)((a.n + 3) / 4), grid.y, grid.z), dim3(256), 0, st, a, D);
    hipLaunchKernelGGL((attn_dkv_kernel<T, D>), grid, dim3(256), dkv_lds<T>(), st, a);
    hipLaunchKernelGGL((attn_dq_kernel<T, D>), grid, dim3(256), dq_lds<T>(), st, a);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

template <typename T> int dispatch(bool bwd, const AttnArgs& a, int d, dim3 grid, hipStream_t st) {
    switch (d) {
        case 64: return bwd ? launch_bwd<T, 64>(a, grid, st) : launch_fwd<T, 64>(a, grid, st);
        case 128: return bwd ? launch_bwd<T, 128>(a, grid, st) : launch_fwd<T, 128>(a, grid, st);
        case 256: return bwd ? launch_bwd<T, 256>(a, grid, st) : launch_fwd<T, 256>(a, grid, st);
        case 512: return bwd ? launch_bwd<T, 512>(a, grid, st) : launch_fwd<T, 512>(a, grid, st);
    }
    return VQK_ERR_SHAPE;
}

int check_shape(int dtype, int b, int n, int heads, int d) {
    VQK_REQUIRE(dtype == VQK_F32 || dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(b > 0 && n > 0 && heads > 0 && b <= 65535 && heads <= 65535, VQK_ERR_SHAPE);
    VQK_REQUIRE(d == 64 || d == 128 || d == 256 || d == 512, VQK_ERR_SHAPE);
    return VQK_OK;
}
bool stride_ok(int dtype, int64_t ld, int heads, int d) {
    const int64_t es = dtype == VQK_BF16 ? 2 : 4;
    return ld >= (int64_t)heads * d && (ld * es) % 16 == 0;
}

}  // namespace

extern "C" int vqk_attn_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int b, int n, int heads, int d,
                            int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, void* stream) {
    const int rc = check_shape(dtype, b, n, heads, d);
    if (rc != VQK_OK) return rc;
    VQK_REQUIRE(q && k && v && o && lse, VQK_ERR_ARG);
    VQK_REQUIRE(stride_ok(dtype, ldq, heads, d) && stride_ok(dtype, ldk, heads, d) && stride_ok(dtype, ldv, heads, d) &&
                    stride_ok(dtype, ldo, heads, d), VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(q) && vqk_aligned16(k) && vqk_aligned16(v) && vqk_aligned16(o), VQK_ERR_ALIGN);
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v; a.out = o; a.lse = lse; a.n = n; a.heads = heads;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.scale = scale;
    const dim3 grid((unsigned)((n + AT - 1) / AT), (unsigned)heads, (unsigned)b);
    return dtype == VQK_BF16 ? dispatch<bf16_raw>(false, a, d, grid, vqk_stream(stream)) : dispatch<float>(false, a, d, grid, vqk_stream(stream));
}

extern "C" int vqk_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const float* lse, const void* dout,
                            void* dq, void* dk, void* dv, float* delta, int b, int n, int heads, int d, int64_t ldq, int64_t ldk,
                            int64_t ldv, int64_t ldo, int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, float scale, void* stream) {
    const int rc = check_shape(dtype, b, n, heads, d);
    if (rc != VQK_OK) return rc;
    VQK_REQUIRE(q && k && v && o && lse && dout && dq && dk && dv && delta, VQK_ERR_ARG);
    VQK_REQUIRE(stride_ok(dtype, ldq, heads, d) && stride_ok(dtype, ldk, heads, d) && stride_ok(dtype, ldv, heads, d) &&
                    stride_ok(dtype, ldo, heads, d) && stride_ok(dtype, lddo, heads, d) && stride_ok(dtype, lddq, heads, d) &&
                    stride_ok(dtype, lddk, heads, d) && stride_ok(dtype, lddv, heads, d), VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(q) && vqk_aligned16(k) && vqk_aligned16(v) && vqk_aligned16(o) && vqk_aligned16(dout) && vqk_aligned16(dq) &&
                    vqk_aligned16(dk) && vqk_aligned16(dv), VQK_ERR_ALIGN);
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout; a.dq = dq; a.dk = dk; a.dv = dv;
    a.lse = const_cast<float*>(lse); a.delta = delta; a.n = n; a.heads = heads;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.lddo = lddo; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv; a.scale = scale;
    const dim3 grid((unsigned)((n + AT - 1) / AT), (unsigned)heads, (unsigned)b);
    return dtype == VQK_BF16 ? dispatch<bf16_raw>(true, a, d, grid, vqk_stream(stream)) : dispatch<float>(true, a, d, grid, vqk_stream(stream));
}
