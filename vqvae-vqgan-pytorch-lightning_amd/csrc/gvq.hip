// ------------------------------------------------------------------------------------------------
// Grouped (product / multi-codebook) quantizer: the D channels of a latent row are cut into G contiguous groups of d = D / G
// channels, group g is looked up in its OWN codebook of K codes -- slab g of e[G K][d] -- and the decoder sees the concatenation:
// K^G effective codes from the standard quantizer's K D codebook floats and 2 N K D lookup FLOP.  Per row r and group g
//   idx[r, g] = argmin_k (|z_rg|^2 + |e_gk|^2) - 2 z_rg.e_gk   in the arithmetic of vq.hip::row_sqnorm_kernel / vq_assign_kernel
//               (assoc 0) applied to the contiguous [N, d] slice and the [K, d] slab, first minimum;
//   q[r, g d .. (g + 1) d) = e[g K + idx[r, g]];  sse = sum |q - z|^2;  hist[g K + idx[r, g]] += 1.
//
// FORWARD = one kernel, grid (ceil(N / 32), G).  Block (b, g) stages the columns of group g of its 32 rows (row pitch D, not d) in a
// [32][d + 4] LDS tile, takes |z_rg|^2 there (one wavefront per row, the row_sqnorm bits) and ranks the tile against slab g streamed
// from L2: the MFMA sequence, k order, next-tile prefetch and half-wave / four-wave merge of cos_forward_kernel (vq_cos.hip) without
// its normalisation.  The epilogue gathers e[g K + k] into the strided slot as fp32 and / or bf16, adds |q - z|^2 to the block's
// partial (SSE of vq_lookup.h; deterministic mode: slot g gridDim.x + b of the ordered-sum workspace) and counts hist with the
// duplicates inside the block first.  |e|^2[G K] is an ARGUMENT (vqk_row_sqnorm_f32 over the weight, launched per forward by the
// operator): no prepared workspace, nothing a captured step could see go stale.
//
// BACKWARD works on the FLAT view: z[N][G d] is [N G][d] in memory, flat row f = r G + g carries the global code id
// (f mod G) K + idx[f], and on that view the quantizer is the standard one:  dz = dq + s cz (z - q);
// de[code] += s ce sum_{f: code(f) = code} (e_code - z_f).  Block = 32 flat rows, a wavefront per row, lane = column.  Default: the rows
// of the block that share a global code are chained (CHAINS of vq_lookup.h; the walk is cos_backward_kernel's 64-pitch one without the
// projection) and ONE coalesced fp32 atomic row per distinct (code, block) goes to de.  Deterministic mode: the per-row terms and the
// global ids go to the caller's workspace GROUP-MAJOR ([G][N][d] and [G][N]: a code's block scans the N ids of its own group, not all
// N G) and a second launch, one block per global code, adds its rows in row order (ORDERED SCAN): no float atomics.
// ------------------------------------------------------------------------------------------------
#include "vq_lookup.h"

namespace {

constexpr int GVQ_MAX_GROUPS = 16;

// |row|^2 of one wavefront's row with the bits of vq.hip::row_sqnorm_kernel on a contiguous row of d floats
__device__ __forceinline__ float gvq_row_ss(const float* p, int d, int lane) {
    float acc = 0.0f;
    for (int k = lane; k < d; k += 64) acc = __fmaf_rn(p[k], p[k], acc);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off, 64));
    return acc;
}

template <int D>
__global__ __launch_bounds__(256) void gvq_forward_kernel(const float* __restrict__ z, const float* __restrict__ e_all,
                                                          const float* __restrict__ e2_all, int64_t n, int k, int groups,
                                                          int64_t* __restrict__ idx, float* __restrict__ q32, bf16_raw* __restrict__ q_lo,
                                                          float* __restrict__ sse, float* __restrict__ sse_part,
                                                          int32_t* __restrict__ hist) {
    constexpr int LD = D + 4, VPR = D / 4;
    __shared__ __attribute__((aligned(16))) float zt[32 * LD];  // group g's columns of the block's rows (rows past n: row n - 1)
    __shared__ float z2_s[32];
    __shared__ float red_d[128];
    __shared__ int red_i[128];
    __shared__ int fin[32];
    __shared__ float part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.y;
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    const int64_t pitch = (int64_t)groups * D;
    const float* zg = z + (int64_t)g * D;                        // row r of the slice: zg + r * pitch
    const float* e = e_all + (int64_t)g * k * D;                 // slab g
    const float* e2 = e2_all + (int64_t)g * k;

    for (int v = tid; v < 32 * VPR; v += 256) {
        const int r = v / VPR, c = v - r * VPR;
        int64_t src = n0 + r; if (src >= n) src = n - 1;
        *reinterpret_cast<f32x4*>(zt + r * LD + 4 * c) = *reinterpret_cast<const f32x4*>(zg + src * pitch + 4 * c);
    }
    __syncthreads();
    for (int i = 0; i < 8; ++i) {
        const int r = wave * 8 + i;
        const float ss = gvq_row_ss(zt + r * LD, D, lane);
        if (lane == 0) z2_s[r] = ss;
    }
    __syncthreads();

    // ranking: vq_assign_kernel<0> on (slice, slab) -- A = codes, B = rows; lane (j, half) owns row j and 16 codes of the tile
    const int j = lane & 31, half = lane >> 5;
    const float zz = z2_s[j];
    const float* zb = zt + j * LD + 4 * half;
    const int tiles = k >> 5;
    const int per_wave = (tiles + 3) >> 2;
    const int t_begin = wave * per_wave;
    const int t_end = min(tiles, t_begin + per_wave);
    // the row's fragments are the same for every tile: registers.  The code fragments and |e|^2 of tile t + 1 are loaded before
    // the MFMAs of tile t
    constexpr int NF = D / 8;
    f32x4 b[NF], a_cur[NF], a_nxt[NF], e2_cur[4], e2_nxt[4];
#pragma unroll
    for (int m = 0; m < NF; ++m) b[m] = *reinterpret_cast<const f32x4*>(zb + 8 * m);
    if (t_begin < t_end) {
        const float* ea = e + (int64_t)(t_begin * 32 + j) * D + 4 * half;
#pragma unroll
        for (int m = 0; m < NF; ++m) a_cur[m] = *reinterpret_cast<const f32x4*>(ea + 8 * m);
#pragma unroll
        for (int u = 0; u < 4; ++u) e2_cur[u] = *reinterpret_cast<const f32x4*>(e2 + t_begin * 32 + 8 * u + 4 * half);
    }
    float best = INFINITY;
    int best_i = 0x7fffffff;
    for (int t = t_begin; t < t_end; ++t) {
        if (t + 1 < t_end) {
            const float* ea = e + (int64_t)((t + 1) * 32 + j) * D + 4 * half;
#pragma unroll
            for (int m = 0; m < NF; ++m) a_nxt[m] = *reinterpret_cast<const f32x4*>(ea + 8 * m);
#pragma unroll
            for (int u = 0; u < 4; ++u) e2_nxt[u] = *reinterpret_cast<const f32x4*>(e2 + (t + 1) * 32 + 8 * u + 4 * half);
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
        for (int u = 0; u < 4; ++u) e2_cur[u] = e2_nxt[u];
    }
    // the argmin merge over half-waves and waves stays written out (vq_lookup.h)
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
        if (n0 + tid < n) idx[(n0 + tid) * groups + g] = (int64_t)bi;
    }
    __syncthreads();

    // epilogue: q = e[g K + k] into the group's slot as fp32 and / or bf16, |q - z|^2
    if (q32 || q_lo || sse) {
        float local = 0.0f;
        for (int v = tid; v < 32 * VPR; v += 256) {
            const int r = v / VPR, c = (v - r * VPR) * 4;
            if (n0 + r >= n) continue;
            const f32x4 ev = *reinterpret_cast<const f32x4*>(e + (int64_t)fin[r] * D + c);
            const f32x4 zv = *reinterpret_cast<const f32x4*>(zt + r * LD + c);
            const int64_t o = (n0 + r) * pitch + (int64_t)g * D + c;
            if (q32) *reinterpret_cast<f32x4*>(q32 + o) = ev;
            if (q_lo) {
                const u16x4 ob = {f32_to_bf16(ev[0]), f32_to_bf16(ev[1]), f32_to_bf16(ev[2]), f32_to_bf16(ev[3])};
                *reinterpret_cast<u16x4*>(q_lo + o) = ob;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) { const float u = __fsub_rn(ev[t], zv[t]); local = __fmaf_rn(u, u, local); }
        }
        if (sse) {
            lk_wave_part(local, part, lane, wave);
            __syncthreads();
            if (tid == 0) lk_sse_emit(part, sse, sse_part, (int64_t)g * gridDim.x + blockIdx.x);
        }
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
        if (leader) atomicAdd(hist + (int64_t)g * k + code, count);
    }
}

// block = 32 FLAT rows (flat row f = r G + g: z, dq, dz and idx are [N G][d] / [N G] in memory), wave w: rows 8 w .. 8 w + 7,
// lane = column (d <= 64).  DE: 0 no codebook gradient, 1 LDS chains + atomics, 2 the per-row terms e - z and the global ids to
// the workspace, group-major (deterministic mode).  A token outside [0, K) is a zero code without a gradient.
template <typename TDQ, bool HAS_DQ, int DE>
__global__ __launch_bounds__(256) void gvq_backward_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                           const int64_t* __restrict__ idx, const TDQ* __restrict__ dq, int64_t n,
                                                           int k, int d, int groups, float cz, float ce, const float* __restrict__ gs,
                                                           float* __restrict__ dz, float* __restrict__ de,
                                                           float* __restrict__ contrib, int64_t* __restrict__ gid) {
    __shared__ float tile[DE == 1 ? 32 * 64 : 1];                // e - z of the block's rows
    __shared__ int code_s[32], next_s[32], first_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nf = n * groups;
    const int64_t f0 = (int64_t)blockIdx.x * 32;
    if (gs) { const float sc = *gs; cz *= sc; ce *= sc; }
    const bool on = lane < d;
    if (tid < 32) {
        const int64_t f = f0 + tid;
        int code = -1;
        if (f < nf) {
            const int64_t c = idx[f];
            const int g = (int)(f % groups);
            if (c >= 0 && c < k) code = g * k + (int)c;
            if (DE == 2) gid[(int64_t)g * n + f / groups] = code;
        }
        code_s[tid] = code;
    }
    __syncthreads();
    for (int i = 0; i < 8; ++i) {
        const int r = wave * 8 + i;
        const int64_t f = f0 + r;
        if (f >= nf) break;                                      // wave-uniform
        const int code = code_s[r];
        const float qv = (on && code >= 0) ? e[(int64_t)code * d + lane] : 0.0f;
        const float zv = on ? z[f * d + lane] : 0.0f;
        float g = 0.0f;
        if (HAS_DQ && on) g = Elem<TDQ>::ld(dq + f * d + lane);
        if (on) dz[f * d + lane] = __fmaf_rn(cz, zv - qv, g);
        const float term = code >= 0 ? qv - zv : 0.0f;
        if (DE == 1) tile[r * 64 + lane] = term;
        if (DE == 2 && on) contrib[((f % groups) * n + f / groups) * d + lane] = term;
    }
    if constexpr (DE == 1) {
        __syncthreads();
        if (tid < 32) lk_build_chains(code_s, first_s, next_s, tid);
        __syncthreads();
        // wave w: heads w, w + 4, ...; ONE coalesced fp32 atomic row per distinct global code of the block
        for (int r = wave; r < 32; r += 4) {
            const int code = code_s[r];
            if (code < 0 || first_s[r] != r) continue;           // wave-uniform
            float s = 0.0f;
            for (int m = r; m >= 0; m = next_s[m]) s += tile[m * 64 + lane];
            if (on) atomicAdd(de + (int64_t)code * d + lane, ce * s);
        }
    }
}

// Deterministic codebook gradient: block = global code (g, k); it scans the N ids of group g in chunks of 256 and thread c < d adds
// column c of the matching rows of contrib[g], lowest row first.
__global__ __launch_bounds__(256) void gvq_code_grad_ordered_kernel(const float* __restrict__ contrib, const int64_t* __restrict__ gid,
                                                                    int64_t n, int k, int d, float ce, const float* __restrict__ gs,
                                                                    float* __restrict__ de) {
    __shared__ unsigned long long masks[4];
    const int64_t code = blockIdx.x;
    const int64_t g = code / k;
    const int tid = threadIdx.x;
    if (gs) ce *= *gs;
    const float* cg = contrib + g * n * d;
    float acc = 0.f;
    lk_ordered_scan(gid + g * n, n, code, masks, tid < d, [&](int64_t r) { acc += cg[r * d + tid]; });
    if (tid < d) de[code * d + tid] += ce * acc;
}

// tokens [N][G] -> q [N][G d]: one thread per (flat row, four columns); a token outside [0, K) gives a zero slice
__global__ __launch_bounds__(256) void gvq_decode_kernel(const int64_t* __restrict__ idx, const float* __restrict__ e, int64_t nf, int k,
                                                         int d, int groups, float* __restrict__ q32, bf16_raw* __restrict__ q_lo) {
    const int d4 = d >> 2;
    const int64_t total = nf * d4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t f = i / d4;
        const int c = (int)(i - f * d4) * 4;
        const int64_t code = idx[f];
        f32x4 ev = {0.f, 0.f, 0.f, 0.f};
        if (code >= 0 && code < k) ev = *reinterpret_cast<const f32x4*>(e + ((f % groups) * k + code) * d + c);
        if (q32) *reinterpret_cast<f32x4*>(q32 + f * d + c) = ev;
        if (q_lo) {
            const u16x4 ob = {f32_to_bf16(ev[0]), f32_to_bf16(ev[1]), f32_to_bf16(ev[2]), f32_to_bf16(ev[3])};
            *reinterpret_cast<u16x4*>(q_lo + f * d + c) = ob;
        }
    }
}

static inline bool gvq_fused_d(int d) { return d == 8 || d == 16 || d == 32 || d == 64; }
static inline bool gvq_groups_ok(int groups) { return groups >= 1 && groups <= GVQ_MAX_GROUPS; }
// K per group; G K global ids fit an int with room to spare, N G flat rows a grid of 32-row blocks
static inline bool gvq_sizes_ok(int64_t n, int k) { return n >= 0 && n < ((int64_t)1 << 31) && k > 0 && k < (1 << 22); }
static inline int64_t gvq_contrib_bytes(int64_t n, int d, int groups) { return (n > 0 ? n : 1) * (int64_t)groups * d * 4; }

}  // namespace

extern "C" {

int vqk_gvq_forward_f32(const float* z, const float* e, const float* e2, int64_t n, int k, int d, int groups, int64_t* idx, float* q,
                        void* q_lo, float* sse, int32_t* hist, void* stream) {
    VQK_REQUIRE(z && e && e2 && idx, VQK_ERR_ARG);
    VQK_REQUIRE(gvq_sizes_ok(n, k) && (k % 32) == 0 && gvq_fused_d(d) && gvq_groups_ok(groups), VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(e) && vqk_aligned16(e2) && (!q || vqk_aligned16(q)) &&
                (!q_lo || (reinterpret_cast<uintptr_t>(q_lo) & 7u) == 0), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)groups);
    const int64_t slots = (int64_t)grid.x * groups;
    hipStream_t st = vqk_stream(stream);
    LK_SSE_PART(sse_part, sse, slots)
#define GVQ_LAUNCH(DD) hipLaunchKernelGGL((gvq_forward_kernel<DD>), grid, dim3(256), 0, st, z, e, e2, n, k, groups, idx, q, \
                                          reinterpret_cast<bf16_raw*>(q_lo), sse, sse_part, hist)
    if (d == 8) GVQ_LAUNCH(8); else if (d == 16) GVQ_LAUNCH(16); else if (d == 32) GVQ_LAUNCH(32); else GVQ_LAUNCH(64);
#undef GVQ_LAUNCH
    VQK_CHECK_LAUNCH();
    if (sse_part) {
        hipLaunchKernelGGL(lk_sse_ordered_kernel<float>, dim3(1), dim3(64), 0, st, (const float*)sse_part, (int)slots, 1, sse);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

int vqk_gvq_decode_f32(const int64_t* idx, const float* e, int64_t n, int k, int d, int groups, float* q, void* q_lo, void* stream) {
    VQK_REQUIRE(idx && e && (q || q_lo), VQK_ERR_ARG);
    VQK_REQUIRE(gvq_sizes_ok(n, k) && d > 0 && (d % 4) == 0 && gvq_groups_ok(groups), VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(e) && (!q || vqk_aligned16(q)) && (!q_lo || (reinterpret_cast<uintptr_t>(q_lo) & 7u) == 0), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    const int64_t nf = n * groups;
    hipLaunchKernelGGL(gvq_decode_kernel, dim3(vqk_grid_1d(nf * (d / 4), 256)), dim3(256), 0, vqk_stream(stream), idx, e, nf, k, d, groups,
                       q, reinterpret_cast<bf16_raw*>(q_lo));
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int64_t vqk_gvq_backward_ws_bytes(int64_t n, int d, int groups) {
    if (n < 0 || n >= ((int64_t)1 << 31) || !gvq_fused_d(d) || !gvq_groups_ok(groups)) return VQK_ERR_SHAPE;
    return gvq_contrib_bytes(n, d, groups) + (n > 0 ? n : 1) * (int64_t)groups * 8;
}

int vqk_gvq_backward_f32(const float* z, const float* e, const int64_t* idx, const void* dq, int dq_dtype, int64_t n, int k, int d,
                         int groups, float cz, float ce, const float* gscale_dev, float* dz, float* de, void* ws, int64_t ws_bytes,
                         void* stream) {
    VQK_REQUIRE(z && e && idx && dz, VQK_ERR_ARG);
    VQK_REQUIRE(gvq_sizes_ok(n, k) && gvq_fused_d(d) && gvq_groups_ok(groups), VQK_ERR_SHAPE);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    const bool ordered = de && vqkd::det_state().on;             // the per-row terms and ids go through ws
    if (ordered) {
        VQK_REQUIRE(ws && ws_bytes >= vqk_gvq_backward_ws_bytes(n, d, groups), VQK_ERR_WORKSPACE);
        VQK_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, VQK_ERR_ALIGN);
    }
    if (n == 0) return VQK_OK;
    const int64_t nf = n * groups;
    const dim3 grid((unsigned)((nf + 31) / 32));
    hipStream_t st = vqk_stream(stream);
    float* contrib = ordered ? reinterpret_cast<float*>(ws) : nullptr;
    int64_t* gid = ordered ? reinterpret_cast<int64_t*>(reinterpret_cast<char*>(ws) + gvq_contrib_bytes(n, d, groups)) : nullptr;
#define GVB(T, Q, E) hipLaunchKernelGGL((gvq_backward_kernel<T, Q, E>), grid, dim3(256), 0, st, z, e, idx, (const T*)dq, n, k, d, groups, \
                                       cz, ce, gscale_dev, dz, de, contrib, gid)
    LK_DISPATCH_DQ_DE(GVB, dq, dq_dtype, !de ? 0 : !ordered ? 1 : 2);
#undef GVB
    VQK_CHECK_LAUNCH();
    if (ordered) {
        hipLaunchKernelGGL(gvq_code_grad_ordered_kernel, dim3((unsigned)(groups * k)), dim3(256), 0, st, (const float*)contrib,
                           (const int64_t*)gid, n, k, d, ce, gscale_dev, de);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

}  // extern "C"
