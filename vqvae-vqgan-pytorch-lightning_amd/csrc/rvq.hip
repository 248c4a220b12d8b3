// ------------------------------------------------------------------------------------------------
// Residual quantizer (Lee et al. 2022, RQ-VAE; Zeghidour et al. 2021, SoundStream): every latent row is approximated by the sum
// of `depth` codes of ONE shared codebook, stage q quantizing what the stages before it left over.
//   r_0 = z;  k_q = argmin_k (|r_{q-1}|^2 + |e_k|^2) - 2 r_{q-1}.e_k  (the standard quantizer's arithmetic, first minimum wins);
//   r_q = r_{q-1} - e[k_q]  (one fp32 subtraction per element);  zhat = ((e[k_1] + e[k_2]) + ...) + e[k_Q]  (stage order).
//
// FORWARD = one kernel: a block owns 32 rows for ALL stages.  The residual tile stays in LDS where vqf_rank (vq_filter.h: the
// standard forward's |r|^2, bf16 filter passes, exact re-rank and overflow fallback, unchanged) ranks it once per stage; the
// stage epilogue gathers e[k_q], adds it into the running zhat (a second LDS tile), subtracts it from the residual tile, adds
// |r_q|^2 to the block's partial of sse[q] (one atomic per block and stage at the end; deterministic mode: the partials go through
// the ordered-sum workspace and a second, one-wave launch adds them in block order) and counts hist[q][k_q].  The barrier that orders a stage's tile write before the next
// stage's reads is vqf_rank's first one.  The error-bound argument of vq_filter.hip holds for any input row, so for residuals;
// everything derived from the codebook (vqk_vq_prepare_f32's workspace) is shared by the stages.
// Each stage evaluates the fp32 expression sequence of vqk_vq_forward_f32 on the materialised residual followed by an fp32
// subtraction and addition: the kernel equals that staged formulation bit for bit.
//
// DECODE adds the gathered rows with the forward's accumulation function (lk_accum): the same bits of zhat for the same tokens.
//
// BACKWARD recomputes the residuals from z, e and idx by the same running subtraction (the same bits; nothing is saved):
//   dz = dq + s cz sum_q r_q (stage order);   de[k] += -s ce sum_{(row, q): k_q = k} r_q.
// Default: per stage, the rows of a 32-row block that share a code are summed through an LDS tile, one coalesced fp32 atomic row
// per distinct (code, block) -- CHAINS of vq_lookup.h.  Deterministic mode: the residual stack R[N * depth][256] is materialised
// in the workspace and one block per code adds its rows of R in (row, stage) order -- ORDERED SCAN of vq_lookup.h; no atomics,
// the same bits every run.  The block partials of sse, their ordered sum and the decode kernel are that header's too.
// ------------------------------------------------------------------------------------------------
#include "vq_filter.h"

namespace {

constexpr int RVQ_MAX_DEPTH = 8;

__device__ __forceinline__ f32x4 rvq_sub(const f32x4 r, const f32x4 ev) {
    f32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = __fsub_rn(r[t], ev[t]);
    return o;
}

// Dynamic LDS: 68 KiB = the residual tile and the zhat tile, [32][FD + 4] floats each.
template <int CT>
__global__ __launch_bounds__(256, 1) void rvq_forward_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                             const bf16_raw* __restrict__ eb, const float* __restrict__ e2,
                                                             const float* __restrict__ eps_e, const float* __restrict__ e2max,
                                                             int64_t n, int k, int depth, int64_t* __restrict__ idx,
                                                             float* __restrict__ q32, bf16_raw* __restrict__ q_lo,
                                                             float* __restrict__ sse, float* __restrict__ sse_part,
                                                             int32_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ZLD = FD + 4;
    float* rt = reinterpret_cast<float*>(smem);                  // [32][FD + 4]: the running residual (rows past n: row n - 1, never updated)
    float* qt = rt + 32 * ZLD;                                   // [32][FD + 4]: the running zhat
    __shared__ VqfLds s;
    __shared__ float sse_s[RVQ_MAX_DEPTH][4];
    const int tid_blk = threadIdx.x;
    const int64_t n0_blk = (int64_t)blockIdx.x * 32;
    const bool want_q = q32 || q_lo;
    vqf_load_rows(z, n0_blk, n, rt);
    for (int q = 0; q < depth; ++q) {
        // K, the block's first row and the thread index are made opaque per stage: what depends on them alone (the predicates of the
        // tile walk, per-thread addresses and predicates) is then recomputed by every stage instead of being hoisted out of the
        // stage loop and kept in registers across the ranking, where it spilled at CT = 8
        int kq = k, tid = tid_blk;
        int64_t n0 = n0_blk;
        asm volatile("" : "+s"(kq), "+s"(n0), "+v"(tid));
        tid &= 255;
        const int lane = tid & 63;
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        vqf_rank<0, CT, false>(z, e, eb, nullptr, e2, eps_e, e2max, n, kq, rt, s, tid);
        const int* fin = s.fin;
        if (tid < 32 && n0 + tid < n) idx[(n0 + tid) * depth + q] = (int64_t)fin[tid];
        // thread (row = tid / 8, sub = tid % 8): columns 4 sub + 32 jj .. + 3, jj = 0..7, in every stage -- a thread reads back
        // only what it wrote itself in both tiles
        float local = 0.0f;
        const int row = tid >> 3, sub = tid & 7;
        if (n0 + row < n) {
            const float* er = e + (int64_t)fin[row] * FD + sub * 4;
            float* rr = rt + row * ZLD + sub * 4;
            float* qr = qt + row * ZLD + sub * 4;
            f32x4 ev[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) ev[jj] = *reinterpret_cast<const f32x4*>(er + 32 * jj);
            const int64_t o = (n0 + row) * FD + sub * 4;
            const bool last = q + 1 == depth;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const f32x4 rv = rvq_sub(*reinterpret_cast<const f32x4*>(rr + 32 * jj), ev[jj]);
                *reinterpret_cast<f32x4*>(rr + 32 * jj) = rv;
#pragma unroll
                for (int t = 0; t < 4; ++t) local = __fmaf_rn(rv[t], rv[t], local);
                if (want_q) {
                    const f32x4 acc = lk_accum(q == 0 ? ev[jj] : *reinterpret_cast<const f32x4*>(qr + 32 * jj), ev[jj], q == 0);
                    if (!last) {
                        *reinterpret_cast<f32x4*>(qr + 32 * jj) = acc;
                    } else {
                        if (q32) *reinterpret_cast<f32x4*>(q32 + o + 32 * jj) = acc;
                        if (q_lo) {
                            typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
                            const u32x2 ob = {pack2_bf16(acc[0], acc[1]), pack2_bf16(acc[2], acc[3])};
                            *reinterpret_cast<u32x2*>(q_lo + o + 32 * jj) = ob;
                        }
                    }
                }
            }
        }
        if (sse) lk_wave_part(local, sse_s[q], lane, wave);
        // histogram of the stage: duplicates inside the block are counted first
        if (hist && tid < 32 && n0 + tid < n) {
            const int me = tid;
            const int code = fin[me];
            int count = 0;
            bool leader = true;
            for (int u = 0; u < 32; ++u) {
                const bool same = (n0 + u < n) && fin[u] == code;
                count += same ? 1 : 0;
                if (same && u < me) leader = false;
            }
            if (leader) atomicAdd(hist + (int64_t)q * k + code, count);
        }
        // (no barrier here: the next ranking writes key / ncand / overflow only before its first barrier, fin after several)
    }
    if (sse) {
        const int tid = tid_blk;
        __syncthreads();
        if (tid < depth) lk_sse_emit(sse_s[tid], sse + tid, sse_part, (int64_t)blockIdx.x * depth + tid);
    }
}

// block = 32 rows x 256 channels, thread (row = tid / 8, sub = tid % 8): columns 4 sub + 32 jj .. + 3.
// DE: 0 no codebook gradient, 1 LDS chains + atomics, 2 the residual stack to rstack[N][depth][256] (deterministic mode).
// An index outside [0, K) (never written by the forward) is treated as a zero code without a gradient.
template <typename TDQ, bool HAS_DQ, int DE>
__global__ __launch_bounds__(256) void rvq_backward_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                           const int64_t* __restrict__ idx, const TDQ* __restrict__ dq, int64_t n,
                                                           int k, int depth, float cz, float ce, const float* __restrict__ gs,
                                                           float* __restrict__ dz, float* __restrict__ de,
                                                           float* __restrict__ rstack) {
    constexpr int ALD = FD + 32;
    __shared__ __attribute__((aligned(16))) float tile[DE == 1 ? 32 * ALD : 4];
    __shared__ int code_s[32], next_s[32], first_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    if (gs) { const float sc = *gs; cz *= sc; ce *= sc; }
    const int row = tid >> 3, sub = tid & 7;
    const bool live = n0 + row < n;
    const int64_t o = (n0 + row) * FD + sub * 4;
    f32x4 rv[8], sum[8];
    if (live) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) rv[jj] = *reinterpret_cast<const f32x4*>(z + o + 32 * jj);
    }
    for (int q = 0; q < depth; ++q) {
        if (DE == 1 && tid < 32) {
            const int64_t c = n0 + tid < n ? idx[(n0 + tid) * depth + q] : -1;
            code_s[tid] = (c >= 0 && c < k) ? (int)c : -1;
        }
        if (live) {
            const int64_t c = idx[(n0 + row) * depth + q];
            const bool ok = c >= 0 && c < k;
            const float* er = e + (ok ? c : 0) * FD + sub * 4;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const f32x4 ev = ok ? *reinterpret_cast<const f32x4*>(er + 32 * jj) : f32x4{0.f, 0.f, 0.f, 0.f};
                rv[jj] = rvq_sub(rv[jj], ev);
                sum[jj] = lk_accum(sum[jj], rv[jj], q == 0);
                if (DE == 1) *reinterpret_cast<f32x4*>(tile + row * ALD + sub * 4 + 32 * jj) = rv[jj];
                if (DE == 2) *reinterpret_cast<f32x4*>(rstack + ((n0 + row) * depth + q) * FD + sub * 4 + 32 * jj) = rv[jj];
            }
        }
        if constexpr (DE == 1) {
            __syncthreads();
            if (tid < 32) lk_build_chains(code_s, first_s, next_s, tid);
            __syncthreads();
            lk_chain_rows(tile, ALD, code_s, first_s, next_s, lane, wave, [&](int code, const float (&a)[4], int) {
                float* drow = de + (int64_t)code * FD;
#pragma unroll
                for (int t = 0; t < 4; ++t) atomicAdd(drow + t * 64 + lane, -ce * a[t]);
            });
            __syncthreads();                                         // the tile and the chains are rewritten by the next stage
        }
    }
    if (live) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const f32x4 g = lk_load_dq4<TDQ, HAS_DQ>(dq + o + 32 * jj);
            f32x4 out;
#pragma unroll
            for (int t = 0; t < 4; ++t) out[t] = __fmaf_rn(cz, sum[jj][t], g[t]);
            *reinterpret_cast<f32x4*>(dz + o + 32 * jj) = out;
        }
    }
}

// Deterministic codebook gradient: one block per code scans the flattened tokens idx[N * depth] in chunks of 256 (a wave's matches
// as one ballot mask, the four masks through LDS); thread c adds channel c of the matching rows of the residual stack, lowest
// (row, stage) first.  de[code] += -s ce sum.
__global__ __launch_bounds__(256) void rvq_code_grad_ordered_kernel(const float* __restrict__ rstack, const int64_t* __restrict__ idx,
                                                                    int64_t rows, float ce, const float* __restrict__ gs,
                                                                    float* __restrict__ de) {
    __shared__ unsigned long long masks[4];
    const int64_t code = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (gs) ce *= *gs;
    float acc = 0.f;
    // lk_ordered_scan written out: through the helper this kernel is allocated 11 VGPRs instead of 13
    for (int64_t r0 = 0; r0 < rows; r0 += 256) {
        const int64_t r = r0 + tid;
        const unsigned long long m = __ballot(r < rows && idx[r] == code);
        if (lane == 0) masks[wave] = m;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned long long mm = masks[w];                        // the same for every thread: no divergence
            while (mm) {
                const int b = __ffsll((long long)mm) - 1;
                acc += rstack[(r0 + w * 64 + b) * FD + tid];
                mm &= mm - 1;
            }
        }
        __syncthreads();
    }
    de[code * FD + tid] += -ce * acc;
}

}  // namespace

extern "C" {

static inline bool rvq_shape_ok(int64_t n, int k, int d, int depth) {
    return n >= 0 && k > 0 && k < (1 << 26) && d == FD && depth >= 1 && depth <= RVQ_MAX_DEPTH;
}

int vqk_rvq_forward_f32(const float* z, const float* e, const void* ws, int64_t ws_bytes, int64_t n, int k, int d, int depth,
                        int64_t* idx, float* q, void* q_lo, float* sse, int32_t* hist, void* stream) {
    VQK_REQUIRE(z && e && ws && idx, VQK_ERR_ARG);
    VQK_REQUIRE(rvq_shape_ok(n, k, d, depth) && (k % 32) == 0, VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(e) && vqk_aligned16(ws) && (!q || vqk_aligned16(q)) && (!q_lo || vqk_aligned16(q_lo)),
                VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqf_off_max(k, d) + 256, VQK_ERR_WORKSPACE);
    if (n == 0) return VQK_OK;
    const char* w = reinterpret_cast<const char*>(ws);
    const bf16_raw* eb = reinterpret_cast<const bf16_raw*>(w);
    const float* eps_e = reinterpret_cast<const float*>(w + vqf_off_eps(k, d));
    const float* e2 = reinterpret_cast<const float*>(w + vqf_off_e2(k, d));
    const float* e2max = reinterpret_cast<const float*>(w + vqf_off_max(k, d));
    const int per_wave = ((k >> 5) + 3) >> 2;
    const int ct = per_wave >= 8 ? 8 : per_wave >= 4 ? 4 : per_wave >= 2 ? 2 : 1;
    constexpr int lds = 2 * 32 * (FD + 4) * 4;                   // residual tile + zhat tile
    const dim3 grid((unsigned)((n + 31) / 32));
    hipStream_t st = vqk_stream(stream);
    LK_SSE_PART(sse_part, sse, (int64_t)grid.x * depth)
#define RVQ_LAUNCH(C) do { \
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&rvq_forward_kernel<C>), \
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds); \
        if (attr != hipSuccess) return VQK_ERR_LAUNCH; \
        hipLaunchKernelGGL((rvq_forward_kernel<C>), grid, dim3(256), (size_t)lds, st, z, e, eb, e2, eps_e, e2max, n, k, depth, idx, q, \
                           reinterpret_cast<bf16_raw*>(q_lo), sse, sse_part, hist); } while (0)
    if (ct == 8) RVQ_LAUNCH(8); else if (ct == 4) RVQ_LAUNCH(4); else if (ct == 2) RVQ_LAUNCH(2); else RVQ_LAUNCH(1);
#undef RVQ_LAUNCH
    VQK_CHECK_LAUNCH();
    if (sse_part) {
        hipLaunchKernelGGL(lk_sse_ordered_kernel<float>, dim3(1), dim3(64), 0, st, (const float*)sse_part, (int)grid.x, depth, sse);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

int vqk_rvq_decode_f32(const int64_t* idx, const float* e, int64_t n, int k, int d, int depth, float* q, void* q_lo, void* stream) {
    VQK_REQUIRE(idx && e && (q || q_lo), VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0 && d > 0 && (d % 4) == 0 && depth >= 1 && depth <= RVQ_MAX_DEPTH, VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(e) && (!q || vqk_aligned16(q)) && (!q_lo || (reinterpret_cast<uintptr_t>(q_lo) & 7u) == 0), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    hipLaunchKernelGGL(lk_decode_kernel<true>, dim3(vqk_grid_1d(n * (d / 4), 256)), dim3(256), 0, vqk_stream(stream), idx, e, n, k, d, depth, q,
                       reinterpret_cast<bf16_raw*>(q_lo));
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int64_t vqk_rvq_backward_ws_bytes(int64_t n, int d, int depth) {
    if (n < 0 || d != FD || depth < 1 || depth > RVQ_MAX_DEPTH) return VQK_ERR_SHAPE;
    return (n > 0 ? n : 1) * depth * (int64_t)d * 4;
}

int vqk_rvq_backward_f32(const float* z, const float* e, const int64_t* idx, const void* dq, int dq_dtype, int64_t n, int k, int d,
                         int depth, float cz, float ce, const float* gscale_dev, float* dz, float* de, void* ws, int64_t ws_bytes,
                         void* stream) {
    VQK_REQUIRE(z && e && idx && dz, VQK_ERR_ARG);
    VQK_REQUIRE(rvq_shape_ok(n, k, d, depth), VQK_ERR_SHAPE);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(e) && vqk_aligned16(dz) && (!dq || vqk_aligned16(dq)) && (!de || vqk_aligned16(de)),
                VQK_ERR_ALIGN);
    const bool ordered = de && vqkd::det_state().on;             // the residual stack goes through ws
    if (ordered) {
        VQK_REQUIRE(ws && ws_bytes >= vqk_rvq_backward_ws_bytes(n, d, depth), VQK_ERR_WORKSPACE);
        VQK_REQUIRE(vqk_aligned16(ws), VQK_ERR_ALIGN);
    }
    if (n == 0) return VQK_OK;
    const dim3 grid((unsigned)((n + 31) / 32));
    hipStream_t st = vqk_stream(stream);
    float* rstack = ordered ? reinterpret_cast<float*>(ws) : nullptr;
#define RVB(T, Q, E) hipLaunchKernelGGL((rvq_backward_kernel<T, Q, E>), grid, dim3(256), 0, st, z, e, idx, (const T*)dq, n, k, depth, cz, \
                                       ce, gscale_dev, dz, de, rstack)
    LK_DISPATCH_DQ_DE(RVB, dq, dq_dtype, !de ? 0 : !ordered ? 1 : 2);
#undef RVB
    VQK_CHECK_LAUNCH();
    if (ordered) {
        hipLaunchKernelGGL(rvq_code_grad_ordered_kernel, dim3((unsigned)k), dim3(256), 0, st, (const float*)rstack, idx, n * depth, ce,
                           gscale_dev, de);
        VQK_CHECK_LAUNCH();
    }
    return VQK_OK;
}

}  // extern "C"
