// ------------------------------------------------------------------------------------------------
// Nearest-codeword assignment (vqvae/modules/vector_quantizers.py:37-44, :337-343) as a bf16 CANDIDATE FILTER followed by
// an EXACT fp32 re-rank of the candidates -- indices stay bit-exact against oracle/vq_oracle.c (and so against the reference's
// own torch.argmin on the fixtures), but the N*K*D products run on the bf16 matrix pipe (2.5 PF) instead of the exact-fp32
// one (157 TF), which bounded vq_assign_reg_kernel at ~27 us for (8192, 1024, 256).
//
// Why the filter cannot lose the winner.  Notation: a_k = z.e_k in exact arithmetic; Z2, E2_k the fp32 squared norms both
// paths share; D_k the distance the exact path computes, fl(fl(Z2 + E2_k) - fl(2 A_k)) (Standard/EMA) or
// fl(fl(Z2 - fl(2 A_k)) + E2_k) (Entropy), A_k the canonical fp32 fma chain; S_k = fl(E2_k - fl(2 At_k)) the filter score,
// At_k the bf16 MFMA dot product of the RNE-rounded operands with fp32 accumulation.
//   |At_k - a_k| <= [(2 u + u^2) + 2^-14 (1 + u)^2] |z| |e_k|,  u = 2^-8 (bf16 unit roundoff; products of two bf16 are
//   exact in fp32; the 256-term accumulation is bounded at 4x the sequential round-to-nearest bound, which also covers a
//   truncating or tree-shaped accumulator)            =>  |S_k - (E2_k - 2 a_k)| <= delta_k := 0.0160 |z| |e_k|
//   |D_k - (Z2 + E2_k - 2 a_k)| <= eta := 2^-13 |z| max|e| + 2^-21 (Z2 + max E2)   (fma chain + the two outer roundings)
// If k* is the exact path's argmin then D_k* <= D_j for all j, hence S_k* - delta_k* <= min_j (S_j + delta_j) + 2 eta:
// every code passing   lo_k := S_k - delta_k  <=  U + H,   U := min_j (S_j + delta_j),  H := 2^-12 |z| max|e| + 2^-20 (Z2 + max E2)
// is a candidate, and k* (with every code tied with it) always is.  The candidates are re-ranked with the canonical fp32 chain
// (k order 8j + {0,4,1,5,2,6,3,7}, the order v_mfma_f32_32x32x2_f32 consumes) and the exact distance formula; the minimum
// of (distance, index) in lexicographic order = torch.argmin's first minimum.
//
// Kernel: block = 4 waves = 32 z rows (bf16 B fragments in registers for the whole kernel) x all K codes, every wave a
// contiguous quarter of the 32-code tiles, walked from a block-dependent start (the whole grid reads the same codebook);
// A fragments = the bf16 codebook in fragment-major order (prepared once per call): sixteen coalesced 1-KiB loads per
// tile, requested a whole tile ahead.  PASS 1 keeps lo_k of the first 8 tiles of every wave in registers (8 x 4 x 32 codes
// = all of K = 1024) and reduces U per row; PASS 2 compares them (or recomputes the tiles beyond) and appends the
// candidates to an LDS list; the block then evaluates its candidates exactly, one thread per candidate (z rows staged in
// LDS, the code row in two batches of 32 independent loads), and takes the row minima with 64-bit LDS atomics on
// (orderable distance bits, index).  A block whose list overflows (a collapsed codebook: thousands of near-ties) falls
// back to the exact-fp32 MFMA loop for its 32 rows -- no host decision, graph-capturable.
//
// Round 4: the quantizer FORWARD is this one kernel (vqk_vq_forward_f32).  What depends on the codebook only -- the bf16
// fragment-major copy, |e|^2, the margin factors, max |e|^2 -- is built by vqk_vq_prepare_f32 when the codebook CHANGES (after
// the optimizer step / the EMA update), not in every step.  The block stages its 32 z rows in LDS first: |z|^2 comes from
// there in the canonical order of row_sqnorm_kernel (bit-identical), the bf16 B fragments are LDS reads instead of
// 1-KiB-strided global loads, the re-rank and the epilogue reuse the tile.  Epilogue (vector_quantizers.py:44-56 fused):
// q = e[idx] gathered as fp32 and / or bf16, sum (q - z)^2 (one atomic per block), code histogram (duplicates inside the
// block counted first: one atomic per distinct code and block).
// ------------------------------------------------------------------------------------------------
#include "vq_filter.h"

namespace {

// codebook -> bf16 (RNE), FRAGMENT-MAJOR: [tile of 32 codes][k-step s 0..15][lane 0..63][8 bf16], lane = 32 * half + (code % 32)
// holds columns 16 s + 8 half .. + 7 of its code -- every MFMA A operand of the filter is ONE coalesced 1-KiB load (the
// row-major form made each load touch 32 different lines).  + delta factors eps_e[k] = F_DELTA * sqrt(E2_k).
// One wave per code row: lane l converts columns 4 l .. 4 l + 3.
__global__ __launch_bounds__(256) void vq_filter_prep_kernel(const float* __restrict__ e, const float* __restrict__ e2_in, int k,
                                                             bf16_raw* __restrict__ eb, float* __restrict__ eps_e,
                                                             float* __restrict__ e2_out) {
    const int lane = threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= k) return;
    const f32x4 v = *reinterpret_cast<const f32x4*>(e + (int64_t)row * FD + lane * 4);
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    const u32x2 o = {pack2_bf16(v[0], v[1]), pack2_bf16(v[2], v[3])};
    const int col = lane * 4, s = col >> 4, half = (col >> 3) & 1, w4 = col & 7;      // 4 columns inside one 8-column fragment slot
    const int64_t dst = ((((int64_t)(row >> 5) * 16 + s) * 64 + half * 32 + (row & 31)) * 8) + w4;
    *reinterpret_cast<u32x2*>(eb + dst) = o;
    float sq;
    if (e2_in) {
        sq = e2_in[row];
    } else {
        // |e|^2 in the canonical order of vq.hip::row_sqnorm_kernel (lane l: fma chain over l, l + 64, ...; xor butterfly 32..1)
        const float* p = e + (int64_t)row * FD;
        sq = 0.0f;
#pragma unroll
        for (int kk = 0; kk < FD; kk += 64) sq = __fmaf_rn(p[kk + lane], p[kk + lane], sq);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sq = __fadd_rn(sq, __shfl_xor(sq, off, 64));
    }
    if (lane == 0) {
        eps_e[row] = F_DELTA * sqrtf(sq);
        if (e2_out) e2_out[row] = sq;
    }
}

// max |e|^2 over the codebook (one block; behind the prep kernel on the same stream)
__global__ __launch_bounds__(256) void vq_filter_max_kernel(const float* __restrict__ e2, int k, float* __restrict__ out) {
    __shared__ float red[4];
    float m2 = 0.0f;
    for (int i = threadIdx.x; i < k; i += 256) m2 = fmaxf(m2, e2[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m2 = fmaxf(m2, __shfl_xor(m2, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m2;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// Dynamic LDS: 34 KiB (the block's z tile).  q32 / q_lo / sse / hist: the optional fused outputs of the quantizer forward;
// the ranking itself is vqf_rank (vq_filter.h).
template <int ASSOC, int CT>
__global__ __launch_bounds__(256, 1) void vq_assign_filter_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                                  const bf16_raw* __restrict__ eb,
                                                                  const float* __restrict__ z2_in, const float* __restrict__ e2,
                                                                  const float* __restrict__ eps_e,
                                                                  const float* __restrict__ e2max_in, int64_t n, int k,
                                                                  int64_t* __restrict__ idx, float* __restrict__ q32,
                                                                  bf16_raw* __restrict__ q_lo, float* __restrict__ sse,
                                                                  int32_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ZLD = FD + 4;
    float* zt = reinterpret_cast<float*>(smem);                  // [32][FD + 4]: the block's z rows (rows past n: row n - 1 again)
    __shared__ VqfLds s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    vqf_rank<ASSOC, CT, true>(z, e, eb, z2_in, e2, eps_e, e2max_in, n, k, zt, s, tid);
    const int* fin = s.fin;
    float* red_m = s.red_m;
    if (tid < 32 && n0 + tid < n) idx[n0 + tid] = (int64_t)fin[tid];
    if (!(q32 || q_lo || sse || hist)) return;      // kernel-uniform

    // ---------------------------------------------------------------- fused epilogue (vector_quantizers.py:44-56)
    // thread (row = tid / 8, sub = tid % 8): columns 4 sub + 32 jj .. + 3, jj = 0..7 -- all 32 rows of the block in flight at
    // once (eight threads cover 128 consecutive bytes of a row per jj); q = e[idx] as fp32 and / or bf16, sum (q - z)^2
    float local = 0.0f;
    {
        const int row = tid >> 3, sub = tid & 7;
        if (n0 + row < n) {
            const int code = fin[row];
            const float* er = e + (int64_t)code * FD + sub * 4;
            const float* zr = zt + row * ZLD + sub * 4;
            f32x4 ev[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) ev[jj] = *reinterpret_cast<const f32x4*>(er + 32 * jj);
            const int64_t o = (n0 + row) * FD + sub * 4;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const f32x4 zv = *reinterpret_cast<const f32x4*>(zr + 32 * jj);
                if (q32) *reinterpret_cast<f32x4*>(q32 + o + 32 * jj) = ev[jj];
                if (q_lo) {
                    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
                    const u32x2 ob = {pack2_bf16(ev[jj][0], ev[jj][1]), pack2_bf16(ev[jj][2], ev[jj][3])};
                    *reinterpret_cast<u32x2*>(q_lo + o + 32 * jj) = ob;
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) { const float dlt = ev[jj][t] - zv[t]; local = __fmaf_rn(dlt, dlt, local); }
            }
        }
    }
    if (sse) lk_wave_part(local, red_m, lane, wave);
    // histogram: duplicates inside the block are counted first (a collapsed codebook puts every row on a few codes)
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
    if (sse) {
        __syncthreads();
        if (tid == 0) lk_sse_emit(red_m, sse, nullptr, 0);
    }
}

// ------------------------------------------------------------------------------------------------
// Quantizer BACKWARD in one kernel (vector_quantizers.py:52-56 differentiated; replaces vq_backward_kernel +
// vq_code_grad_kernel = 8 + 51 us): block = 32 rows x 256 channels.
//   dz[row] = dq[row] + s cz (z[row] - e[idx[row]])
//   dE[k]  += s ce sum_{rows of the block with idx == k} (e[k] - z[row])
// The rows of a block that share a code are summed through an LDS tile first (CHAINS of vq_lookup.h), so the
// block sends ONE coalesced fp32 atomic row per DISTINCT code to dE: a collapsed codebook (every row on a few codes: the
// state of a fresh model) costs a few atomics per block instead of one per (row, channel), a spread-out assignment at most
// N x 256 uncontended ones.  Deterministic mode keeps the ordered two-kernel form (vq.hip).
// ------------------------------------------------------------------------------------------------
template <typename TDQ, bool HAS_DQ, bool HAS_DE>
__global__ __launch_bounds__(256) void vq_backward_fused_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                                const int64_t* __restrict__ idx, const TDQ* __restrict__ dq,
                                                                int64_t n, float cz, float ce, const float* __restrict__ gs,
                                                                float* __restrict__ dz, float* __restrict__ de) {
    constexpr int ALD = FD + 32;                                 // row pitch of the difference tile: the eight rows of a wave's
    __shared__ __attribute__((aligned(16))) float diff[HAS_DE ? 32 * ALD : 4];    // 16-byte stores land in disjoint bank halves
    __shared__ int code_s[32], next_s[32], first_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    if (gs) { const float s = *gs; cz *= s; ce *= s; }
    if (tid < 32) code_s[tid] = n0 + tid < n ? (int)idx[n0 + tid] : -1;
    {
        // thread (row = tid / 8, sub = tid % 8): columns 4 sub + 32 jj .. + 3 -- every load of the block in one batch
        const int row = tid >> 3, sub = tid & 7;
        if (n0 + row < n) {
            const int code = (int)idx[n0 + row];
            const int64_t o = (n0 + row) * FD + sub * 4;
            const float* er = e + (int64_t)code * FD + sub * 4;
            f32x4 zv[8], ev[8], g[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                zv[jj] = *reinterpret_cast<const f32x4*>(z + o + 32 * jj);
                ev[jj] = *reinterpret_cast<const f32x4*>(er + 32 * jj);
                g[jj] = lk_load_dq4<TDQ, HAS_DQ>(dq + o + 32 * jj);
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                f32x4 out, df;
#pragma unroll
                for (int t = 0; t < 4; ++t) { out[t] = __fmaf_rn(cz, zv[jj][t] - ev[jj][t], g[jj][t]); df[t] = ev[jj][t] - zv[jj][t]; }
                *reinterpret_cast<f32x4*>(dz + o + 32 * jj) = out;
                if constexpr (HAS_DE) *reinterpret_cast<f32x4*>(diff + row * ALD + sub * 4 + 32 * jj) = df;
            }
        }
    }
    if constexpr (!HAS_DE) return;
    __syncthreads();
    if (tid < 32) lk_build_chains(code_s, first_s, next_s, tid);
    __syncthreads();
    lk_chain_rows(diff, ALD, code_s, first_s, next_s, lane, wave, [&](int code, const float (&a)[4], int) {
        float* drow = de + (int64_t)code * FD;
#pragma unroll
        for (int t = 0; t < 4; ++t) atomicAdd(drow + t * 64 + lane, ce * a[t]);
    });
}

// EMA statistics (vector_quantizers.py:159-163: counts[k] = #rows on code k, dw[k] = sum of their z) with the same per-block
// pre-aggregation as the fused backward: the 32 rows of a block that share a code are chained and summed through an LDS tile,
// ONE coalesced fp32 atomic row (+ one count) per distinct code and block -- ema_stats_kernel issued one atomic per (row,
// channel): 120 us at (8192, 1024, 256) on the collapsed codebook of a fresh model (every row contends for a few code rows).
__global__ __launch_bounds__(256) void ema_stats_block_kernel(const float* __restrict__ z, const int64_t* __restrict__ idx, int64_t n,
                                                              float* __restrict__ counts, float* __restrict__ dw) {
    constexpr int ALD = FD + 32;
    __shared__ __attribute__((aligned(16))) float tile[32 * ALD];
    __shared__ int code_s[32], next_s[32], first_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    if (tid < 32) code_s[tid] = n0 + tid < n ? (int)idx[n0 + tid] : -1;
    {
        const int row = tid >> 3, sub = tid & 7;
        if (n0 + row < n) {
            const int64_t o = (n0 + row) * FD + sub * 4;
            f32x4 zv[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) zv[jj] = *reinterpret_cast<const f32x4*>(z + o + 32 * jj);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) *reinterpret_cast<f32x4*>(tile + row * ALD + sub * 4 + 32 * jj) = zv[jj];
        }
    }
    __syncthreads();
    if (tid < 32) lk_build_chains(code_s, first_s, next_s, tid);
    __syncthreads();
    lk_chain_rows(tile, ALD, code_s, first_s, next_s, lane, wave, [&](int code, const float (&a)[4], int cnt) {
        float* drow = dw + (int64_t)code * FD;
#pragma unroll
        for (int t = 0; t < 4; ++t) atomicAdd(drow + t * 64 + lane, a[t]);
        if (lane == 0) atomicAdd(counts + code, (float)cnt);
    });
}

}  // namespace

extern "C" {

int64_t vqk_vq_filter_ws_bytes(int k, int d) { return vqf_off_max(k, d) + 256; }

static int vqf_prepare(const float* e, const float* e2_in, int k, int d, void* ws, hipStream_t st) {
    char* w = reinterpret_cast<char*>(ws);
    float* e2w = reinterpret_cast<float*>(w + vqf_off_e2(k, d));
    hipLaunchKernelGGL(vq_filter_prep_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, e, e2_in, k,
                       reinterpret_cast<bf16_raw*>(w), reinterpret_cast<float*>(w + vqf_off_eps(k, d)), e2w);
    hipLaunchKernelGGL(vq_filter_max_kernel, dim3(1), dim3(256), 0, st, (const float*)e2w, k,
                       reinterpret_cast<float*>(w + vqf_off_max(k, d)));
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

static int vqf_launch(const float* z, const float* e, const void* ws, const float* z2, const float* e2, int64_t n, int k, int d,
                      int assoc, int64_t* idx, float* q32, void* q_lo, float* sse, int32_t* hist, hipStream_t st) {
    const char* w = reinterpret_cast<const char*>(ws);
    const bf16_raw* eb = reinterpret_cast<const bf16_raw*>(w);
    const float* eps_e = reinterpret_cast<const float*>(w + vqf_off_eps(k, d));
    const float* e2w = e2 ? e2 : reinterpret_cast<const float*>(w + vqf_off_e2(k, d));
    const float* e2max = reinterpret_cast<const float*>(w + vqf_off_max(k, d));
    const int per_wave = ((k >> 5) + 3) >> 2;
    const int ct = per_wave >= 8 ? 8 : per_wave >= 4 ? 4 : per_wave >= 2 ? 2 : 1;
    constexpr int lds = 34 * 1024;                               // the block's z tile
    const dim3 grid((unsigned)((n + 31) / 32));
#define VQF_LAUNCH(A, C) hipLaunchKernelGGL((vq_assign_filter_kernel<A, C>), grid, dim3(256), (size_t)lds, st, z, e, eb, z2, e2w, \
                                            eps_e, e2max, n, k, idx, q32, reinterpret_cast<bf16_raw*>(q_lo), sse, hist)
    if (assoc == 0) {
        if (ct == 8) VQF_LAUNCH(0, 8); else if (ct == 4) VQF_LAUNCH(0, 4); else if (ct == 2) VQF_LAUNCH(0, 2); else VQF_LAUNCH(0, 1);
    } else {
        if (ct == 8) VQF_LAUNCH(1, 8); else if (ct == 4) VQF_LAUNCH(1, 4); else if (ct == 2) VQF_LAUNCH(1, 2); else VQF_LAUNCH(1, 1);
    }
#undef VQF_LAUNCH
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_vq_assign_filtered_f32(const float* z, const float* e, const float* z2, const float* e2, int64_t n, int k, int d,
                               int assoc, int64_t* idx, void* ws, int64_t ws_bytes, void* stream) {
    VQK_REQUIRE(z && e && z2 && e2 && idx && ws, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0 && d == FD && (k % 32) == 0 && k < (1 << 26), VQK_ERR_SHAPE);
    VQK_REQUIRE(assoc == 0 || assoc == 1, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(e) && vqk_aligned16(ws) && vqk_aligned16(e2), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqk_vq_filter_ws_bytes(k, d), VQK_ERR_ARG);
    if (n == 0) return VQK_OK;
    hipStream_t st = vqk_stream(stream);
    const int rc = vqf_prepare(e, e2, k, d, ws, st);
    if (rc != VQK_OK) return rc;
    return vqf_launch(z, e, ws, z2, e2, n, k, d, assoc, idx, nullptr, nullptr, nullptr, nullptr, st);
}

int vqk_vq_prepare_f32(const float* e, int k, int d, void* ws, int64_t ws_bytes, void* stream) {
    VQK_REQUIRE(e && ws, VQK_ERR_ARG);
    VQK_REQUIRE(k > 0 && d == FD && (k % 32) == 0 && k < (1 << 26), VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(e) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqk_vq_filter_ws_bytes(k, d), VQK_ERR_WORKSPACE);
    return vqf_prepare(e, nullptr, k, d, ws, vqk_stream(stream));
}

int vqk_vq_forward_f32(const float* z, const float* e, const void* ws, int64_t ws_bytes, int64_t n, int k, int d, int assoc,
                       int64_t* idx, float* q, void* q_lo, float* sse, int32_t* hist, void* stream) {
    VQK_REQUIRE(z && e && ws && idx, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0 && d == FD && (k % 32) == 0 && k < (1 << 26), VQK_ERR_SHAPE);
    VQK_REQUIRE(assoc == 0 || assoc == 1, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(e) && vqk_aligned16(ws) && (!q || vqk_aligned16(q)) && (!q_lo || vqk_aligned16(q_lo)),
                VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqk_vq_filter_ws_bytes(k, d), VQK_ERR_WORKSPACE);
    if (n == 0) return VQK_OK;
    return vqf_launch(z, e, ws, nullptr, nullptr, n, k, d, assoc, idx, q, q_lo, sse, hist, vqk_stream(stream));
}

int vqk_ema_stats_fused_f32(const float* z, const int64_t* idx, int64_t n, int k, int d, float* counts, float* dw, void* stream) {
    VQK_REQUIRE(z && idx && counts && dw, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0 && d == FD, VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(z), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    if (vqkd::det_state().on) return vqk_ema_stats_f32(z, idx, n, k, d, counts, dw, stream);      // the ordered form (vq.hip)
    hipLaunchKernelGGL(ema_stats_block_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, vqk_stream(stream), z, idx, n, counts, dw);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_vq_backward_fused_f32(const float* z, const float* e, const int64_t* idx, const void* dq, int dq_dtype, int64_t n, int k,
                              int d, float cz, float ce, const float* gscale_dev, float* dz, float* de, void* stream) {
    VQK_REQUIRE(z && e && idx && dz, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0 && d == FD, VQK_ERR_SHAPE);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(vqk_aligned16(z) && vqk_aligned16(e) && vqk_aligned16(dz) && (!dq || vqk_aligned16(dq)), VQK_ERR_ALIGN);
    if (n == 0) return VQK_OK;
    const dim3 grid((unsigned)((n + 31) / 32));
#define VQB(T, Q, E) hipLaunchKernelGGL((vq_backward_fused_kernel<T, Q, (E) != 0>), grid, dim3(256), 0, vqk_stream(stream), z, e, idx, \
                                       (const T*)dq, n, cz, ce, gscale_dev, dz, de)
    LK_DISPATCH_DQ_DE(VQB, dq, dq_dtype, de ? 1 : 0);
#undef VQB
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // extern "C"
