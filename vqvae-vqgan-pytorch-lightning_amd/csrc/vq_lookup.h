// The block-level pieces the nearest-code quantizers share: standard / EMA (vq.hip, vq_filter.hip), residual (rvq.hip) and cosine
// (vq_cos.hip).  The rankings stay where they are (vqf_rank in vq_filter.h, the MFMA loops of vq.hip and cos_forward_kernel); what
// a kernel does with the 32 winners of its block is here, once.  Pieces, not a framework: a kernel owns its barriers, its LDS and
// its accumulators and calls a piece between them.  Every piece began as the standard quantizer's text and was copied into the
// residual and the cosine quantizer; the schemes they implement:
//   CHAINS       (vq_backward_fused_kernel): the rows of a block that share a code form a chain in row order; every wave walks
//                the chains whose head it owns and adds the members' rows of an LDS tile lowest row first: ONE coalesced fp32
//                atomic row per distinct (code, block).  A collapsed codebook costs a few atomics per block, not one per element.
//   ORDERED SCAN (ema_stats_ordered_kernel; deterministic mode): one block per code scans the tokens in chunks of 256, a wave's
//                matches as one ballot mask, the four masks through LDS; every thread visits the matching rows lowest first.
//                No atomics, the same bits every run.
//   SSE          the block's partial of a squared-error sum: waves by butterfly, then (w0 + w1) + (w2 + w3); one float atomic
//                per block or, in deterministic mode, a slot of the ordered-sum workspace that lk_sse_ordered_kernel adds up
//                in block order.
//   DECODE       tokens -> the sum of their code rows in stage order (depth 1: the code row); a token outside [0, K) reads
//                nothing and adds nothing.
// What stays written out, because through a helper the register allocation of the kernel changed (profiles/vq_lookup_core_ab.txt):
// the argmin merge over half-waves and waves at the end of every ranking (vq.hip, vq_filter.h::exact_block, cos_forward_kernel:
// through one function cos_forward_kernel<64> went from 199 to 151 VGPRs, <16> from 83 to 111, vq_assign_filter_kernel<., 1> from
// 138 to 140 AGPRs, rvq_forward_kernel<1> from 174 to 172) and the ordered scan of rvq_code_grad_ordered_kernel (11 instead of 13
// VGPRs).  The block histogram of the three fused forwards (thread r < 32 counts the rows of the block on its code, the lowest row
// of a code adds the count: duplicates inside the block first) stays written out as well: as a function it left the figures alone
// but reordered 230 to 720 instructions of the ranking kernels, and rvq_forward_kernel measured 0.5 to 1 % slower.
// cos_backward_kernel keeps its own chain walk: 64 columns and a projection before the atomic.
#pragma once
#include "common.h"

namespace {

// CALLER: threads tid < 32 between two barriers, code_s[32] written (-1: no code).  first_s[r] == r marks a chain's head,
// next_s[r] its next member (-1: none).
// (an LDS float atomic per element was tried first: ds_add_f32 under the 8-way bank conflicts of the tile cost 9 us)
__device__ __forceinline__ void lk_build_chains(const int* code_s, int* first_s, int* next_s, int tid) {
    const int code = code_s[tid];
    int first = tid, next = -1;
    if (code >= 0) {
        for (int u = 0; u < tid; ++u)
            if (code_s[u] == code) { first = u; break; }
        for (int u = tid + 1; u < 32; ++u)
            if (code_s[u] == code) { next = u; break; }
    }
    first_s[tid] = first; next_s[tid] = next;
}

// 256-column tile [32][ald]: wave w owns the heads w, w + 4, ...; lane: columns lane + 64 t.  emit(code, a, members) once per
// distinct code of the block, a = the chain's rows added in row order (the sum inside a block is deterministic; the order of the
// blocks' atomics is not).
template <typename Emit>
__device__ __forceinline__ void lk_chain_rows(const float* tile, int ald, const int* code_s, const int* first_s, const int* next_s,
                                              int lane, int wave, Emit&& emit) {
    for (int r = wave; r < 32; r += 4) {
        if (code_s[r] < 0 || first_s[r] != r) continue;          // wave-uniform
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        int cnt = 0;
        for (int m = r; m >= 0; m = next_s[m]) {
            ++cnt;
#pragma unroll
            for (int t = 0; t < 4; ++t) a[t] += tile[m * ald + t * 64 + lane];
        }
        emit(code_s[r], a, cnt);
    }
}

// block of 256 threads = code `code`; visit(row) for every row < rows with idx[row] == code, lowest row first, the same sequence
// in every thread with `walk` set (the masks are the same for every thread: no divergence; a thread without a column to add
// skips the walk).  Returns the number of matches (in the walking threads).
template <typename Visit>
__device__ __forceinline__ int lk_ordered_scan(const int64_t* idx, int64_t rows, int64_t code, unsigned long long* masks, bool walk,
                                               Visit&& visit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cnt = 0;
    for (int64_t r0 = 0; r0 < rows; r0 += 256) {
        const int64_t r = r0 + tid;
        const unsigned long long m = __ballot(r < rows && idx[r] == code);
        if (lane == 0) masks[wave] = m;
        __syncthreads();
        if (walk) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unsigned long long mm = masks[w];
                cnt += __popcll(mm);
                while (mm) {
                    const int b = __ffsll((long long)mm) - 1;
                    visit(r0 + w * 64 + b);
                    mm &= mm - 1;
                }
            }
        }
        __syncthreads();
    }
    return cnt;
}

// a wave's sum of `local` to part[wave]; the caller's barrier, then lk_sse_emit in ONE thread
__device__ __forceinline__ void lk_wave_part(float local, float* part, int lane, int wave) {
    local = wave_sum(local);
    if (lane == 0) part[wave] = local;
}
__device__ __forceinline__ void lk_sse_emit(const float* part, float* sse, float* sse_part, int64_t slot) {
    const float tot = (part[0] + part[1]) + (part[2] + part[3]);
    if (sse_part) sse_part[slot] = tot;                          // deterministic mode: added in block order below
    else atomicAdd(sse, tot);
}

// deterministic mode: sse[q] += the blocks' partials part[blocks][depth] in block order (one thread per stage)
// (a template so that only the files that launch it carry it)
template <typename T>
__global__ void lk_sse_ordered_kernel(const T* __restrict__ part, int blocks, int depth, T* __restrict__ sse) {
    const int q = threadIdx.x;
    if (q >= depth) return;
    T acc = 0.0f;
    for (int b = 0; b < blocks; ++b) acc += part[(int64_t)b * depth + q];
    sse[q] += acc;
}

// the ordered-sum workspace of vqk_set_deterministic for `slots` block partials (nullptr: default mode, one float atomic per block)
#define LK_SSE_PART(var, want, slots) \
    float* var = nullptr; \
    if ((want) && vqkd::det_state().on) { \
        const vqkd::DetState& det = vqkd::det_state(); \
        VQK_REQUIRE(det.ws && det.bytes >= (int64_t)(slots) * 4, VQK_ERR_WORKSPACE); \
        var = det.ws; \
    }

// 16 bytes of the upstream gradient as fp32: fp32, bf16 or absent (zeros)
template <typename TDQ, bool HAS_DQ>
__device__ __forceinline__ f32x4 lk_load_dq4(const TDQ* p) {
    if constexpr (!HAS_DQ) return f32x4{0.f, 0.f, 0.f, 0.f};
    else if constexpr (sizeof(TDQ) == 4) return *reinterpret_cast<const f32x4*>(p);
    else {
        const u16x4 r = *reinterpret_cast<const u16x4*>(p);
        return f32x4{bf16_to_f32(r[0]), bf16_to_f32(r[1]), bf16_to_f32(r[2]), bf16_to_f32(r[3])};
    }
}

// LAUNCH(T, HAS_DQ, DE) for the upstream gradient's type / absence and the codebook-gradient mode `de_mode` (0: none, 1: chains +
// atomics, 2: ordered; a kernel with two modes maps DE != 0 to its flag)
#define LK_DISPATCH_DQ_DE(LAUNCH, dq, dq_dtype, de_mode) do { \
        if (!(dq)) { if ((de_mode) == 0) LAUNCH(float, false, 0); else if ((de_mode) == 1) LAUNCH(float, false, 1); else LAUNCH(float, false, 2); } \
        else if ((dq_dtype) == VQK_F32) { if ((de_mode) == 0) LAUNCH(float, true, 0); else if ((de_mode) == 1) LAUNCH(float, true, 1); else LAUNCH(float, true, 2); } \
        else { if ((de_mode) == 0) LAUNCH(bf16_raw, true, 0); else if ((de_mode) == 1) LAUNCH(bf16_raw, true, 1); else LAUNCH(bf16_raw, true, 2); } \
    } while (0)

// acc <- acc + ev in one fp32 addition per element; the first term assigns (0 + x would turn a -0 into +0)
__device__ __forceinline__ f32x4 lk_accum(const f32x4 acc, const f32x4 ev, bool first) {
    if (first) return ev;
    f32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = __fadd_rn(acc[t], ev[t]);
    return o;
}

// q[row] = sum over the row's `depth` tokens of e[token] (lk_accum, stage order): one thread per (row, four columns).
// PACKED: the bf16 copy through the packed hardware conversion (the residual quantizer's), else the software rounding of
// f32_to_bf16 (the cosine quantizer's) -- the two agree on every finite value and on infinities, not on a NaN's payload.
template <bool PACKED>
__global__ __launch_bounds__(256) void lk_decode_kernel(const int64_t* __restrict__ idx, const float* __restrict__ e, int64_t n, int k,
                                                        int d, int depth, float* __restrict__ q32, bf16_raw* __restrict__ q_lo) {
    const int d4 = d >> 2;
    const int64_t total = n * d4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / d4;
        const int c = (int)(i - row * d4) * 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        bool first = true;
        for (int q = 0; q < depth; ++q) {
            const int64_t code = idx[row * depth + q];
            if (code < 0 || code >= k) continue;
            acc = lk_accum(acc, *reinterpret_cast<const f32x4*>(e + code * d + c), first);
            first = false;
        }
        if (q32) *reinterpret_cast<f32x4*>(q32 + row * d + c) = acc;
        if (q_lo) {
            if constexpr (PACKED) {
                typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
                const u32x2 ob = {vqk_pack_bf16x2(acc[0], acc[1]), vqk_pack_bf16x2(acc[2], acc[3])};
                *reinterpret_cast<u32x2*>(q_lo + row * d + c) = ob;
            } else {
                const u16x4 ob = {f32_to_bf16(acc[0]), f32_to_bf16(acc[1]), f32_to_bf16(acc[2]), f32_to_bf16(acc[3])};
                *reinterpret_cast<u16x4*>(q_lo + row * d + c) = ob;
            }
        }
    }
}

}  // namespace
