// ------------------------------------------------------------------------------------------------
// The candidate filter + exact re-rank of csrc/vq_filter.hip as device functions (that file's header states the error bound and
// the kernel design): vqf_rank ranks the 32 rows of a block's LDS tile against the whole codebook and leaves the winners in
// VqfLds::fin.  Two kernels are built on it: vq_assign_filter_kernel (vq_filter.hip: one ranking per block, the input rows) and
// rvq_forward_kernel (rvq.hip: one ranking per stage, the tile holding the running residual).
// ------------------------------------------------------------------------------------------------
#pragma once
#include "vq_lookup.h"

namespace {

constexpr int FD = 256;                                          // embedding_dim of every reference config
constexpr int FCAP = 2048;                                       // candidate list capacity per block (64 per row on average)
constexpr float F_DELTA = 0.0160f;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

__device__ __forceinline__ unsigned pack2_bf16(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));   // v_cvt_pk_bf16_f32: round to nearest even
}

__device__ __forceinline__ unsigned orderable(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int ASSOC>
__device__ __forceinline__ float exact_dist(float zz, float e2c, float ab) {
    const float ab2 = 2.0f * ab;
    if (ASSOC == 0) return __fsub_rn(__fadd_rn(zz, e2c), ab2);
    return __fadd_rn(__fsub_rn(zz, ab2), e2c);
}

// the exact-fp32 MFMA loop of vq.hip::vq_assign_kernel for this block's 32 rows (overflow fallback); zt: the block's z tile
// [32][FD + 4] in LDS (already staged), zz: |z|^2 of the lane's row; the winners go to fin[32] (LDS)
template <int ASSOC>
__device__ void exact_block(const float* __restrict__ e, const float* __restrict__ e2, int k, const float* zt, float zz,
                            float* red_d, int* red_i, int* fin) {
    constexpr int ld = FD + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const float* zb = zt + j * ld + 4 * half;
    const int tiles = (k + 31) >> 5, per_wave = (tiles + 3) >> 2;
    const int t_begin = wave * per_wave, t_end = min(tiles, t_begin + per_wave);
    float best = INFINITY;
    int best_i = 0x7fffffff;
    for (int t = t_begin; t < t_end; ++t) {
        int code_row = t * 32 + j; if (code_row >= k) code_row = k - 1;
        const float* ea = e + (int64_t)code_row * FD + 4 * half;
        f32x16 acc = {0};
#pragma unroll 4
        for (int m = 0; m < FD; m += 8) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(ea + m);
            const f32x4 b = *reinterpret_cast<const f32x4*>(zb + m);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int code = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (code < k) {
                const float dist = exact_dist<ASSOC>(zz, e2[code], acc[r]);
                if (dist < best) { best = dist; best_i = code; }
            }
        }
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
        fin[tid] = (bi == 0x7fffffff) ? 0 : bi;
    }
}

// static LDS of one ranking (the z tile itself is dynamic LDS: [32][FD + 4] floats)
struct VqfLds {
    unsigned long long key[32];
    unsigned cand[FCAP];
    float red_u[4][32];
    float red_m[4];
    int ncand, overflow;
    float fb_d[128];
    int fb_i[128];
    float z2s[32];
    int fin[32];
};

// stage the rows n0 .. n0 + 31 of z in the tile zt [32][FD + 4] (coalesced 16-byte loads; rows past n: row n - 1 again)
__device__ __forceinline__ void vqf_load_rows(const float* __restrict__ z, int64_t n0, int64_t n, float* zt) {
    constexpr int ZLD = FD + 4;
    const int tid = threadIdx.x;
    f32x4 st[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int v = it * 256 + tid, r = v >> 6, c = v & 63;
        int64_t src = n0 + r; if (src >= n) src = n - 1;
        st[it] = *reinterpret_cast<const f32x4*>(z + src * FD + 4 * c);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int v = it * 256 + tid, r = v >> 6, c = v & 63;
        *reinterpret_cast<f32x4*>(zt + r * ZLD + 4 * c) = st[it];
    }
}

// One ranking of the tile zt [32][FD + 4] against the codebook: s.fin[r] = the exact path's argmin of row r, s.z2s[r] = |row r|^2.
// LOADZ: stage the rows n0 .. n0 + 31 of z into zt first (rows past n: row n - 1 again); otherwise the caller wrote zt and this
// function's first barrier orders that write before the reads.  Ends with a barrier: fin is visible to every thread.
// k % 32 == 0.  CT: tiles per wave whose lo values stay in REGISTERS between the passes (8 x 4 waves x 32 codes = all of
// K = 1024); tiles beyond them are recomputed in pass 2.  z2_in / e2max_in: optional precomputed |z|^2 per row / max |e|^2.
// tid: threadIdx.x, handed in by the kernel.
template <int ASSOC, int CT, bool LOADZ>
__device__ __forceinline__ void vqf_rank(const float* __restrict__ z, const float* __restrict__ e, const bf16_raw* __restrict__ eb,
                                         const float* __restrict__ z2_in, const float* __restrict__ e2,
                                         const float* __restrict__ eps_e, const float* __restrict__ e2max_in, int64_t n, int k,
                                         float* zt, VqfLds& lds, const int tid) {
    constexpr int ZLD = FD + 4;
    unsigned* cand = lds.cand;
    unsigned long long* key = lds.key;
    float (*red_u)[32] = lds.red_u;
    float* red_m = lds.red_m;
    int& ncand = lds.ncand;
    int& overflow = lds.overflow;
    float* fb_d = lds.fb_d;
    int* fb_i = lds.fb_i;
    float* z2s = lds.z2s;
    int* fin = lds.fin;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    const int j = lane & 31, half = lane >> 5;
    int64_t zrow = n0 + j; if (zrow >= n) zrow = n - 1;
    if (tid < 32) key[tid] = ~0ull;
    if (tid == 0) { ncand = 0; overflow = 0; }

    const int tiles = k >> 5;
    const int per_wave = (tiles + 3) >> 2;
    const int t_begin = wave * per_wave;
    const int t_end = min(tiles, t_begin + per_wave);
    const int cnt = max(t_end - t_begin, 0);
    // every block of the grid walks the same codebook: start each block at a different tile of its waves' ranges so that the
    // 256 CUs do not all ask the L2 for the same lines at the same moment (tile order inside a wave is free)
    const int rot = cnt > 0 ? (int)(blockIdx.x % (unsigned)cnt) : 0;
    auto tile_of = [&](int tt) -> int { int q = tt + rot; if (q >= cnt) q -= cnt; return t_begin + q; };
    // A fragments of one tile: 16 coalesced 1-KiB loads (fragment-major bf16 codebook)
    auto load_tile = [&](int t, u32x4 (&dst)[16]) {
        const bf16_raw* p = eb + (int64_t)t * (16 * 64 * 8) + lane * 8;
#pragma unroll
        for (int i = 0; i < 16; ++i) dst[i] = *reinterpret_cast<const u32x4*>(p + i * (64 * 8));
    };
    // the z tile first (coalesced 16-byte loads, HBM latency), the first two codebook tiles (L2) behind it
    if constexpr (LOADZ) vqf_load_rows(z, n0, n, zt);
    u32x4 fa[3][16];                                             // fragment ring: two tiles in flight behind the one being multiplied
    if (cnt > 0) load_tile(tile_of(0), fa[0]);
    if (cnt > 1) load_tile(tile_of(1), fa[1]);
    // max E2 over the codebook: prepared with the codebook, or K floats read by every block
    float e2max;
    if (e2max_in) {
        e2max = e2max_in[0];
    } else {
        float m2 = 0.0f;
        for (int i = tid; i < k; i += 256) m2 = fmaxf(m2, e2[i]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m2 = fmaxf(m2, __shfl_xor(m2, off, 64));
        if (lane == 0) red_m[wave] = m2;
    }
    __syncthreads();
    if (!e2max_in) e2max = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    // |z|^2: wave w owns rows 8 w .. 8 w + 7, canonical order of row_sqnorm_kernel (lane l: fma chain over l, l + 64, l + 128,
    // l + 192, then the xor butterfly 32 .. 1) => the same bits
    if (z2_in) {
        if (tid < 32) { int64_t r = n0 + tid; if (r >= n) r = n - 1; z2s[tid] = z2_in[r]; }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float* p = zt + (wave * 8 + i) * ZLD;
            float acc = 0.0f;
#pragma unroll
            for (int kk = 0; kk < FD; kk += 64) acc = __fmaf_rn(p[kk + lane], p[kk + lane], acc);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off, 64));
            if (lane == 0) z2s[wave * 8 + i] = acc;
        }
    }
    // this lane's slice of its z row as bf16 B fragments: k-step s covers columns 16 s + 8 half .. + 7
    bf16x8_t zf[16];
    {
        const float* zp = zt + j * ZLD + 8 * half;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(zp + 16 * s);
            const f32x4 b = *reinterpret_cast<const f32x4*>(zp + 16 * s + 4);
            const u32x4 o = {pack2_bf16(a[0], a[1]), pack2_bf16(a[2], a[3]), pack2_bf16(b[0], b[1]), pack2_bf16(b[2], b[3])};
            zf[s] = __builtin_bit_cast(bf16x8_t, o);
        }
    }
    __syncthreads();
    const float zz = z2s[j];
    const float zn = sqrtf(zz);
    const float hmargin = 2.44140625e-4f * zn * sqrtf(e2max) + 9.5367431640625e-7f * (zz + e2max);    // 2^-12, 2^-20

    // lo / hi of one tile from its fragments: acc = bf16 MFMA dot products of (32 codes) x (32 z rows); the lane owns z row j
    // and the 16 codes t*32 + (r&3) + 8*(r>>2) + 4*half
    // (vector-memory results return IN ORDER: the tile's own |e|^2 / margin loads are issued BEFORE the fragment prefetch of a
    // later tile -- `prefetch` -- so that waiting for them does not wait for the prefetch as well)
    auto tile_scores = [&](int t, const u32x4 (&frag)[16], float (&lo)[16], float (&hi)[16], auto&& prefetch) {
        f32x4 e2q[4], epq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            e2q[q] = *reinterpret_cast<const f32x4*>(e2 + t * 32 + 8 * q + 4 * half);
            epq[q] = *reinterpret_cast<const f32x4*>(eps_e + t * 32 + 8 * q + 4 * half);
        }
        __builtin_amdgcn_sched_barrier(0);
        prefetch();
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc = {0};
#pragma unroll
        for (int i = 0; i < 16; ++i)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, frag[i]), zf[i], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float sc = __fsub_rn(e2q[r >> 2][r & 3], 2.0f * acc[r]);
            const float dl = zn * epq[r >> 2][r & 3];
            lo[r] = sc - dl; hi[r] = sc + dl;
        }
    };

    // ---------------------------------------------------------------- pass 1: U = min_k hi_k per row
    // (the NEXT tile's sixteen loads are issued before this tile's MFMAs: a whole tile of matrix work covers the L2 latency)
    float u = INFINITY;
    float lo_reg[CT][16];
#pragma unroll
    for (int tt = 0; tt < CT; ++tt) {
        if (tt < cnt) {
            float hi[16];
            tile_scores(tile_of(tt), fa[tt % 3], lo_reg[tt], hi, [&]() { if (tt + 2 < cnt) load_tile(tile_of(tt + 2), fa[(tt + 2) % 3]); });
#pragma unroll
            for (int r = 0; r < 16; ++r) u = fminf(u, hi[r]);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) lo_reg[tt][r] = INFINITY;
        }
    }
    // tiles beyond the register cache (K > 1024): same ring, three tiles per trip (ring slot = tile % 3; CT % 3 == CT_R)
    constexpr int CT_R = CT % 3;
    for (int tt = CT; tt < cnt; tt += 3) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (tt + q < cnt) {
                float lo[16], hi[16];
                tile_scores(tile_of(tt + q), fa[(CT_R + q) % 3], lo, hi,
                            [&]() { if (tt + q + 2 < cnt) load_tile(tile_of(tt + q + 2), fa[(CT_R + q + 2) % 3]); });
#pragma unroll
                for (int r = 0; r < 16; ++r) u = fminf(u, hi[r]);
            }
        }
    }
    u = fminf(u, __shfl_xor(u, 32, 64));
    if (half == 0) red_u[wave][j] = u;
    __syncthreads();
    const float thr = fminf(fminf(red_u[0][j], red_u[1][j]), fminf(red_u[2][j], red_u[3][j])) + hmargin;

    // ---------------------------------------------------------------- pass 2: candidates
    // a lane's candidates of the cached tiles are counted first and appended with ONE LDS atomic (a returning atomic per
    // candidate cost a round trip each: 3 us of the kernel)
    auto tile_mask = [&](const float (&lo)[16]) -> unsigned {
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) mask |= (lo[r] <= thr ? 1u : 0u) << r;
        return mask;
    };
    auto append = [&](int t, unsigned mask, int& pos) {
        while (mask) {
            const int r = __builtin_ctz(mask);
            mask &= mask - 1;
            if (pos < FCAP) cand[pos] = ((unsigned)j << 26) | (unsigned)(t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half);
            else overflow = 1;
            ++pos;
        }
    };
    {
        unsigned masks[CT];
        int total = 0;
#pragma unroll
        for (int tt = 0; tt < CT; ++tt) {
            masks[tt] = tt < cnt ? tile_mask(lo_reg[tt]) : 0u;
            total += __builtin_popcount(masks[tt]);
        }
        if (total) {
            int pos = atomicAdd(&ncand, total);
#pragma unroll
            for (int tt = 0; tt < CT; ++tt)
                if (masks[tt]) append(tile_of(tt), masks[tt], pos);
        }
    }
    if (CT < cnt) {
        load_tile(tile_of(CT), fa[0]);
        if (CT + 1 < cnt) load_tile(tile_of(CT + 1), fa[1]);
    }
    for (int tt = CT; tt < cnt; tt += 3) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (tt + q < cnt) {
                float lo[16], hi[16];
                tile_scores(tile_of(tt + q), fa[q], lo, hi, [&]() { if (tt + q + 2 < cnt) load_tile(tile_of(tt + q + 2), fa[(q + 2) % 3]); });
                const unsigned mask = tile_mask(lo);
                if (mask) {
                    int pos = atomicAdd(&ncand, __builtin_popcount(mask));
                    append(tile_of(tt + q), mask, pos);
                }
            }
        }
    }
    __syncthreads();
    if (overflow) {                                              // block-uniform
        exact_block<ASSOC>(e, e2, k, zt, zz, fb_d, fb_i, fin);
    } else {
        // ------------------------------------------------------------ exact re-rank, one thread per candidate
        // The 256-term fma chain is sequential by definition; what can be hidden is its operand traffic: the z rows come from
        // the LDS tile, a candidate's code row arrives in two batches of 32 independent 16-byte loads (two L2 round trips
        // instead of sixteen).
        const int nc = ncand;
        for (int c = tid; c < nc; c += 256) {
            const unsigned pk = cand[c];
            const int row = (int)(pk >> 26), code = (int)(pk & 0x03ffffffu);
            const float* zr = zt + row * ZLD;
            const float* er = e + (int64_t)code * FD;
            float acc = 0.0f;
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
                f32x4 ev[32];
#pragma unroll
                for (int i = 0; i < 32; ++i) ev[i] = *reinterpret_cast<const f32x4*>(er + hb * 128 + 4 * i);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const f32x4 za = *reinterpret_cast<const f32x4*>(zr + hb * 128 + 8 * i);
                    const f32x4 zb = *reinterpret_cast<const f32x4*>(zr + hb * 128 + 8 * i + 4);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        acc = __fmaf_rn(ev[2 * i][t], za[t], acc);
                        acc = __fmaf_rn(ev[2 * i + 1][t], zb[t], acc);
                    }
                }
            }
            const float dist = exact_dist<ASSOC>(z2s[row], e2[code], acc);
            // a NaN distance is never a candidate's winner: a row whose distances are ALL NaN keeps index 0 (as torch.argmin
            // does for an all-NaN row); a row with some NaN codes returns the finite argmin here, the first NaN in torch --
            // the exact kernel (vq.hip) behaves the same way, NaN latents / codes are outside the contract
            if (dist == dist)
                atomicMin(&key[row], ((unsigned long long)orderable(dist) << 32) | (unsigned)code);
        }
        __syncthreads();
        if (tid < 32) {
            const unsigned long long kk = key[tid];
            fin[tid] = kk == ~0ull ? 0 : (int)(kk & 0xffffffffull);
        }
    }
    __syncthreads();
}

// workspace: bf16 fragment-major codebook | eps_e[K] | e2[K] | max e2 (256-byte aligned sections)
static inline int64_t vqf_off_eps(int k, int d) { return ((int64_t)k * d * 2 + 255) & ~(int64_t)255; }
static inline int64_t vqf_off_e2(int k, int d) { return vqf_off_eps(k, d) + (((int64_t)k * 4 + 255) & ~(int64_t)255); }
static inline int64_t vqf_off_max(int k, int d) { return vqf_off_e2(k, d) + (((int64_t)k * 4 + 255) & ~(int64_t)255); }

}  // namespace
