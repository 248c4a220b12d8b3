// ------------------------------------------------------------------------------------------------
// k-means codebook initialisation: k-means++ seeding (Arthur & Vassilvitskii 2007) and the centroid update of a Lloyd iteration.
// The assignment and the per-cluster sums of an iteration are vq.hip / vq_filter.hip's (vqk_vq_assign*_f32, vqk_ema_stats*_f32).
//
// SEEDING, pick j of K (include/vqk.h states the rule): with c = x[picks[j-1]] read on the device,
//   mind[i] <- min(mind[i], sum_d (x[i,d] - c[d])^2)        the difference form: a row bit-equal to c gets exactly 0
//   S = sum_i mind[i], t = u[j] S, picks[j] = the first row whose running sum of mind exceeds t     (float64)
// Nothing comes back to the host between the picks: the loop is 2 K - 1 launches on one stream.
//
// Launch 1 (kmeans_seed_update_kernel, ceil(N / 64) blocks): a block owns 64 consecutive rows, whatever N and D -- the summation
// order depends on the shape only.  A row is spread over G lanes (G = the power of two >= D / 4, at most 64; lane s of the group
// loads the 16-byte chunks s, s + G, ... of the row, the centre's chunks stay in its registers), every lane runs one fma chain over
// its elements and the group adds across lanes by an xor tree.  Lane 0 of the group updates mind; the block's 64 new values are
// added in float64 by one wave (xor tree) into part[block].  D = 256: one row per wave and load instruction, 16 rows per wave.
//
// Launch 2 (kmeans_seed_pick_kernel, ONE block): the kernel boundary is what makes every block's partial visible -- no block waits
// for another, no counter, no fence.  The blocks' partials are summed in three fixed levels (a thread's segment of consecutive
// blocks, groups of 16 segments, the 16 groups), then ONE thread descends the same levels with the running sum it carries: the
// first group whose end exceeds t, the first segment in it, the first block, the first row.  Each level's running sum is sequential,
// so monotone: the entry it stops at holds a positive value.  Where rounding (a level's sum was added in another association than
// the running sum below it) leaves no entry that exceeds t, the level takes its LAST positive entry -- at every level, that is the
// largest row with mind > 0.  S == 0 (fewer distinct rows than centres): floor(u N), clamped.
//
// What bounds a pick: the N x D x 4 bytes of x (launch 1; 64 MiB at N = 65,536, D = 256, resident in the 256 MiB Infinity Cache
// from the second pick on) plus the latency chain of launch 2 (a handful of dependent LDS / L2 reads and ~100 float64 adds).
// ------------------------------------------------------------------------------------------------
#include "common.h"

namespace {

constexpr int KM_ROWS = 64;                    // rows per block of the seeding update (vqk_kmeans_seed_ws_bytes, ops.KMEANS_SEED_ROWS)
constexpr int KM_MAX_D = 1024;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int64_t km_uniform_pick(double u, int64_t n) {
    int64_t p = (int64_t)floor(u * (double)n);
    if (p > n - 1) p = n - 1;
    if (p < 0) p = 0;
    return p;
}

// step 0: mind <- +inf, picks[0] = floor(u[0] N) clamped, total[0] = +inf (the sum of what mind holds)
__global__ __launch_bounds__(256) void kmeans_seed_first_kernel(int64_t n, const double* __restrict__ u, int64_t* __restrict__ picks,
                                                                float* __restrict__ mind, double* __restrict__ total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) mind[i] = __builtin_inff();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        picks[0] = km_uniform_pick(u[0], n);
        if (total) total[0] = (double)__builtin_inff();
    }
}

// G lanes per row, C 16-byte chunks per lane (C > 1 only with G = 64: D > 256)
template <int G, int C>
__global__ __launch_bounds__(256) void kmeans_seed_update_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                 const int64_t* __restrict__ picks, int j, float* __restrict__ mind,
                                                                 double* __restrict__ part) {
    constexpr int PASSES = G >= 4 ? G / 4 : 1;                   // 256 / G rows per pass; G < 4: one pass, threads past row 63 idle
    constexpr int RPP = 256 / G;
    constexpr int UB = (8 / C) < PASSES ? (8 / C) : PASSES;      // passes whose loads are issued together (8 x 16 bytes per lane)
    __shared__ float m_s[KM_ROWS];
    const int tid = threadIdx.x, sub = tid & (G - 1), rsub = tid / G;
    const int d4 = d >> 2;
    int64_t prev = picks[j - 1];
    prev = prev < 0 ? 0 : (prev > n - 1 ? n - 1 : prev);         // (written by the step before: in range; a foreign value reads no stray row)
    f32x4 cv[C];
    bool has[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int chunk = sub + c * G;
        has[c] = chunk < d4;
        cv[c] = has[c] ? *reinterpret_cast<const f32x4*>(x + prev * d + chunk * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int64_t n0 = (int64_t)blockIdx.x * KM_ROWS;
#pragma unroll
    for (int p0 = 0; p0 < PASSES; p0 += UB) {
        f32x4 v[UB][C];
#pragma unroll
        for (int p = 0; p < UB; ++p) {
            const int rib = (p0 + p) * RPP + rsub;
            const int64_t row = n0 + rib;
            const bool live = rib < KM_ROWS && row < n;
#pragma unroll
            for (int c = 0; c < C; ++c)
                v[p][c] = (live && has[c]) ? *reinterpret_cast<const f32x4*>(x + row * d + (sub + c * G) * 4) : cv[c];
        }
#pragma unroll
        for (int p = 0; p < UB; ++p) {
            const int rib = (p0 + p) * RPP + rsub;
            const int64_t row = n0 + rib;
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float df = __fsub_rn(v[p][c][t], cv[c][t]);
                    acc = __fmaf_rn(df, df, acc);
                }
            }
#pragma unroll
            for (int off = G >> 1; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
            if (sub == 0 && rib < KM_ROWS) {
                float m = 0.f;                                    // rows past n add nothing to the block's sum
                if (row < n) {
                    m = fminf(mind[row], acc);
                    mind[row] = m;
                }
                m_s[rib] = m;
            }
        }
    }
    __syncthreads();
    if (tid < 64) {
        const double s = wave_sum_f64((double)m_s[tid]);
        if (tid == 0) part[blockIdx.x] = s;
    }
}

// first q in [0, cnt) with acc + v[q] > t, acc the sequential running sum; none: the last q with v[q] > 0.
// acc <- the running sum in front of q.  No early exit: the loads of v do not wait for the adds.
template <typename Load>
__device__ __forceinline__ int km_descend(int cnt, double t, double& acc, Load load) {
    int found = -1, last_pos = -1;
    double acc_found = acc, acc_last = acc, run = acc;
    for (int q = 0; q < cnt; ++q) {
        const double vq = load(q);
        const double nxt = run + vq;
        if (found < 0 && nxt > t) { found = q; acc_found = run; }
        if (vq > 0.0) { last_pos = q; acc_last = run; }
        run = nxt;
    }
    if (found >= 0) { acc = acc_found; return found; }
    acc = acc_last;
    return last_pos < 0 ? 0 : last_pos;                          // (a level below a positive sum always holds a positive entry)
}

__global__ __launch_bounds__(256) void kmeans_seed_pick_kernel(const double* __restrict__ part, int64_t blocks, int64_t n,
                                                               const float* __restrict__ mind, const double* __restrict__ u, int j,
                                                               int64_t* __restrict__ picks, double* __restrict__ total) {
    __shared__ double seg_s[256];
    __shared__ double grp_s[16];
    const int tid = threadIdx.x;
    const int64_t per = (blocks + 255) / 256;                    // consecutive blocks per thread
    {
        const int64_t b0 = (int64_t)tid * per;
        const int64_t b1 = b0 + per < blocks ? b0 + per : blocks;
        double s = 0.0;
        for (int64_t b = b0; b < b1; ++b) s += part[b];
        seg_s[tid] = s;
    }
    __syncthreads();
    if (tid < 16) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += seg_s[tid * 16 + q];
        grp_s[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) sum += grp_s[q];
    if (total) total[j] = sum;
    const double uj = u[j];
    int64_t pick = km_uniform_pick(uj, n);                       // S == 0: every row coincides with a centre
    if (sum > 0.0) {
        const double t = uj * sum;
        double acc = 0.0;
        const int g = km_descend(16, t, acc, [&](int q) { return grp_s[q]; });
        const int s = g * 16 + km_descend(16, t, acc, [&](int q) { return seg_s[g * 16 + q]; });
        const int64_t b0 = (int64_t)s * per;
        const int64_t left = blocks - b0;
        const int64_t b = b0 + km_descend((int)(left < per ? left : per), t, acc, [&](int q) { return part[b0 + q]; });
        const int64_t r0 = b * KM_ROWS;
        const int64_t rows = n - r0 < KM_ROWS ? n - r0 : KM_ROWS;
        pick = r0 + km_descend((int)rows, t, acc, [&](int q) { return (double)mind[r0 + q]; });
    }
    picks[j] = pick;
}

// one wave per centre: c <- sums / count where count > 0; moved = |c_new - c_old|^2 (float64 sum, rounded once)
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ counts, const float* __restrict__ sums, int k,
                                                            int d, float* __restrict__ centres, float* __restrict__ moved) {
    const int lane = threadIdx.x & 63;
    const int code = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (code >= k) return;                                       // wave-uniform
    const float cnt = counts[code];
    double mv = 0.0;
    if (cnt > 0.f) {
        for (int c = lane * 4; c < d; c += 256) {
            const int64_t o = (int64_t)code * d + c;
            const f32x4 sv = {sums[o], sums[o + 1], sums[o + 2], sums[o + 3]};      // (the packed buffer puts sums K floats in: any alignment)
            const f32x4 old = *reinterpret_cast<const f32x4*>(centres + o);
            f32x4 nv;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                nv[t] = __fdiv_rn(sv[t], cnt);
                const double df = (double)nv[t] - (double)old[t];
                mv += df * df;
            }
            *reinterpret_cast<f32x4*>(centres + o) = nv;
        }
    }
    mv = wave_sum_f64(mv);
    if (moved && lane == 0) moved[code] = (float)mv;
}

}  // namespace

extern "C" {

static inline bool km_seed_shape_ok(int64_t n, int d) {
    return n >= 1 && n <= ((int64_t)1 << 36) && d >= 4 && d <= KM_MAX_D && (d % 4) == 0;
}

int64_t vqk_kmeans_seed_ws_bytes(int64_t n) {
    if (n < 1 || n > ((int64_t)1 << 36)) return VQK_ERR_SHAPE;
    const int64_t blocks = (n + KM_ROWS - 1) / KM_ROWS;
    return ((blocks * 8 + 15) / 16) * 16;
}

int vqk_kmeans_seed_step_f32(const float* x, int64_t n, int d, int k, int j, const double* u, int64_t* picks, float* mind,
                             double* total, void* ws, int64_t ws_bytes, void* stream) {
    VQK_REQUIRE(x && u && picks && mind && ws, VQK_ERR_ARG);
    VQK_REQUIRE(km_seed_shape_ok(n, d) && k >= 1 && j >= 0 && j < k, VQK_ERR_SHAPE);
    VQK_REQUIRE(ws_bytes >= vqk_kmeans_seed_ws_bytes(n), VQK_ERR_WORKSPACE);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    hipStream_t st = vqk_stream(stream);
    if (j == 0) {
        hipLaunchKernelGGL(kmeans_seed_first_kernel, dim3(vqk_grid_1d(n, 256)), dim3(256), 0, st, n, u, picks, mind, total);
        VQK_CHECK_LAUNCH();
        return VQK_OK;
    }
    const int64_t blocks = (n + KM_ROWS - 1) / KM_ROWS;
    double* part = reinterpret_cast<double*>(ws);
    const dim3 grid((unsigned)blocks);
    const int d4 = d / 4;
#define KM_UPDATE(G, C) hipLaunchKernelGGL((kmeans_seed_update_kernel<G, C>), grid, dim3(256), 0, st, x, n, d, (const int64_t*)picks, j, mind, part)
    if (d4 <= 1) KM_UPDATE(1, 1);
    else if (d4 <= 2) KM_UPDATE(2, 1);
    else if (d4 <= 4) KM_UPDATE(4, 1);
    else if (d4 <= 8) KM_UPDATE(8, 1);
    else if (d4 <= 16) KM_UPDATE(16, 1);
    else if (d4 <= 32) KM_UPDATE(32, 1);
    else if (d4 <= 64) KM_UPDATE(64, 1);
    else if (d4 <= 128) KM_UPDATE(64, 2);
    else if (d4 <= 192) KM_UPDATE(64, 3);
    else KM_UPDATE(64, 4);
#undef KM_UPDATE
    VQK_CHECK_LAUNCH();
    hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3(1), dim3(256), 0, st, (const double*)part, blocks, n, (const float*)mind, u, j,
                       picks, total);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_kmeans_update_f32(const float* counts, const float* sums, int k, int d, float* centres, float* moved, void* stream) {
    VQK_REQUIRE(counts && sums && centres, VQK_ERR_ARG);
    VQK_REQUIRE(k >= 1 && d >= 4 && (d % 4) == 0, VQK_ERR_SHAPE);
    VQK_REQUIRE(vqk_aligned16(centres), VQK_ERR_ALIGN);
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, vqk_stream(stream), counts, sums, k, d, centres,
                       moved);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // extern "C"
