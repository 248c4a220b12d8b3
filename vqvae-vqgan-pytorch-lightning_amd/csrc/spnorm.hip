// Spatially conditioned GroupNorm (MoVQ / diffusers SpatialNorm), NHWC:
//   u = GroupNorm_32(f) * gamma + beta  (unbiased variance, as norm.hip);  out = act(u * M[n, i / r, j / r, :] + A[n, i / r, j / r, :])
// with the modulation tables M, A [N][h][w][C] fp32 at the LATENT resolution, r = H / h = W / w a power of two.
// Backward (g = dy * act'(p), xh the normalised value, m = (C / 32) * H * W):
//   P = sum over the r x r block of g,  Q = sum over the r x r block of g * xh
//   dA = P,  dM = gamma * Q + beta * P,  dbeta[c] = sum M * P,  dgamma[c] = sum M * Q
//   S1[n][grp] = sum gamma * M * P,  S2[n][grp] = sum gamma * M * Q,  df = rstd * (g * M * gamma - S1 / m - xh * S2 / (m - 1))
// Thread mapping: as in norm.hip a thread owns one 16-byte channel vector slot; the block's 256 threads form `rows` pixel rows
// (a power of two).  The r x r block of a latent pixel is owned by ONE workgroup: `teams` latent pixels side by side when
// r * r < rows, else one at a time with r * r / rows vectors per thread; a thread keeps the M / A vectors of its latent pixel in
// registers for all of them (the other rows of the block re-read the same lines from L1 / L2).  No float atomics anywhere:
// per-block partial sums are stored and added in a fixed order, the bits are the same on every run in every mode.
#include "common.h"

namespace {

constexpr int kGroups = 32;

struct SpGeo {
    int h, w, lr;             // latent map, log2 r
    int c, cpg;               // channels, channels per group
    int rows;                 // pixel rows of a block (power of two, rows * (c / V) <= 256)
    int teams, vpi, it;       // latent pixels per iteration, vectors per thread and latent pixel, iterations per block
    int nblk;                 // blocks per sample = ceil(h * w / (teams * it))
};

__device__ __forceinline__ float sp_sigmoid(float y) { return __builtin_amdgcn_rcpf(1.0f + __expf(-y)); }

template <int V> __device__ __forceinline__ void sp_ld_f32(const float* p, float (&o)[V]) {
#pragma unroll
    for (int i = 0; i < V; i += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + i);
        o[i] = v[0]; o[i + 1] = v[1]; o[i + 2] = v[2]; o[i + 3] = v[3];
    }
}

// first map pixel (flat index over [N][H][W]) of latent pixel lp of sample n
__device__ __forceinline__ int64_t sp_base(const SpGeo& g, int n, int lp) {
    const int a = lp / g.w, b = lp - a * g.w;
    const int64_t wm = (int64_t)g.w << g.lr;
    return ((int64_t)n * ((int64_t)g.h << g.lr) + ((int64_t)a << g.lr)) * wm + ((int64_t)b << g.lr);
}
// pixel `wi` (row-major in the r x r block) relative to sp_base
__device__ __forceinline__ int64_t sp_in_block(const SpGeo& g, int wi) {
    return (int64_t)(wi >> g.lr) * ((int64_t)g.w << g.lr) + (wi & ((1 << g.lr) - 1));
}

// per-thread double partials [2][V] -> col[2][c] double, rows added in row order
template <int V>
__device__ __forceinline__ void sp_block_colsum(const double (&p0)[V], const double (&p1)[V], bool active, int prow, int slot,
                                                int c, int rows, double* part, double* col) {
    if (active) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            part[(prow * 2 + 0) * c + slot * V + i] = p0[i];
            part[(prow * 2 + 1) * c + slot * V + i] = p1[i];
        }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 2 * c; o += 256) {
        const int j = o / c, ch = o - j * c;
        double a = 0.0;
        for (int r = 0; r < rows; ++r) a += part[(r * 2 + j) * c + ch];
        col[o] = a;
    }
    __syncthreads();
}

// statistics: a block sums a contiguous run of pixels; gpart[((n * nblk + blk) * 32 + grp) * 2] = {sum, sum of squares}
template <typename T>
__global__ __launch_bounds__(256) void spnorm_stats_kernel(const T* __restrict__ f, int64_t hw, int c, int cpg, int rows, int ppb,
                                                           double* __restrict__ gpart) {
    constexpr int V = Vec16<T>::N;
    __shared__ double part[2 * 256 * V];
    __shared__ double col[2 * 512];
    const int vpp = c / V, slot = threadIdx.x % vpp, prow = threadIdx.x / vpp;
    const bool active = prow < rows;
    const int n = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * ppb, p1 = min(hw, p0 + ppb);
    double ds[V], dss[V];
    float s[V], ss[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { ds[i] = 0.0; dss[i] = 0.0; s[i] = 0.f; ss[i] = 0.f; }
    if (active) {
        const T* base = f + (int64_t)n * hw * c + slot * V;
        int cnt = 0;
#pragma unroll 4
        for (int64_t p = p0 + prow; p < p1; p += rows) {
            float v[V];
            Vec16<T>::load(base + p * c, v);
#pragma unroll
            for (int i = 0; i < V; ++i) { s[i] += v[i]; ss[i] = __fmaf_rn(v[i], v[i], ss[i]); }
            if (++cnt == 16) {                                       // fp32 runs of 16 terms, then double
                cnt = 0;
#pragma unroll
                for (int i = 0; i < V; ++i) { ds[i] += (double)s[i]; dss[i] += (double)ss[i]; s[i] = 0.f; ss[i] = 0.f; }
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) { ds[i] += (double)s[i]; dss[i] += (double)ss[i]; }
    }
    sp_block_colsum<V>(ds, dss, active, prow, slot, c, rows, part, col);
    for (int g = threadIdx.x; g < kGroups; g += 256) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < cpg; ++i) { a += col[g * cpg + i]; b += col[c + g * cpg + i]; }
        double* q = gpart + (((int64_t)n * gridDim.x + blockIdx.x) * kGroups + g) * 2;
        q[0] = a; q[1] = b;
    }
}

// one thread per (sample, group): the blocks' partials in block order -> (mean, rstd), the arithmetic of norm.hip's finalize
__global__ void spnorm_stats_finish_kernel(const double* __restrict__ gpart, int nblk, int total, double m, float eps,
                                           float* __restrict__ stats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int n = i / kGroups, g = i - n * kGroups;
    double s = 0.0, ss = 0.0;
    for (int k = 0; k < nblk; ++k) {
        const double* q = gpart + (((int64_t)n * nblk + k) * kGroups + g) * 2;
        s += q[0]; ss += q[1];
    }
    const double mean = s / m;
    double var = (ss - s * mean) / (m - 1.0);          // unbiased
    if (var < 0.0) var = 0.0;
    stats[2 * i] = (float)mean;
    stats[2 * i + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

// MODE 0: out = act(u * M + A);  MODE 1 (sweep 2 of the backward): out = df, `dy` and the finished group sums gfin are read
template <typename T, bool SILU, int MODE>
__global__ __launch_bounds__(256) void spnorm_stream_kernel(const T* __restrict__ f, const float* __restrict__ stats,
                                                            const float* __restrict__ mt, const float* __restrict__ at,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const T* __restrict__ dy, const float* __restrict__ gfin,
                                                            T* __restrict__ out, SpGeo g) {
    constexpr int V = Vec16<T>::N;
    const int vpp = g.c / V, slot = threadIdx.x % vpp, prow = threadIdx.x / vpp;
    if (prow >= g.rows) return;                                      // (no barrier in this kernel)
    const int n = blockIdx.y, hwl = g.h * g.w;
    float mean[V], rstd[V], gam[V], bet[V], c1[V], c2[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int ch = slot * V + i, grp = ch / g.cpg;
        mean[i] = stats[((int64_t)n * kGroups + grp) * 2]; rstd[i] = stats[((int64_t)n * kGroups + grp) * 2 + 1];
        gam[i] = gamma[ch]; bet[i] = beta[ch];
        if constexpr (MODE == 1) { c1[i] = gfin[((int64_t)n * kGroups + grp) * 2]; c2[i] = gfin[((int64_t)n * kGroups + grp) * 2 + 1]; }
        else { c1[i] = 0.f; c2[i] = 0.f; }
    }
    const int team = prow >> (2 * g.lr), w0 = prow & ((1 << (2 * g.lr)) - 1);
    for (int it = 0; it < g.it; ++it) {
        const int lp = ((int)blockIdx.x * g.it + it) * g.teams + team;
        if (lp >= hwl) break;
        float mv[V], av[V];
        const int64_t toff = ((int64_t)n * hwl + lp) * g.c + slot * V;
        sp_ld_f32<V>(mt + toff, mv);
        sp_ld_f32<V>(at + toff, av);
        const int64_t base = sp_base(g, n, lp);
#pragma unroll 4
        for (int i = 0; i < g.vpi; ++i) {
            const int64_t off = (base + sp_in_block(g, w0 + i * g.rows)) * g.c + slot * V;
            float v[V], d[V] = {};
            Vec16<T>::load(f + off, v);
            if constexpr (MODE == 1) Vec16<T>::load(dy + off, d);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float xh = (v[k] - mean[k]) * rstd[k];
                const float u = __fmaf_rn(xh, gam[k], bet[k]);
                const float p = __fmaf_rn(u, mv[k], av[k]);
                if constexpr (MODE == 0) {
                    v[k] = SILU ? p * sp_sigmoid(p) : p;
                } else {
                    float gg = d[k];
                    if (SILU) { const float sg = sp_sigmoid(p); gg *= sg * (1.0f + p * (1.0f - sg)); }
                    v[k] = rstd[k] * (gg * mv[k] * gam[k] - c1[k] - xh * c2[k]);
                }
            }
            Vec16<T>::store_nt(out + off, v);
        }
    }
}

// sweep 1 of the backward: dM, dA (plain stores, the block owns its latent pixels), the block's group sums S1 / S2 to
// gpart[((n * nblk + blk) * 32 + grp) * 2] and its channel sums to cpart[(n * nblk + blk) * 2c + {0: dbeta, c: dgamma} + ch]
template <typename T, bool SILU>
__global__ __launch_bounds__(256) void spnorm_bwd_reduce_kernel(const T* __restrict__ f, const float* __restrict__ stats,
                                                                const float* __restrict__ mt, const float* __restrict__ at,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const T* __restrict__ dy, float* __restrict__ dm,
                                                                float* __restrict__ da, double* __restrict__ gpart,
                                                                float* __restrict__ cpart, SpGeo g) {
    constexpr int V = Vec16<T>::N;
    __shared__ float pq[2 * 256 * V];            // [rows][2][c]: the threads' P / Q partials of the current latent pixels
    __shared__ float outl[2 * 256 * V];          // [teams][2][c]: M * P, M * Q of the current latent pixels
    __shared__ double col[2 * 512];
    const int vpp = g.c / V, slot = threadIdx.x % vpp, prow = threadIdx.x / vpp, c = g.c;
    const bool active = prow < g.rows;
    const int n = blockIdx.y, hwl = g.h * g.w;
    float mean[V], rstd[V], gam[V], bet[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int ch = slot * V + i, grp = ch / g.cpg;
        mean[i] = stats[((int64_t)n * kGroups + grp) * 2]; rstd[i] = stats[((int64_t)n * kGroups + grp) * 2 + 1];
        gam[i] = gamma[ch]; bet[i] = beta[ch];
    }
    const int team = prow >> (2 * g.lr), w0 = prow & ((1 << (2 * g.lr)) - 1);
    const int r2min = g.rows / g.teams;          // rows that share a latent pixel
    double ca[2] = {0.0, 0.0}, cb[2] = {0.0, 0.0};
    for (int it = 0; it < g.it; ++it) {          // (uniform trip count: the barriers below are reached by every thread)
        const int lp0 = ((int)blockIdx.x * g.it + it) * g.teams;
        const int lp = lp0 + team;
        double dp[V], dq[V];
#pragma unroll
        for (int k = 0; k < V; ++k) { dp[k] = 0.0; dq[k] = 0.0; }
        if (active && lp < hwl) {
            float mv[V], av[V], ps[V], qs[V];
            const int64_t toff = ((int64_t)n * hwl + lp) * c + slot * V;
            sp_ld_f32<V>(mt + toff, mv);
            sp_ld_f32<V>(at + toff, av);
#pragma unroll
            for (int k = 0; k < V; ++k) { ps[k] = 0.f; qs[k] = 0.f; }
            const int64_t base = sp_base(g, n, lp);
            int cnt = 0;
#pragma unroll 4
            for (int i = 0; i < g.vpi; ++i) {
                const int64_t off = (base + sp_in_block(g, w0 + i * g.rows)) * c + slot * V;
                float v[V], d[V];
                Vec16<T>::load(f + off, v);
                Vec16<T>::load(dy + off, d);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float xh = (v[k] - mean[k]) * rstd[k];
                    float gg = d[k];
                    if (SILU) {
                        const float p = __fmaf_rn(__fmaf_rn(xh, gam[k], bet[k]), mv[k], av[k]);
                        const float sg = sp_sigmoid(p);
                        gg *= sg * (1.0f + p * (1.0f - sg));
                    }
                    ps[k] += gg;
                    qs[k] = __fmaf_rn(gg, xh, qs[k]);
                }
                if (++cnt == 16) {                                   // fp32 runs of 16 terms, then double
                    cnt = 0;
#pragma unroll
                    for (int k = 0; k < V; ++k) { dp[k] += (double)ps[k]; dq[k] += (double)qs[k]; ps[k] = 0.f; qs[k] = 0.f; }
                }
            }
#pragma unroll
            for (int k = 0; k < V; ++k) { dp[k] += (double)ps[k]; dq[k] += (double)qs[k]; }
        }
        if (active) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                pq[(prow * 2 + 0) * c + slot * V + k] = (float)dp[k];
                pq[(prow * 2 + 1) * c + slot * V + k] = (float)dq[k];
            }
        }
        __syncthreads();
        for (int o = threadIdx.x; o < g.teams * c; o += 256) {       // one thread per (latent pixel, channel): rows in row order
            const int t = o / c, ch = o - t * c;
            double ps = 0.0, qs = 0.0;
            for (int k = 0; k < r2min; ++k) {
                ps += (double)pq[((t * r2min + k) * 2 + 0) * c + ch];
                qs += (double)pq[((t * r2min + k) * 2 + 1) * c + ch];
            }
            float mp = 0.f, mq = 0.f;
            if (lp0 + t < hwl) {
                const int64_t idx = ((int64_t)n * hwl + lp0 + t) * c + ch;
                const float mval = mt[idx];
                da[idx] = (float)ps;
                dm[idx] = (float)((double)gamma[ch] * qs + (double)beta[ch] * ps);
                mp = (float)((double)mval * ps); mq = (float)((double)mval * qs);
            }
            outl[(t * 2 + 0) * c + ch] = mp;
            outl[(t * 2 + 1) * c + ch] = mq;
        }
        __syncthreads();
        for (int ch = threadIdx.x, k = 0; ch < c; ch += 256, ++k)
            for (int t = 0; t < g.teams; ++t) { ca[k] += (double)outl[(t * 2 + 0) * c + ch]; cb[k] += (double)outl[(t * 2 + 1) * c + ch]; }
    }
    for (int ch = threadIdx.x, k = 0; ch < c; ch += 256, ++k) { col[ch] = ca[k]; col[c + ch] = cb[k]; }
    __syncthreads();
    float* cp = cpart + ((int64_t)n * gridDim.x + blockIdx.x) * 2 * c;
    for (int o = threadIdx.x; o < 2 * c; o += 256) cp[o] = (float)col[o];
    for (int grp = threadIdx.x; grp < kGroups; grp += 256) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = 0; i < g.cpg; ++i) {
            const int ch = grp * g.cpg + i;
            s1 += col[ch] * (double)gamma[ch];
            s2 += col[c + ch] * (double)gamma[ch];
        }
        double* q = gpart + (((int64_t)n * gridDim.x + blockIdx.x) * kGroups + grp) * 2;
        q[0] = s1; q[1] = s2;
    }
}

// channel partials cpart[R][2c] -> part2[S][2c]: segment seg adds its rows in a fixed order (4 waves interleaved, then wave order)
__global__ __launch_bounds__(256) void spnorm_chan_partial_kernel(const float* __restrict__ cpart, int64_t nrows, int c2, int rps,
                                                                  double* __restrict__ part2) {
    __shared__ double sh[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int colx = blockIdx.x * 64 + lane, seg = blockIdx.y;
    const int64_t r0 = (int64_t)seg * rps, r1 = min(nrows, r0 + rps);
    double a = 0.0;
    if (colx < c2) {
#pragma unroll 4
        for (int64_t r = r0 + wv; r < r1; r += 4) a += (double)cpart[r * c2 + colx];
    }
    sh[wv][lane] = a;
    __syncthreads();
    if (wv == 0 && colx < c2) part2[(int64_t)seg * c2 + colx] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

// thread t < 2c: the segments in order, ADDED onto dbeta / dgamma (one writer per element);  thread t < N * 32: the blocks' group
// sums in block order -> gfin = {S1 / m, S2 / (m - 1)}
__global__ void spnorm_bwd_finish_kernel(const double* __restrict__ part2, int nseg, int c, float* __restrict__ dgamma,
                                         float* __restrict__ dbeta, const double* __restrict__ gpart, int nblk, int total, double m,
                                         float* __restrict__ gfin) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 2 * c) {
        double a = 0.0;
        for (int s = 0; s < nseg; ++s) a += part2[(int64_t)s * 2 * c + t];
        if (t < c) dbeta[t] += (float)a; else dgamma[t - c] += (float)a;
    }
    if (t < total) {
        const int n = t / kGroups, grp = t - n * kGroups;
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < nblk; ++k) {
            const double* q = gpart + (((int64_t)n * nblk + k) * kGroups + grp) * 2;
            s1 += q[0]; s2 += q[1];
        }
        gfin[2 * t] = (float)(s1 / m);
        gfin[2 * t + 1] = (float)(s2 / (m - 1.0));
    }
}

struct SpPlan {
    SpGeo g;
    int64_t hw;               // map pixels per sample
    int sppb, snblk;          // statistics pass: pixels per block, blocks per sample
    int nseg, rps;            // channel finish: segments, rows per segment
    int64_t off_gfin, off_part2, off_cpart, bytes;      // workspace layout (gpart at 0)
};

int sp_plan(int dtype, int n, int h, int w, int r, int c, SpPlan* p) {
    VQK_REQUIRE(dtype == VQK_F32 || dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0 && c > 0 && c <= 512 && c % kGroups == 0, VQK_ERR_SHAPE);
    int lr = 0;
    while ((1 << lr) < r) ++lr;
    VQK_REQUIRE(r >= 1 && r <= 32 && (1 << lr) == r, VQK_ERR_SHAPE);
    VQK_REQUIRE((int64_t)h * w < (1 << 24) && ((int64_t)h * r) * ((int64_t)w * r) < ((int64_t)1 << 31), VQK_ERR_SHAPE);
    const int v = dtype == VQK_F32 ? 4 : 8, vpp = c / v;
    SpGeo& g = p->g;
    g.h = h; g.w = w; g.lr = lr; g.c = c; g.cpg = c / kGroups;
    g.rows = 1;
    while (g.rows * 2 * vpp <= 256) g.rows *= 2;
    const int r2 = r * r, hwl = h * w;
    g.teams = r2 >= g.rows ? 1 : g.rows / r2;
    g.vpi = r2 >= g.rows ? r2 / g.rows : 1;
    g.it = g.vpi >= 32 ? 1 : 32 / g.vpi;
    // no more iterations than the sample has latent pixels for, and blocks enough to fill the device
    while (g.it > 1 && (int64_t)(g.it / 2) * g.teams >= hwl) g.it /= 2;
    while (g.it > 1 && (int64_t)((hwl + g.it * g.teams - 1) / (g.it * g.teams)) * n < 2048) g.it /= 2;
    g.nblk = (hwl + g.it * g.teams - 1) / (g.it * g.teams);
    p->hw = (int64_t)hwl * r2;
    int64_t ppb = (int64_t)g.rows * 16;
    if ((p->hw + ppb - 1) / ppb > 512) {
        ppb = (p->hw + 511) / 512;
        ppb = (ppb + g.rows - 1) / g.rows * g.rows;
    }
    p->sppb = (int)ppb;
    p->snblk = (int)((p->hw + ppb - 1) / ppb);
    const int64_t nrows = (int64_t)n * g.nblk;
    p->nseg = (int)(nrows / 64 < 1 ? 1 : (nrows / 64 > 32 ? 32 : nrows / 64));
    p->rps = (int)((nrows + p->nseg - 1) / p->nseg);
    const int64_t nb = g.nblk > p->snblk ? g.nblk : p->snblk;
    int64_t o = (int64_t)n * nb * kGroups * 2 * sizeof(double);          // gpart (forward: snblk, backward: nblk blocks per sample)
    p->off_part2 = o; o += (int64_t)p->nseg * 2 * c * sizeof(double);
    p->off_gfin = o;  o += (int64_t)n * kGroups * 2 * sizeof(float);
    o = (o + 15) / 16 * 16;
    p->off_cpart = o; o += nrows * 2 * c * sizeof(float);
    p->bytes = o;
    return VQK_OK;
}

}  // namespace

extern "C" {

int64_t vqk_spnorm_ws_bytes(int dtype, int n, int h, int w, int r, int c) {
    SpPlan p;
    const int rc = sp_plan(dtype, n, h, w, r, c, &p);
    return rc ? rc : p.bytes;
}

int vqk_spnorm_forward(int dtype, const void* f, const float* m, const float* a, const float* gamma, const float* beta, void* out,
                       float* stats, void* ws, int64_t ws_bytes, int n, int h, int w, int r, int c, int groups, float eps, int silu,
                       void* stream) {
    VQK_REQUIRE(f && m && a && gamma && beta && out && stats && ws, VQK_ERR_ARG);
    VQK_REQUIRE(groups == kGroups, VQK_ERR_SHAPE);
    SpPlan p;
    const int rc = sp_plan(dtype, n, h, w, r, c, &p);
    if (rc) return rc;
    VQK_REQUIRE(vqk_aligned16(f) && vqk_aligned16(out) && vqk_aligned16(m) && vqk_aligned16(a) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= p.bytes, VQK_ERR_WORKSPACE);
    hipStream_t st = vqk_stream(stream);
    double* gpart = reinterpret_cast<double*>(ws);
    const dim3 sgrid((unsigned)p.snblk, (unsigned)n), grid((unsigned)p.g.nblk, (unsigned)n);
    if (dtype == VQK_F32) hipLaunchKernelGGL(spnorm_stats_kernel<float>, sgrid, dim3(256), 0, st, (const float*)f, p.hw, c, p.g.cpg, p.g.rows, p.sppb, gpart);
    else hipLaunchKernelGGL(spnorm_stats_kernel<bf16_raw>, sgrid, dim3(256), 0, st, (const bf16_raw*)f, p.hw, c, p.g.cpg, p.g.rows, p.sppb, gpart);
    const int total = n * kGroups;
    hipLaunchKernelGGL(spnorm_stats_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, st, gpart, p.snblk, total,
                       (double)p.hw * p.g.cpg, eps, stats);
#define VQK_SP_APPLY(T, S) hipLaunchKernelGGL((spnorm_stream_kernel<T, S, 0>), grid, dim3(256), 0, st, (const T*)f, stats, m, a, gamma, beta, \
                                              (const T*)nullptr, (const float*)nullptr, (T*)out, p.g)
    if (dtype == VQK_F32) { if (silu) VQK_SP_APPLY(float, true); else VQK_SP_APPLY(float, false); }
    else { if (silu) VQK_SP_APPLY(bf16_raw, true); else VQK_SP_APPLY(bf16_raw, false); }
#undef VQK_SP_APPLY
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_spnorm_backward(int dtype, const void* f, const float* stats, const float* m, const float* a, const float* gamma,
                        const float* beta, const void* dy, void* df, float* dm, float* da, float* dgamma, float* dbeta, void* ws,
                        int64_t ws_bytes, int n, int h, int w, int r, int c, int groups, int silu, void* stream) {
    VQK_REQUIRE(f && stats && m && a && gamma && beta && dy && df && dm && da && dgamma && dbeta && ws, VQK_ERR_ARG);
    VQK_REQUIRE(groups == kGroups, VQK_ERR_SHAPE);
    SpPlan p;
    const int rc = sp_plan(dtype, n, h, w, r, c, &p);
    if (rc) return rc;
    VQK_REQUIRE(vqk_aligned16(f) && vqk_aligned16(dy) && vqk_aligned16(df) && vqk_aligned16(m) && vqk_aligned16(a) && vqk_aligned16(ws),
                VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= p.bytes, VQK_ERR_WORKSPACE);
    hipStream_t st = vqk_stream(stream);
    char* wsb = reinterpret_cast<char*>(ws);
    double* gpart = reinterpret_cast<double*>(wsb);
    double* part2 = reinterpret_cast<double*>(wsb + p.off_part2);
    float* gfin = reinterpret_cast<float*>(wsb + p.off_gfin);
    float* cpart = reinterpret_cast<float*>(wsb + p.off_cpart);
    const dim3 grid((unsigned)p.g.nblk, (unsigned)n);
#define VQK_SP_RED(T, S) hipLaunchKernelGGL((spnorm_bwd_reduce_kernel<T, S>), grid, dim3(256), 0, st, (const T*)f, stats, m, a, gamma, beta, \
                                            (const T*)dy, dm, da, gpart, cpart, p.g)
    if (dtype == VQK_F32) { if (silu) VQK_SP_RED(float, true); else VQK_SP_RED(float, false); }
    else { if (silu) VQK_SP_RED(bf16_raw, true); else VQK_SP_RED(bf16_raw, false); }
#undef VQK_SP_RED
    const int64_t nrows = (int64_t)n * p.g.nblk;
    hipLaunchKernelGGL(spnorm_chan_partial_kernel, dim3((unsigned)((2 * c + 63) / 64), (unsigned)p.nseg), dim3(256), 0, st, cpart, nrows,
                       2 * c, p.rps, part2);
    const int total = n * kGroups, fin = total > 2 * c ? total : 2 * c;
    hipLaunchKernelGGL(spnorm_bwd_finish_kernel, dim3((fin + 255) / 256), dim3(256), 0, st, part2, p.nseg, c, dgamma, dbeta, gpart,
                       p.g.nblk, total, (double)p.hw * p.g.cpg, gfin);
#define VQK_SP_DF(T, S) hipLaunchKernelGGL((spnorm_stream_kernel<T, S, 1>), grid, dim3(256), 0, st, (const T*)f, stats, m, a, gamma, beta, \
                                           (const T*)dy, gfin, (T*)df, p.g)
    if (dtype == VQK_F32) { if (silu) VQK_SP_DF(float, true); else VQK_SP_DF(float, false); }
    else { if (silu) VQK_SP_DF(bf16_raw, true); else VQK_SP_DF(bf16_raw, false); }
#undef VQK_SP_DF
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // extern "C"
