// ------------------------------------------------------------------------------------------------
// Running statistics of a training run (include/vqk.h: vqk_scalar_accum / vqk_arena_stats; scalarlog.py).
//
// The reference logs the epoch means of its losses through Lightning's self.log(..., on_epoch=True, sync_dist=True)
// (vqvae/model.py:229-230, :277-286, :342-348, :365-366).  Here the step's scalars stay on the device, so the epoch sums are
// kept on the device too:
//   scalar_accum_kernel   up to 16 device scalars (fp32 / bf16) into fp64 epoch accumulators, one thread per scalar.  The source
//                         POINTERS are kernel arguments: an eager step produces new tensors every step and a device table would
//                         cost an upload per step.  Launches arrive in stream order, so a slot's sum is a fixed-order fp64 sum;
//                         (double)x * w is exact (24 bits x an integer below 2^20), so the sum has the bits of a float64 host
//                         loop over the same values whether or not the compiler fuses the multiply into the add.
//   arena_stats_kernel    one read-only pass over a FlatAdamW gradient arena: per parameter group sum x^2, max |x| over the
//                         finite x = (double)g * (double)scale and the exact count of non-finite elements.  Every thread sums
//                         its elements in fp64 (one rounding per square -- this file is compiled with -ffp-contract=off, so the
//                         terms are the ones a float64 reference squares -- and one per addition), a wave folds its lanes by
//                         shuffles, a block its waves through LDS, and the block's partial goes to the caller's workspace.
//   arena_finish_kernel   ONE block adds the per-block partials in index order, writes the step's out[G+1][3] and folds it into
//                         the epoch accumulators.  No float atomics, no hand-off between blocks inside a launch: the same bits
//                         every run.
// Segments of the arena are binary-searched and cached per thread exactly as adamw_kernel (optim.hip) does it.
// ------------------------------------------------------------------------------------------------
#include "common.h"

#pragma STDC FP_CONTRACT OFF

namespace {

struct ScalarArgs {
    const void* src[VQK_SCALAR_MAX];
    double w[VQK_SCALAR_MAX];
    int dtype[VQK_SCALAR_MAX];
    int slot[VQK_SCALAR_MAX];
    int n;
};

__global__ __launch_bounds__(64) void scalar_accum_kernel(const ScalarArgs a, double* __restrict__ acc) {
    const int k = threadIdx.x;
    if (k >= a.n) return;
    const float xf = a.dtype[k] == VQK_BF16 ? bf16_to_f32(*static_cast<const bf16_raw*>(a.src[k])) : *static_cast<const float*>(a.src[k]);
    const bool finite = (__float_as_uint(xf) & 0x7f800000u) != 0x7f800000u;
    const double x = (double)xf;
    double* s = acc + (int64_t)a.slot[k] * VQK_SCALAR_SLOT_DOUBLES;
    s[0] += x * a.w[k];                  // non-finite values enter the sum: the mean turns NaN as Lightning's would
    s[1] += a.w[k];
    s[2] = x;                            // last
    if (x < s[3]) s[3] = x;              // min / max: a NaN compares false and is skipped (it is counted below)
    if (x > s[4]) s[4] = x;
    if (!finite) s[5] += 1.0;
    s[6] += 1.0;                         // calls
}

constexpr int AS_THREADS = 256;
constexpr int AS_CHUNK = AS_THREADS * 4 * 8;          // elements a block owns per grid stride (adamw_kernel's chunk)
constexpr int AS_MAX_BLOCKS = 256 * 8;                // memory-bound sizing: 256 CUs x 8 blocks, the rest by grid stride

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const double o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

__global__ __launch_bounds__(AS_THREADS) void arena_stats_kernel(const float* __restrict__ g, int64_t n,
                                                                 const int64_t* __restrict__ seg_end,
                                                                 const int32_t* __restrict__ seg_group, int nseg, int ngroups,
                                                                 float scale, int vec_ok, double* __restrict__ part) {
    // a thread's sums per group: its own column of the three tables (no other thread touches it before the barrier)
    __shared__ double sh_sq[VQK_ARENA_MAX_GROUPS][AS_THREADS];
    __shared__ double sh_mx[VQK_ARENA_MAX_GROUPS][AS_THREADS];
    __shared__ unsigned sh_nf[VQK_ARENA_MAX_GROUPS][AS_THREADS];          // (a thread meets fewer than 2^32 elements: numel <= 2^38)
    __shared__ double red[VQK_ARENA_MAX_GROUPS][3][AS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = 0; q < ngroups; ++q) { sh_sq[q][tid] = 0.0; sh_mx[q][tid] = 0.0; sh_nf[q][tid] = 0u; }

    const double sc = (double)scale;
    int64_t s_lo = 0, s_hi = -1;                         // cached segment [s_lo, s_hi) and its group
    int grp = -1;
    int cur = -1;                                        // group of the running sums below
    double sq = 0.0, mx = 0.0;
    unsigned nf = 0u;
    auto lookup = [&](int64_t i) {
        if (i >= s_lo && i < s_hi) return;
        int lo = 0, hi = nseg - 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (seg_end[mid] > i) hi = mid; else lo = mid + 1; }
        grp = seg_group[lo];
        s_lo = lo ? seg_end[lo - 1] : 0;
        s_hi = seg_end[lo];
        if (i >= s_hi || grp >= ngroups) grp = -1;       // beyond the last segment end / an id the caller did not size for
    };
    auto flush = [&]() {
        if (cur >= 0) { sh_sq[cur][tid] += sq; sh_mx[cur][tid] = mx > sh_mx[cur][tid] ? mx : sh_mx[cur][tid]; sh_nf[cur][tid] += nf; }
        sq = 0.0; mx = 0.0; nf = 0u;
    };
    auto one = [&](float gf) {
        if (grp < 0) return;                             // padding: read, never used
        if (grp != cur) { flush(); cur = grp; }
        if ((__float_as_uint(gf) & 0x7f800000u) == 0x7f800000u) { nf += 1u; return; }
        const double x = (double)gf * sc;                // exact: 24 x 24 bits
        const double ax = fabs(x);
        sq += x * x;
        mx = ax > mx ? ax : mx;
    };

    const int64_t nchunks = (n + AS_CHUNK - 1) / AS_CHUNK;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t base = chunk * AS_CHUNK;
        if (vec_ok && base + AS_CHUNK <= n) {
            f32x4 gv[8];                                 // the chunk's eight loads in flight before the first is used
#pragma unroll
            for (int it = 0; it < 8; ++it)               // (plain loads: the optimizer step reads g next)
                gv[it] = *reinterpret_cast<const f32x4*>(g + base + it * (AS_THREADS * 4) + tid * 4);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int64_t i = base + it * (AS_THREADS * 4) + tid * 4;
                lookup(i);
                if (i + 4 <= s_hi) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) one(gv[it][e]);
                } else {                                 // a tensor's end inside the vector (its padding follows)
#pragma unroll
                    for (int e = 0; e < 4; ++e) { lookup(i + e); one(gv[it][e]); }
                }
            }
        } else {                                         // the arena's tail, or an arena that is not 16-byte aligned
            for (int it = 0; it < 8; ++it) {
                const int64_t i = base + it * (AS_THREADS * 4) + tid * 4;
                for (int e = 0; e < 4 && i + e < n; ++e) { lookup(i + e); one(g[i + e]); }
            }
        }
    }
    flush();
    // own column -> wave (shuffles) -> block (LDS): a fixed tree, the same bits every run
    for (int q = 0; q < ngroups; ++q) {
        const double a = wave_sum_f64(sh_sq[q][tid]), b = wave_max_f64(sh_mx[q][tid]), c = wave_sum_f64((double)sh_nf[q][tid]);
        if (lane == 0) { red[q][0][wave] = a; red[q][1][wave] = b; red[q][2][wave] = c; }
    }
    __syncthreads();
    if (tid < ngroups) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int w = 0; w < AS_THREADS / 64; ++w) {
            a += red[tid][0][w]; b = red[tid][1][w] > b ? red[tid][1][w] : b; c += red[tid][2][w];
        }
        double* p = part + ((int64_t)blockIdx.x * ngroups + tid) * 3;
        p[0] = a; p[1] = b; p[2] = c;
    }
}

// out[q] = {sumsq, maxabs, nonfinite} for q < G and out[G] = the whole arena (the groups added in id order);
// acc[q] = {sum of norms, max norm, max maxabs, sum of nonfinite, steps}
__global__ __launch_bounds__(AS_THREADS) void arena_finish_kernel(const double* __restrict__ part, int nblocks, int ngroups,
                                                                  double* __restrict__ out, double* __restrict__ acc) {
    __shared__ double red[VQK_ARENA_MAX_GROUPS][3][AS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = 0; q < ngroups; ++q) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int blk = tid; blk < nblocks; blk += AS_THREADS) {           // index order per thread, then the fixed tree
            const double* p = part + ((int64_t)blk * ngroups + q) * 3;
            a += p[0]; b = p[1] > b ? p[1] : b; c += p[2];
        }
        a = wave_sum_f64(a); b = wave_max_f64(b); c = wave_sum_f64(c);
        if (lane == 0) { red[q][0][wave] = a; red[q][1][wave] = b; red[q][2][wave] = c; }
    }
    __syncthreads();
    if (tid == 0) {
        double ta = 0.0, tb = 0.0, tc = 0.0;
        for (int q = 0; q <= ngroups; ++q) {
            double a = 0.0, b = 0.0, c = 0.0;
            if (q < ngroups) {
                for (int w = 0; w < AS_THREADS / 64; ++w) {
                    a += red[q][0][w]; b = red[q][1][w] > b ? red[q][1][w] : b; c += red[q][2][w];
                }
                ta += a; tb = b > tb ? b : tb; tc += c;
            } else {
                a = ta; b = tb; c = tc;
            }
            out[q * 3 + 0] = a; out[q * 3 + 1] = b; out[q * 3 + 2] = c;
            if (acc) {
                double* e = acc + q * VQK_ARENA_ACC_DOUBLES;
                const double norm = sqrt(a);
                e[0] += norm;
                e[1] = norm > e[1] ? norm : e[1];
                e[2] = b > e[2] ? b : e[2];
                e[3] += c;
                e[4] += 1.0;
            }
        }
    }
}

int arena_blocks(int64_t numel) {
    int64_t b = (numel + AS_CHUNK - 1) / AS_CHUNK;
    if (b < 1) b = 1;
    return (int)(b < AS_MAX_BLOCKS ? b : AS_MAX_BLOCKS);
}

}  // namespace

extern "C" int vqk_scalar_accum(const void* const* src, const int* dtype, const double* weight, const int* slot, int n, double* acc,
                                int nslots, void* stream) {
    VQK_REQUIRE(src && dtype && weight && slot && acc, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 1 && n <= VQK_SCALAR_MAX && nslots >= 1, VQK_ERR_SHAPE);
    VQK_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7u) == 0, VQK_ERR_ALIGN);
    ScalarArgs a;
    a.n = n;
    for (int k = 0; k < n; ++k) {
        VQK_REQUIRE(src[k], VQK_ERR_ARG);
        VQK_REQUIRE(dtype[k] == VQK_F32 || dtype[k] == VQK_BF16, VQK_ERR_DTYPE);
        VQK_REQUIRE((reinterpret_cast<uintptr_t>(src[k]) & (dtype[k] == VQK_F32 ? 3u : 1u)) == 0, VQK_ERR_ALIGN);
        // an integer in [0, 2^20): (double)x * w is then exact
        VQK_REQUIRE(weight[k] >= 0.0 && weight[k] < 1048576.0 && weight[k] == (double)(int64_t)weight[k], VQK_ERR_ARG);
        VQK_REQUIRE(slot[k] >= 0 && slot[k] < nslots, VQK_ERR_ARG);
        for (int j = 0; j < k; ++j) VQK_REQUIRE(slot[j] != slot[k], VQK_ERR_ARG);      // one thread owns one slot
        a.src[k] = src[k]; a.dtype[k] = dtype[k]; a.w[k] = weight[k]; a.slot[k] = slot[k];
    }
    for (int k = n; k < VQK_SCALAR_MAX; ++k) { a.src[k] = nullptr; a.dtype[k] = 0; a.w[k] = 0.0; a.slot[k] = 0; }
    hipLaunchKernelGGL(scalar_accum_kernel, dim3(1), dim3(64), 0, vqk_stream(stream), a, acc);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

extern "C" int64_t vqk_arena_stats_ws_bytes(int64_t numel, int ngroups) {
    if (numel < 1 || numel > ((int64_t)1 << 38) || ngroups < 1 || ngroups > VQK_ARENA_MAX_GROUPS) return -1;
    return (int64_t)arena_blocks(numel) * ngroups * 3 * (int64_t)sizeof(double);
}

extern "C" int vqk_arena_stats(const float* g, int64_t numel, const int64_t* seg_end, const int32_t* seg_group, int nseg,
                               int ngroups, float scale, void* ws, int64_t ws_bytes, double* out, double* acc, void* stream) {
    VQK_REQUIRE(g && seg_end && seg_group && ws && out, VQK_ERR_ARG);
    VQK_REQUIRE(numel >= 1 && numel <= ((int64_t)1 << 38) && nseg >= 1 && ngroups >= 1 && ngroups <= VQK_ARENA_MAX_GROUPS, VQK_ERR_SHAPE);
    VQK_REQUIRE(scale == scale && scale - scale == 0.0f, VQK_ERR_ARG);                 // a finite scale
    VQK_REQUIRE((reinterpret_cast<uintptr_t>(g) & 3u) == 0, VQK_ERR_ALIGN);
    VQK_REQUIRE(((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(acc) |
                  reinterpret_cast<uintptr_t>(seg_end)) & 7u) == 0 && (reinterpret_cast<uintptr_t>(seg_group) & 3u) == 0, VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqk_arena_stats_ws_bytes(numel, ngroups), VQK_ERR_WORKSPACE);
    const int blocks = arena_blocks(numel);
    hipStream_t st = vqk_stream(stream);
    hipLaunchKernelGGL(arena_stats_kernel, dim3((unsigned)blocks), dim3(AS_THREADS), 0, st, g, numel, seg_end, seg_group, nseg, ngroups,
                       scale, (int)vqk_aligned16(g), static_cast<double*>(ws));
    VQK_CHECK_LAUNCH();
    hipLaunchKernelGGL(arena_finish_kernel, dim3(1), dim3(AS_THREADS), 0, st, static_cast<const double*>(ws), blocks, ngroups, out, acc);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}
