// n-layer PatchGAN discriminator kernels (include/vqk.h, "PatchGAN discriminator"): 4x4 convs with padding 1 and stride 1 / 2 as
// gather-GEMMs on the matrix pipe (forward, data gradient, weight gradient) and BatchNorm (+ LeakyReLU) over NHWC rows.
// No float atomics anywhere in this file: sums that cross workgroups go through caller-owned workspaces in per-block slabs and are
// added in index order by a finish launch, so every output has the same bits on every run.
//
// Conv tiles: 128 (or 64) rows x 64 columns x 32 reduction elements per step, 4 waves as 2 x 2, each wave 32x32 MFMA tiles
// (VQK_BF16: mfma_f32_32x32x16_bf16, VQK_F32: the exact mfma_f32_32x32x2f32); operands staged global -> registers -> LDS with the
// next step's loads in flight over the current step's MFMAs.  Weights are read from the fp32 master [Cout][4][4][Cin] directly (the
// bf16 mode rounds them to nearest even on the way into LDS).
#include "common.h"

namespace {

constexpr int BK = 32;              // reduction elements per LDS step
constexpr int NT = 64;              // tile columns
constexpr int THREADS = 256;
constexpr float SLOPE = 0.2f;

template <typename T> struct Pg;
template <> struct Pg<float> { static constexpr int E = 4, LD = 36; };          // row pitch in elements: 144 B
template <> struct Pg<bf16_raw> { static constexpr int E = 8, LD = 40; };       // 80 B

__device__ __forceinline__ float to_t(float v, float*) { return v; }
__device__ __forceinline__ bf16_raw to_t(float v, bf16_raw*) { return (bf16_raw)(vqk_pack_bf16x2(v, v) & 0xffffu); }
// element e (a compile-time constant after unrolling) of a 16-byte chunk held in registers
__device__ __forceinline__ float chunk_elem(const vqk_u32x4& v, int e, float*) { return __uint_as_float(v[e]); }
__device__ __forceinline__ bf16_raw chunk_elem(const vqk_u32x4& v, int e, bf16_raw*) { return (bf16_raw)((v[e >> 1] >> (16 * (e & 1))) & 0xffffu); }

// acc[i] (rows 32 i .. 32 i + 31 of `a`) += a b^T over the BK elements of one LDS step.  fp32: lane (r, h) reads k = 8 s + 4 h + 0..3
// of its row as one 16-byte vector and feeds MFMA j of step s with element j -- the same k on both sides, all a sum over k needs.
template <int MA> __device__ __forceinline__ void mma_step(f32x16 (&acc)[MA], const float* a, const float* b, int lane) {
    constexpr int LD = Pg<float>::LD;
    const float* pa = a + (lane & 31) * LD + 4 * (lane >> 5);
    const float* pb = b + (lane & 31) * LD + 4 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < BK / 8; ++s) {
        const f32x4 vb = *reinterpret_cast<const f32x4*>(pb + 8 * s);
#pragma unroll
        for (int i = 0; i < MA; ++i) {
            const f32x4 va = *reinterpret_cast<const f32x4*>(pa + i * 32 * LD + 8 * s);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[j], vb[j], acc[i], 0, 0, 0);
        }
    }
}
template <int MA> __device__ __forceinline__ void mma_step(f32x16 (&acc)[MA], const bf16_raw* a, const bf16_raw* b, int lane) {
    constexpr int LD = Pg<bf16_raw>::LD;
    const bf16_raw* pa = a + (lane & 31) * LD + 8 * (lane >> 5);
    const bf16_raw* pb = b + (lane & 31) * LD + 8 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
        const bf16x8_t vb = *reinterpret_cast<const bf16x8_t*>(pb + 16 * s);
#pragma unroll
        for (int i = 0; i < MA; ++i) {
            const bf16x8_t va = *reinterpret_cast<const bf16x8_t*>(pa + i * 32 * LD + 16 * s);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, vb, acc[i], 0, 0, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// forward / data gradient: out[pixel][col] = sum_{tap, c} src[pixel * mul + off(tap)][c] * W(col, tap, c)
// ------------------------------------------------------------------------------------------------------------------------
enum { MODE_FPROP = 0, MODE_DGRAD1 = 1, MODE_DGRAD2 = 2 };

struct ConvArgs {
    const void* src; const float* w; const float* bias; void* out;
    int n, hs, ws, cs;              // source tensor [n][hs][ws][cs]
    int ho, wo, co_ld;              // output tensor [n][ho][wo][co_ld]
    int ncols;                      // real output columns (forward: Cout, data gradient: the weight's Cin); the rest of co_ld gets zeros
    int kreal;                      // real channels of the reduction axis (forward: the weight's Cin, data gradient: Cout)
    int cin_w;                      // the weight's Cin
    int wstride_n, wstride_c;       // weight element strides of a column / of a reduction channel
    int stride, lrelu, wvec;        // wvec: 16-byte weight loads are legal (Cin % 4 == 0, 16-byte aligned master)
};

// tap t of the launch -> source offset (dy, dx) and the weight's kernel position kh * 4 + kw
template <int MODE> __device__ __forceinline__ void tap_of(int t, int py, int px, int& dy, int& dx, int& widx) {
    if (MODE == MODE_FPROP) {
        const int kh = t >> 2, kw = t & 3;
        dy = kh - 1; dx = kw - 1; widx = t;
    } else if (MODE == MODE_DGRAD1) {
        const int kh = t >> 2, kw = t & 3;
        dy = 1 - kh; dx = 1 - kw; widx = t;
    } else {                        // input parity (py, px) sees kh = (1 - py) + 2 a, kw = (1 - px) + 2 b at dy[j + py - a][i + px - b]
        const int a = t >> 1, b = t & 1;
        dy = py - a; dx = px - b; widx = ((1 - py) + 2 * a) * 4 + (1 - px) + 2 * b;
    }
}

template <typename T, int MODE>
__global__ __launch_bounds__(THREADS) void pg_conv_kernel(const ConvArgs p) {
    constexpr int E = Pg<T>::E, LD = Pg<T>::LD, MT = 128, MA = 2;
    constexpr int CPR = BK / E;                     // 16-byte chunks per tile row
    constexpr int NA = MT * CPR / THREADS;          // chunks of the gathered operand per thread
    constexpr int TAPS = MODE == MODE_DGRAD2 ? 4 : 16;
    __shared__ __attribute__((aligned(16))) T sA[MT * LD];
    __shared__ __attribute__((aligned(16))) T sB[NT * LD];
    __shared__ int s_opix[MT];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int py = MODE == MODE_DGRAD2 ? (int)(blockIdx.z >> 1) : 0, px = MODE == MODE_DGRAD2 ? (int)(blockIdx.z & 1) : 0;
    // the grid of output pixels this launch (phase) owns and how it maps onto the output tensor
    const int hsub = MODE == MODE_DGRAD2 ? (p.ho - py + 1) / 2 : p.ho;
    const int wsub = MODE == MODE_DGRAD2 ? (p.wo - px + 1) / 2 : p.wo;
    const int mul = MODE == MODE_FPROP ? p.stride : 1;
    const int mtot = p.n * hsub * wsub;
    const int m0 = blockIdx.x * MT, n0 = blockIdx.y * NT;
    if (m0 >= mtot) return;
    const int K = TAPS * p.cs;

    if (tid < MT) {
        const int m = m0 + tid;
        int o = -1;
        if (m < mtot) {
            const int img = m / (hsub * wsub), rem = m - img * (hsub * wsub);
            const int j = rem / wsub, i = rem - j * wsub;
            const int oy = MODE == MODE_DGRAD2 ? 2 * j + py : j, ox = MODE == MODE_DGRAD2 ? 2 * i + px : i;
            o = (img * p.ho + oy) * p.wo + ox;
        }
        s_opix[tid] = o;
    }
    // rows of the gathered operand this thread stages: chunk column kc (the same for all of them), rows arow + i * (THREADS / CPR)
    const int kc = tid % CPR, arow = tid / CPR;
    int by[NA], bx[NA], bimg[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int m = m0 + arow + i * (THREADS / CPR);
        if (m < mtot) {
            const int img = m / (hsub * wsub), rem = m - img * (hsub * wsub);
            const int j = rem / wsub;
            by[i] = j * mul; bx[i] = (rem - j * wsub) * mul; bimg[i] = img;
        } else {
            by[i] = -(1 << 28); bx[i] = -(1 << 28); bimg[i] = 0;
        }
    }
    const T* src = reinterpret_cast<const T*>(p.src);
    vqk_u32x4 ra[NA];
    float rb[8];

    auto load_tile = [&](int k0) {
        {   // gathered operand: one 16-byte chunk = E channels of one tap of one pixel
            const int kk = k0 + kc * E;
            const int t = kk / p.cs, c = kk - t * p.cs;
            int dy, dx, widx;
            tap_of<MODE>(t, py, px, dy, dx, widx);
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int sy = by[i] + dy, sx = bx[i] + dx;
                const bool ok = kk < K && sy >= 0 && sy < p.hs && sx >= 0 && sx < p.ws;
                vqk_u32x4 v = {0u, 0u, 0u, 0u};
                if (ok) v = *reinterpret_cast<const vqk_u32x4*>(src + (((int64_t)bimg[i] * p.hs + sy) * p.ws + sx) * p.cs + c);
                ra[i] = v;
            }
        }
        // weights, fp32 master: forward -- 8 consecutive k of one column; data gradient -- 8 consecutive columns of one k
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            int kk, n;
            if (MODE == MODE_FPROP) { n = n0 + (tid >> 2); kk = k0 + (tid & 3) * 8 + 4 * g; }
            else { kk = k0 + (tid >> 3); n = n0 + (tid & 7) * 8 + 4 * g; }
            const int t = kk / p.cs, c = kk - t * p.cs;
            int dy, dx, widx;
            tap_of<MODE>(t, py, px, dy, dx, widx);
            const int64_t base = (int64_t)n * p.wstride_n + (int64_t)c * p.wstride_c + widx * p.cin_w;
            // (forward: the 4 elements walk c, bounded by kreal; data gradient: they walk n, bounded by ncols)
            const int lim = MODE == MODE_FPROP ? p.kreal - c : p.ncols - n;
            const bool inr = kk < K && (MODE == MODE_FPROP ? n < p.ncols : c < p.kreal);
            if (p.wvec) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (inr && lim >= 4) v = *reinterpret_cast<const f32x4*>(p.w + base);
                rb[4 * g] = v[0]; rb[4 * g + 1] = v[1]; rb[4 * g + 2] = v[2]; rb[4 * g + 3] = v[3];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) rb[4 * g + e] = (inr && e < lim) ? p.w[base + e] : 0.f;
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < NA; ++i)
            *reinterpret_cast<vqk_u32x4*>(&sA[(arow + i * (THREADS / CPR)) * LD + kc * E]) = ra[i];
        if (MODE == MODE_FPROP) {
            T* d = &sB[(tid >> 2) * LD + (tid & 3) * 8];
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = to_t(rb[e], (T*)nullptr);
        } else {
            T* d = &sB[(tid & 7) * 8 * LD + (tid >> 3)];
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e * LD] = to_t(rb[e], (T*)nullptr);
        }
    };

    f32x16 acc[MA];
#pragma unroll
    for (int i = 0; i < MA; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const int wm = wid >> 1, wn = wid & 1;

    load_tile(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
        store_tile();
        __syncthreads();
        if (k0 + BK < K) load_tile(k0 + BK);
        mma_step<MA>(acc, sA + wm * (MT / 2) * LD, sB + wn * 32 * LD, lane);
        __syncthreads();
    }

    // epilogue: column = lane & 31, rows over the registers (C/D map of the 32x32 MFMA)
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= p.co_ld) return;
    const bool real = col < p.ncols;
    const float bias = (real && p.bias) ? p.bias[col] : 0.f;
    T* out = reinterpret_cast<T*>(p.out);
#pragma unroll
    for (int i = 0; i < MA; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * (MT / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int o = s_opix[row];
            if (o < 0) continue;
            float v = real ? acc[i][r] + bias : 0.f;
            if (p.lrelu) v = v > 0.f ? v : SLOPE * v;
            out[(int64_t)o * p.co_ld + col] = to_t(v, (T*)nullptr);
        }
}

// ------------------------------------------------------------------------------------------------------------------------
// weight gradient: part[split][co][tap][ci] = sum_{pixels of the split} dy[p][co] x[p * s + tap - 1][ci]
// ------------------------------------------------------------------------------------------------------------------------
struct WgArgs {
    const void* x; const void* dy; float* part;
    int n, h, w, cin, cin_w;        // x [n][h][w][cin], the weight's Cin
    int ho, wo, cout, co_ld;        // dy [n][ho][wo][co_ld]
    int stride, ptot, tiles_per_split, ktiles;
};

template <typename T, int MT>
__global__ __launch_bounds__(THREADS) void pg_wgrad_kernel(const WgArgs p) {
    constexpr int E = Pg<T>::E, LD = Pg<T>::LD, MA = MT / 64;
    constexpr int NA = MT / E * BK / THREADS;       // dy chunks per thread
    constexpr int NB = NT / E * BK / THREADS;       // x chunks per thread
    __shared__ __attribute__((aligned(16))) T sA[MT * LD];
    __shared__ __attribute__((aligned(16))) T sB[NT * LD];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n0 = blockIdx.x * NT, m0 = blockIdx.y * MT;
    const int kt0 = blockIdx.z * p.tiles_per_split;
    const int kt1 = min(kt0 + p.tiles_per_split, p.ktiles);
    const int pl = tid & 31, cq = tid >> 5;         // pixel of the step, first chunk row

    // the x chunks of this thread: column chunk -> (tap, first channel), fixed over the pixel loop
    int xc[NB], xdy[NB], xdx[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int colc = n0 + (cq + i * 8) * E;
        const int t = colc / p.cin;
        xc[i] = t < 16 ? colc - t * p.cin : -1;
        xdy[i] = (t >> 2) - 1; xdx[i] = (t & 3) - 1;
    }
    const T* x = reinterpret_cast<const T*>(p.x);
    const T* dy = reinterpret_cast<const T*>(p.dy);
    vqk_u32x4 ra[NA], rb[NB];

    auto load_tile = [&](int kt) {
        const int pix = kt * BK + pl;
        const bool pok = pix < p.ptot;
        const int img = pix / (p.ho * p.wo), rem = pix - img * (p.ho * p.wo);
        const int oy = rem / p.wo, ox = rem - oy * p.wo;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int co = m0 + (cq + i * 8) * E;
            vqk_u32x4 v = {0u, 0u, 0u, 0u};
            if (pok && co < p.co_ld) v = *reinterpret_cast<const vqk_u32x4*>(dy + (int64_t)pix * p.co_ld + co);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int sy = oy * p.stride + xdy[i], sx = ox * p.stride + xdx[i];
            vqk_u32x4 v = {0u, 0u, 0u, 0u};
            if (pok && xc[i] >= 0 && sy >= 0 && sy < p.h && sx >= 0 && sx < p.w)
                v = *reinterpret_cast<const vqk_u32x4*>(x + (((int64_t)img * p.h + sy) * p.w + sx) * p.cin + xc[i]);
            rb[i] = v;
        }
    };
    // transposing store: chunk element e of pixel pl -> LDS row (chunk row * E + e), column pl
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
#pragma unroll
            for (int e = 0; e < E; ++e) sA[((cq + i * 8) * E + e) * LD + pl] = chunk_elem(ra[i], e, (T*)nullptr);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
#pragma unroll
            for (int e = 0; e < E; ++e) sB[((cq + i * 8) * E + e) * LD + pl] = chunk_elem(rb[i], e, (T*)nullptr);
        }
    };

    f32x16 acc[MA];
#pragma unroll
    for (int i = 0; i < MA; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const int wm = wid >> 1, wn = wid & 1;

    if (kt0 < kt1) load_tile(kt0);
    for (int kt = kt0; kt < kt1; ++kt) {
        store_tile();
        __syncthreads();
        if (kt + 1 < kt1) load_tile(kt + 1);
        mma_step<MA>(acc, sA + wm * (MT / 2) * LD, sB + wn * 32 * LD, lane);
        __syncthreads();
    }

    const int col = n0 + wn * 32 + (lane & 31);
    const int t = col / p.cin, ci = col - t * p.cin;
    if (t >= 16 || ci >= p.cin_w) return;
    float* part = p.part + (int64_t)blockIdx.z * p.cout * 16 * p.cin_w + t * p.cin_w + ci;
#pragma unroll
    for (int i = 0; i < MA; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = m0 + wm * (MT / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (co < p.cout) part[(int64_t)co * 16 * p.cin_w] = acc[i][r];
        }
}

// dw[i] (+)= scale * (part[0][i] + part[1][i] + ...), the partials added in split order
__global__ __launch_bounds__(THREADS) void pg_wgrad_finish_kernel(const float* part, float* dw, int64_t elems, int splits, float scale,
                                                                  int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= elems) return;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += part[(int64_t)z * elems + i];
    dw[i] = accumulate ? dw[i] + scale * s : scale * s;
}

// ------------------------------------------------------------------------------------------------------------------------
// BatchNorm (+ LeakyReLU) over [rows][c]
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bn_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float bn_z(float xh, float g, float b) { return __fmaf_rn(xh, g, b); }

// per-block partial sums in fp64: forward (BWD = 0) sum x, sum x^2; backward sum g, sum g xhat with g = dy through the LeakyReLU mask
template <typename T, int BWD>
__global__ __launch_bounds__(THREADS) void pg_bn_partial_kernel(const T* x, const T* dy, const float* gamma, const float* beta,
                                                                const float* mean, const float* rstd, int64_t rows, int c,
                                                                int64_t rows_per_block, int lrelu, double* part) {
    constexpr int E = Pg<T>::E;
    __shared__ double red[THREADS * E * 2];
    const int tid = threadIdx.x;
    const int cc = c / E, rl_n = THREADS / cc;
    const int ch = (tid % cc) * E, rl = tid / cc;
    double s0[E], s1[E];
#pragma unroll
    for (int e = 0; e < E; ++e) { s0[e] = 0.0; s1[e] = 0.0; }
    if (rl < rl_n) {
        float g[E], b[E], mu[E], rs[E];
        if (BWD) {
#pragma unroll
            for (int e = 0; e < E; ++e) { g[e] = gamma[ch + e]; b[e] = beta[ch + e]; mu[e] = mean[ch + e]; rs[e] = rstd[ch + e]; }
        }
        const int64_t r0 = blockIdx.x * rows_per_block;
        const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
        for (int64_t r = r0 + rl; r < r1; r += rl_n) {
            float v[E];
            Vec16<T>::load(x + r * c + ch, v);
            if (BWD) {
                float d[E];
                Vec16<T>::load(dy + r * c + ch, d);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float xh = bn_xhat(v[e], mu[e], rs[e]);
                    const float gg = (lrelu && !(bn_z(xh, g[e], b[e]) > 0.f)) ? SLOPE * d[e] : d[e];
                    s0[e] += (double)gg; s1[e] += (double)gg * (double)xh;
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) { s0[e] += (double)v[e]; s1[e] += (double)v[e] * (double)v[e]; }
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) { red[(rl * c + ch + e) * 2] = s0[e]; red[(rl * c + ch + e) * 2 + 1] = s1[e]; }
    }
    __syncthreads();
    for (int k = tid; k < c; k += THREADS) {
        double a0 = 0.0, a1 = 0.0;
        for (int q = 0; q < rl_n; ++q) { a0 += red[(q * c + k) * 2]; a1 += red[(q * c + k) * 2 + 1]; }
        part[((int64_t)blockIdx.x * 2) * c + k] = a0;
        part[((int64_t)blockIdx.x * 2 + 1) * c + k] = a1;
    }
}

__global__ __launch_bounds__(THREADS) void pg_bn_finish_fwd_kernel(const double* part, int blocks, int64_t rows, int c, float eps,
                                                                   float momentum, float* mean, float* rstd, float* running_mean,
                                                                   float* running_var, int64_t* nbt) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k == 0 && nbt) *nbt += 1;
    if (k >= c) return;
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < blocks; ++b) { s0 += part[((int64_t)b * 2) * c + k]; s1 += part[((int64_t)b * 2 + 1) * c + k]; }
    const double m = s0 / (double)rows;
    double var = s1 / (double)rows - m * m;
    if (var < 0.0) var = 0.0;
    mean[k] = (float)m;
    rstd[k] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) running_mean[k] = (float)((1.0 - (double)momentum) * (double)running_mean[k] + (double)momentum * m);
    if (running_var) running_var[k] = (float)((1.0 - (double)momentum) * (double)running_var[k]
                                              + (double)momentum * var * ((double)rows / (double)(rows - 1)));
}

// y = leaky(gamma xhat + beta); stats = (mean, rstd) of the batch, or (running_mean, running_var) in eval mode
template <typename T>
__global__ __launch_bounds__(THREADS) void pg_bn_apply_kernel(const T* x, const float* gamma, const float* beta, const float* s_mean,
                                                              const float* s_second, int eval, float eps, int64_t rows, int c, int lrelu,
                                                              T* y) {
    constexpr int E = Pg<T>::E;
    const int cc = c / E;
    const int64_t chunks = rows * cc;
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < chunks; q += (int64_t)gridDim.x * THREADS) {
        const int ch = (int)(q % cc) * E;
        float v[E], o[E];
        Vec16<T>::load(x + q * E, v);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const float rs = eval ? 1.0f / sqrtf(s_second[ch + e] + eps) : s_second[ch + e];
            const float z = bn_z(bn_xhat(v[e], s_mean[ch + e], rs), gamma[ch + e], beta[ch + e]);
            o[e] = (lrelu && !(z > 0.f)) ? SLOPE * z : z;
        }
        Vec16<T>::store(y + q * E, o);
    }
}

__global__ __launch_bounds__(THREADS) void pg_bn_finish_bwd_kernel(const double* part, int blocks, int64_t rows, int c, float* dgamma,
                                                                   float* dbeta, int accumulate, float* means) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= c) return;
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < blocks; ++b) { s0 += part[((int64_t)b * 2) * c + k]; s1 += part[((int64_t)b * 2 + 1) * c + k]; }
    if (dbeta) dbeta[k] = accumulate ? dbeta[k] + (float)s0 : (float)s0;
    if (dgamma) dgamma[k] = accumulate ? dgamma[k] + (float)s1 : (float)s1;
    means[k] = (float)(s0 / (double)rows);
    means[c + k] = (float)(s1 / (double)rows);
}

// db[k] (+)= scale * column sum k of a [rows][c] tensor, from the forward partials (their first moment), k < cout
__global__ __launch_bounds__(THREADS) void pg_bias_finish_kernel(const double* part, int blocks, int c, int cout, float scale, float* db,
                                                                 int accumulate) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= cout) return;
    double s0 = 0.0;
    for (int b = 0; b < blocks; ++b) s0 += part[((int64_t)b * 2) * c + k];
    const float v = (float)((double)scale * s0);
    db[k] = accumulate ? db[k] + v : v;
}

// dx = gamma rstd (g - mean(g) - xhat mean(g xhat))
template <typename T>
__global__ __launch_bounds__(THREADS) void pg_bn_dx_kernel(const T* x, const T* dy, const float* gamma, const float* beta, const float* mean,
                                                           const float* rstd, const float* means, int64_t rows, int c, int lrelu, T* dx) {
    constexpr int E = Pg<T>::E;
    const int cc = c / E;
    const int64_t chunks = rows * cc;
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < chunks; q += (int64_t)gridDim.x * THREADS) {
        const int ch = (int)(q % cc) * E;
        float v[E], d[E], o[E];
        Vec16<T>::load(x + q * E, v);
        Vec16<T>::load(dy + q * E, d);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const float g = gamma[ch + e], rs = rstd[ch + e];
            const float xh = bn_xhat(v[e], mean[ch + e], rs);
            const float gg = (lrelu && !(bn_z(xh, g, beta[ch + e]) > 0.f)) ? SLOPE * d[e] : d[e];
            o[e] = g * rs * (gg - means[ch + e] - xh * means[c + ch + e]);
        }
        Vec16<T>::store(dx + q * E, o);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------
inline int out_size(int in, int stride) { return (in + 2 - 4) / stride + 1; }

int conv_shape_ok(int dtype, int n, int h, int w, int cin, int cin_w, int cout, int co_ld, int stride) {
    VQK_REQUIRE(dtype == VQK_F32 || dtype == VQK_BF16, VQK_ERR_DTYPE);
    const int e = dtype == VQK_F32 ? 4 : 8;
    VQK_REQUIRE(stride == 1 || stride == 2, VQK_ERR_SHAPE);
    VQK_REQUIRE(n >= 1 && h >= 2 && w >= 2 && cin >= e && cin % e == 0 && cin_w >= 1 && cin_w <= cin && cin <= 4096, VQK_ERR_SHAPE);
    VQK_REQUIRE(cout >= 1 && cout <= 4096 && co_ld >= cout && co_ld % e == 0 && co_ld < cout + e, VQK_ERR_SHAPE);
    const int ho = out_size(h, stride), wo = out_size(w, stride);
    VQK_REQUIRE(ho >= 1 && wo >= 1, VQK_ERR_SHAPE);
    // pixel indices, row counts and per-split slab offsets stay below 2^31 (element offsets are 64-bit)
    VQK_REQUIRE((int64_t)n * h * w < (1ll << 30) && (int64_t)n * h * w * cin < (1ll << 40), VQK_ERR_SHAPE);
    return VQK_OK;
}

struct WgPlan { int mt, ktiles, tiles_per_split, splits; int64_t elems; };

WgPlan wgrad_plan(int n, int h, int w, int cin, int cin_w, int cout, int stride) {
    WgPlan pl;
    const int64_t ptot = (int64_t)n * out_size(h, stride) * out_size(w, stride);
    pl.mt = cout <= 64 ? 64 : 128;
    pl.ktiles = (int)((ptot + BK - 1) / BK);
    const int tiles = ((cout + pl.mt - 1) / pl.mt) * ((16 * cin + NT - 1) / NT);
    int want = (1024 + tiles - 1) / tiles;                    // ~4 workgroups per CU when the pixel count allows it
    if (want < 1) want = 1;
    int tps = (pl.ktiles + want - 1) / want;
    if (tps < 4) tps = 4;                                     // at least 128 pixels per partial
    pl.tiles_per_split = tps;
    pl.splits = (pl.ktiles + tps - 1) / tps;                  // every split owns at least one step
    pl.elems = (int64_t)cout * 16 * cin_w;
    return pl;
}

int bn_blocks(int64_t rows) {
    int64_t g = (rows + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 512 ? 512 : g));
}

template <typename T> int launch_conv(int mode, const ConvArgs& a, hipStream_t st) {
    const int hsub = mode == MODE_DGRAD2 ? (a.ho + 1) / 2 : a.ho, wsub = mode == MODE_DGRAD2 ? (a.wo + 1) / 2 : a.wo;
    const int64_t mtot = (int64_t)a.n * hsub * wsub;
    dim3 grid((unsigned)((mtot + 127) / 128), (unsigned)((a.co_ld + NT - 1) / NT), mode == MODE_DGRAD2 ? 4 : 1);
    if (mode == MODE_FPROP) hipLaunchKernelGGL((pg_conv_kernel<T, MODE_FPROP>), grid, dim3(THREADS), 0, st, a);
    else if (mode == MODE_DGRAD1) hipLaunchKernelGGL((pg_conv_kernel<T, MODE_DGRAD1>), grid, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((pg_conv_kernel<T, MODE_DGRAD2>), grid, dim3(THREADS), 0, st, a);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // namespace

extern "C" {

int vqk_conv4x4_fprop(int dtype, const void* x, const float* w, const float* bias, void* y, int n, int h, int wd, int cin, int cin_w,
                      int cout, int co_ld, int stride, int lrelu, void* stream) {
    const int st = conv_shape_ok(dtype, n, h, wd, cin, cin_w, cout, co_ld, stride);
    if (st != VQK_OK) return st;
    VQK_REQUIRE(x && w && y, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(y), VQK_ERR_ALIGN);
    VQK_REQUIRE((reinterpret_cast<uintptr_t>(w) & 3u) == 0 && (reinterpret_cast<uintptr_t>(bias) & 3u) == 0, VQK_ERR_ALIGN);
    ConvArgs a;
    a.src = x; a.w = w; a.bias = bias; a.out = y;
    a.n = n; a.hs = h; a.ws = wd; a.cs = cin;
    a.ho = out_size(h, stride); a.wo = out_size(wd, stride); a.co_ld = co_ld;
    a.ncols = cout; a.kreal = cin_w; a.cin_w = cin_w;
    a.wstride_n = 16 * cin_w; a.wstride_c = 1;
    a.stride = stride; a.lrelu = lrelu ? 1 : 0;
    a.wvec = (cin_w % 4 == 0 && vqk_aligned16(w)) ? 1 : 0;
    return dtype == VQK_F32 ? launch_conv<float>(MODE_FPROP, a, vqk_stream(stream)) : launch_conv<bf16_raw>(MODE_FPROP, a, vqk_stream(stream));
}

int vqk_conv4x4_dgrad(int dtype, const void* dy, const float* w, void* dx, int n, int h, int wd, int cin, int cin_w, int cout, int co_ld,
                      int stride, void* stream) {
    const int st = conv_shape_ok(dtype, n, h, wd, cin, cin_w, cout, co_ld, stride);
    if (st != VQK_OK) return st;
    VQK_REQUIRE(dy && w && dx, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(dy) && vqk_aligned16(dx), VQK_ERR_ALIGN);
    VQK_REQUIRE((reinterpret_cast<uintptr_t>(w) & 3u) == 0, VQK_ERR_ALIGN);
    ConvArgs a;
    a.src = dy; a.w = w; a.bias = nullptr; a.out = dx;
    a.n = n; a.hs = out_size(h, stride); a.ws = out_size(wd, stride); a.cs = co_ld;
    a.ho = h; a.wo = wd; a.co_ld = cin;
    a.ncols = cin_w; a.kreal = cout; a.cin_w = cin_w;
    a.wstride_n = 1; a.wstride_c = 16 * cin_w;
    a.stride = stride; a.lrelu = 0;
    a.wvec = (cin_w % 4 == 0 && vqk_aligned16(w)) ? 1 : 0;
    const int mode = stride == 1 ? MODE_DGRAD1 : MODE_DGRAD2;
    return dtype == VQK_F32 ? launch_conv<float>(mode, a, vqk_stream(stream)) : launch_conv<bf16_raw>(mode, a, vqk_stream(stream));
}

int vqk_conv4x4_wgrad_plan(int n, int h, int wd, int cin, int cin_w, int cout, int stride) {
    if (conv_shape_ok(VQK_F32, n, h, wd, (cin + 3) / 4 * 4, cin_w, cout, (cout + 3) / 4 * 4, stride) != VQK_OK) return VQK_ERR_SHAPE;
    return wgrad_plan(n, h, wd, cin, cin_w, cout, stride).splits;
}

int64_t vqk_conv4x4_wgrad_ws_bytes(int n, int h, int wd, int cin, int cin_w, int cout, int stride) {
    if (conv_shape_ok(VQK_F32, n, h, wd, (cin + 3) / 4 * 4, cin_w, cout, (cout + 3) / 4 * 4, stride) != VQK_OK) return VQK_ERR_SHAPE;
    const WgPlan pl = wgrad_plan(n, h, wd, cin, cin_w, cout, stride);
    return ((int64_t)pl.splits * pl.elems * 4 + 15) / 16 * 16;
}

int vqk_conv4x4_wgrad(int dtype, const void* x, const void* dy, float* dw, int n, int h, int wd, int cin, int cin_w, int cout, int co_ld,
                      int stride, float scale, int accumulate, void* ws, int64_t ws_bytes, void* stream) {
    const int st = conv_shape_ok(dtype, n, h, wd, cin, cin_w, cout, co_ld, stride);
    if (st != VQK_OK) return st;
    VQK_REQUIRE(x && dy && dw && ws, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(dy) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE((reinterpret_cast<uintptr_t>(dw) & 3u) == 0, VQK_ERR_ALIGN);
    const WgPlan pl = wgrad_plan(n, h, wd, cin, cin_w, cout, stride);
    VQK_REQUIRE(ws_bytes >= (int64_t)pl.splits * pl.elems * 4, VQK_ERR_WORKSPACE);
    WgArgs a;
    a.x = x; a.dy = dy; a.part = reinterpret_cast<float*>(ws);
    a.n = n; a.h = h; a.w = wd; a.cin = cin; a.cin_w = cin_w;
    a.ho = out_size(h, stride); a.wo = out_size(wd, stride); a.cout = cout; a.co_ld = co_ld;
    a.stride = stride; a.ptot = n * a.ho * a.wo; a.tiles_per_split = pl.tiles_per_split; a.ktiles = pl.ktiles;
    hipStream_t s = vqk_stream(stream);
    dim3 grid((unsigned)((16 * cin + NT - 1) / NT), (unsigned)((cout + pl.mt - 1) / pl.mt), (unsigned)pl.splits);
    if (dtype == VQK_F32) {
        if (pl.mt == 64) hipLaunchKernelGGL((pg_wgrad_kernel<float, 64>), grid, dim3(THREADS), 0, s, a);
        else hipLaunchKernelGGL((pg_wgrad_kernel<float, 128>), grid, dim3(THREADS), 0, s, a);
    } else {
        if (pl.mt == 64) hipLaunchKernelGGL((pg_wgrad_kernel<bf16_raw, 64>), grid, dim3(THREADS), 0, s, a);
        else hipLaunchKernelGGL((pg_wgrad_kernel<bf16_raw, 128>), grid, dim3(THREADS), 0, s, a);
    }
    VQK_CHECK_LAUNCH();
    hipLaunchKernelGGL(pg_wgrad_finish_kernel, dim3((unsigned)((pl.elems + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a.part, dw,
                       pl.elems, pl.splits, scale, accumulate ? 1 : 0);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

static int bn_shape_ok(int dtype, int64_t rows, int c) {
    VQK_REQUIRE(dtype == VQK_F32 || dtype == VQK_BF16, VQK_ERR_DTYPE);
    const int e = dtype == VQK_F32 ? 4 : 8;
    VQK_REQUIRE(rows >= 1 && rows < (1ll << 40) && c >= e && c % e == 0 && c / e <= THREADS, VQK_ERR_SHAPE);
    return VQK_OK;
}

int64_t vqk_bn_ws_bytes(int64_t rows, int c) {
    if (rows < 1 || c < 4 || c % 4) return VQK_ERR_SHAPE;
    return ((int64_t)bn_blocks(rows) * 2 * c * 8 + (int64_t)2 * c * 4 + 15) / 16 * 16;
}

int vqk_bn_forward(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                   float* running_mean, float* running_var, int64_t* num_batches_tracked, int64_t rows, int c, float eps, float momentum,
                   int training, int lrelu, void* ws, int64_t ws_bytes, void* stream) {
    const int st = bn_shape_ok(dtype, rows, c);
    if (st != VQK_OK) return st;
    VQK_REQUIRE(x && gamma && beta && y, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(y), VQK_ERR_ALIGN);
    VQK_REQUIRE(eps > 0.f && momentum >= 0.f && momentum <= 1.f, VQK_ERR_ARG);
    hipStream_t s = vqk_stream(stream);
    const int64_t chunks = rows * (c / (dtype == VQK_F32 ? 4 : 8));
    const int agrid = vqk_grid_1d(chunks, THREADS);
    if (training) {
        VQK_REQUIRE(rows >= 2, VQK_ERR_SHAPE);                // one value per channel has no variance (torch raises as well)
        VQK_REQUIRE(mean && rstd && ws, VQK_ERR_ARG);
        VQK_REQUIRE(vqk_aligned16(ws), VQK_ERR_ALIGN);
        VQK_REQUIRE(ws_bytes >= vqk_bn_ws_bytes(rows, c), VQK_ERR_WORKSPACE);
        const int blocks = bn_blocks(rows);
        const int64_t rpb = (rows + blocks - 1) / blocks;
        double* part = reinterpret_cast<double*>(ws);
        if (dtype == VQK_F32)
            hipLaunchKernelGGL((pg_bn_partial_kernel<float, 0>), dim3(blocks), dim3(THREADS), 0, s, (const float*)x, (const float*)nullptr,
                               gamma, beta, (const float*)nullptr, (const float*)nullptr, rows, c, rpb, 0, part);
        else
            hipLaunchKernelGGL((pg_bn_partial_kernel<bf16_raw, 0>), dim3(blocks), dim3(THREADS), 0, s, (const bf16_raw*)x,
                               (const bf16_raw*)nullptr, gamma, beta, (const float*)nullptr, (const float*)nullptr, rows, c, rpb, 0, part);
        VQK_CHECK_LAUNCH();
        hipLaunchKernelGGL(pg_bn_finish_fwd_kernel, dim3((c + THREADS - 1) / THREADS), dim3(THREADS), 0, s, part, blocks, rows, c, eps,
                           momentum, mean, rstd, running_mean, running_var, num_batches_tracked);
        VQK_CHECK_LAUNCH();
    } else {
        VQK_REQUIRE(running_mean && running_var, VQK_ERR_ARG);
    }
    const float* m1 = training ? mean : running_mean;
    const float* m2 = training ? rstd : running_var;
    if (dtype == VQK_F32)
        hipLaunchKernelGGL(pg_bn_apply_kernel<float>, dim3(agrid), dim3(THREADS), 0, s, (const float*)x, gamma, beta, m1, m2,
                           training ? 0 : 1, eps, rows, c, lrelu ? 1 : 0, (float*)y);
    else
        hipLaunchKernelGGL(pg_bn_apply_kernel<bf16_raw>, dim3(agrid), dim3(THREADS), 0, s, (const bf16_raw*)x, gamma, beta, m1, m2,
                           training ? 0 : 1, eps, rows, c, lrelu ? 1 : 0, (bf16_raw*)y);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_conv4x4_bgrad(int dtype, const void* dy, float* db, int64_t rows, int co_ld, int cout, float scale, int accumulate, void* ws,
                      int64_t ws_bytes, void* stream) {
    const int st = bn_shape_ok(dtype, rows, co_ld);
    if (st != VQK_OK) return st;
    VQK_REQUIRE(cout >= 1 && cout <= co_ld, VQK_ERR_SHAPE);
    VQK_REQUIRE(dy && db && ws, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(dy) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqk_bn_ws_bytes(rows, co_ld), VQK_ERR_WORKSPACE);
    hipStream_t s = vqk_stream(stream);
    const int blocks = bn_blocks(rows);
    const int64_t rpb = (rows + blocks - 1) / blocks;
    double* part = reinterpret_cast<double*>(ws);
    if (dtype == VQK_F32)
        hipLaunchKernelGGL((pg_bn_partial_kernel<float, 0>), dim3(blocks), dim3(THREADS), 0, s, (const float*)dy, (const float*)nullptr,
                           (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, rows, co_ld, rpb, 0,
                           part);
    else
        hipLaunchKernelGGL((pg_bn_partial_kernel<bf16_raw, 0>), dim3(blocks), dim3(THREADS), 0, s, (const bf16_raw*)dy,
                           (const bf16_raw*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                           (const float*)nullptr, rows, co_ld, rpb, 0, part);
    VQK_CHECK_LAUNCH();
    hipLaunchKernelGGL(pg_bias_finish_kernel, dim3((cout + THREADS - 1) / THREADS), dim3(THREADS), 0, s, part, blocks, co_ld, cout, scale, db,
                       accumulate ? 1 : 0);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_bn_backward(int dtype, const void* x, const void* dy, const float* gamma, const float* beta, const float* mean, const float* rstd,
                    void* dx, float* dgamma, float* dbeta, int accumulate, int64_t rows, int c, int lrelu, void* ws, int64_t ws_bytes,
                    void* stream) {
    const int st = bn_shape_ok(dtype, rows, c);
    if (st != VQK_OK) return st;
    VQK_REQUIRE(rows >= 2, VQK_ERR_SHAPE);
    VQK_REQUIRE(x && dy && gamma && beta && mean && rstd && dx && ws, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(dy) && vqk_aligned16(dx) && vqk_aligned16(ws), VQK_ERR_ALIGN);
    VQK_REQUIRE(ws_bytes >= vqk_bn_ws_bytes(rows, c), VQK_ERR_WORKSPACE);
    hipStream_t s = vqk_stream(stream);
    const int blocks = bn_blocks(rows);
    const int64_t rpb = (rows + blocks - 1) / blocks;
    double* part = reinterpret_cast<double*>(ws);
    float* means = reinterpret_cast<float*>(part + (int64_t)blocks * 2 * c);
    const int64_t chunks = rows * (c / (dtype == VQK_F32 ? 4 : 8));
    const int agrid = vqk_grid_1d(chunks, THREADS);
    if (dtype == VQK_F32)
        hipLaunchKernelGGL((pg_bn_partial_kernel<float, 1>), dim3(blocks), dim3(THREADS), 0, s, (const float*)x, (const float*)dy, gamma, beta,
                           mean, rstd, rows, c, rpb, lrelu ? 1 : 0, part);
    else
        hipLaunchKernelGGL((pg_bn_partial_kernel<bf16_raw, 1>), dim3(blocks), dim3(THREADS), 0, s, (const bf16_raw*)x, (const bf16_raw*)dy,
                           gamma, beta, mean, rstd, rows, c, rpb, lrelu ? 1 : 0, part);
    VQK_CHECK_LAUNCH();
    hipLaunchKernelGGL(pg_bn_finish_bwd_kernel, dim3((c + THREADS - 1) / THREADS), dim3(THREADS), 0, s, part, blocks, rows, c, dgamma, dbeta,
                       accumulate ? 1 : 0, means);
    VQK_CHECK_LAUNCH();
    if (dtype == VQK_F32)
        hipLaunchKernelGGL(pg_bn_dx_kernel<float>, dim3(agrid), dim3(THREADS), 0, s, (const float*)x, (const float*)dy, gamma, beta, mean,
                           rstd, means, rows, c, lrelu ? 1 : 0, (float*)dx);
    else
        hipLaunchKernelGGL(pg_bn_dx_kernel<bf16_raw>, dim3(agrid), dim3(THREADS), 0, s, (const bf16_raw*)x, (const bf16_raw*)dy, gamma, beta,
                           mean, rstd, means, rows, c, lrelu ? 1 : 0, (bf16_raw*)dx);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // extern "C"
