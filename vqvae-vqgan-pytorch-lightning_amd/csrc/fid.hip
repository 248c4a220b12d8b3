// The FID Inception-v3 network (fid.py) on fp32 storage, NHWC: the input transform of torch-fidelity / torchmetrics
// (uint8 quantisation, TF1 bilinear resize to 299 x 299, (v - 128) / 128), the implicit-GEMM conv with the BatchNorm folded
// into weight and bias (epilogue relu(acc + bias), written into a channel slice of the concat), the pools, the global mean and
// the fp64 feature statistics of the Frechet distance.
//
// Conv products are exact fp32 on the matrix pipe (v_mfma_f32_32x32x2_f32: bit-for-bit a k-ordered fmaf chain per MFMA).
#include "common.h"

namespace {

constexpr int FID_OUT = 299;

// ------------------------------------------------------------------------------------------------ preprocess
struct PreGeom {
    int n, h, w;
    int64_t sn, sc, sh, sw;     // element strides of the [n][3][h][w] input view
    float sy, sx;               // in / out, rounded to fp32 (torch-fidelity multiplies an fp32 grid by an fp32 scale)
};

// ConvertImageDtype(torch.uint8) after a clamp to [0, 1]: trunc(x * 255.999f)
__device__ __forceinline__ float fid_quant(float v) {
    return truncf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.999f);
}

__global__ __launch_bounds__(256) void fid_preprocess_kernel(const float* __restrict__ x, float* __restrict__ y, PreGeom g) {
#pragma clang fp contract(off)
    const int64_t total = (int64_t)g.n * FID_OUT * FID_OUT;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int img = (int)(i / (FID_OUT * FID_OUT));
        const int rem = (int)(i - (int64_t)img * FID_OUT * FID_OUT);
        const int oy = rem / FID_OUT, ox = rem - oy * FID_OUT;
        // TF1 resize (align_corners=False, no half-pixel offset): src = dst * scale, i0 = floor(src), i1 = min(i0 + 1, in - 1)
        const float fy = (float)oy * g.sy, fx = (float)ox * g.sx;
        const int y0 = min((int)fy, g.h - 1), x0 = min((int)fx, g.w - 1);
        const int y1 = min(y0 + 1, g.h - 1), x1 = min(x0 + 1, g.w - 1);
        const float ty = fy - (float)y0, tx = fx - (float)x0;
        float o[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* p = x + img * g.sn + c * g.sc;
            const float tl = fid_quant(p[y0 * g.sh + x0 * g.sw]), tr = fid_quant(p[y0 * g.sh + x1 * g.sw]);
            const float bl = fid_quant(p[y1 * g.sh + x0 * g.sw]), br = fid_quant(p[y1 * g.sh + x1 * g.sw]);
            const float top = tl + (tr - tl) * tx;
            const float bot = bl + (br - bl) * tx;
            const float v = top + (bot - top) * ty;
            o[c] = (v - 128.0f) / 128.0f;
        }
        o[3] = 0.0f;
        const f32x4 out = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4*>(y + 4 * i) = out;
    }
}

// ------------------------------------------------------------------------------------------------ conv
// C[M = n*oh*ow pixels][cout] = im2col(x)[M][K] . W[cout][K]^T, K = kh*kw*cin in (ky, kx, ci) order (KRSC weights).
// Block: 256 threads = 2 x 2 waves, tile 64 pixels x 64 couts, K-step 16.  Each thread loads one 16-byte chunk of the A tile
// and one of the B tile per step (row tid / 4, chunk tid % 4); cin % 4 == 0 keeps a chunk inside one tap.  The next step's
// chunks are loaded while the current step's MFMAs run.  Each wave owns a 32 x 32 accumulator (32x32x2 f32: lane l holds
// A[row l & 31][k l >> 5] and B[k l >> 5][col l & 31]; a 16-byte fragment read covers four k-pairs).
constexpr int CBM = 64, CBN = 64, CKS = 16, CLD = CKS + 4;     // LDS row stride 20 floats (80 B): rows spread over the banks

struct ConvGeomF {
    const float* x; const float* w; const float* bias; float* y;
    int h, w_, cin, oh, ow, cout, kh, kw, stride, ph, pw, c_total, c_off, K;
    int64_t m;
};

__global__ __launch_bounds__(256) void fid_conv_kernel(ConvGeomF g) {
    __shared__ __attribute__((aligned(16))) float sa[CBM * CLD];
    __shared__ __attribute__((aligned(16))) float sb[CBN * CLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * CBM;
    const int n0 = blockIdx.y * CBN;

    // load slot of this thread
    const int lr = tid >> 2, lc = (tid & 3) * 4;
    const int64_t m = m0 + lr;
    const bool mok = m < g.m;
    int iy0 = 0, ix0 = 0;
    const float* ximg = g.x;
    if (mok) {
        const int64_t ohw = (int64_t)g.oh * g.ow;
        const int64_t img = m / ohw;
        const int rem = (int)(m - img * ohw);
        const int oy = rem / g.ow, ox = rem - oy * g.ow;
        iy0 = oy * g.stride - g.ph;
        ix0 = ox * g.stride - g.pw;
        ximg = g.x + img * g.h * g.w_ * g.cin;
    }
    const int co_ld = n0 + lr;
    const bool cok = co_ld < g.cout;
    const float* wrow = g.w + (int64_t)(cok ? co_ld : 0) * g.K;

    int k = lc, ky = 0, kx = 0, ci = lc;
    while (ci >= g.cin) { ci -= g.cin; if (++kx == g.kw) { kx = 0; ++ky; } }

    f32x4 ra, rb;
    auto load = [&]() {
        ra = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        rb = ra;
        if (k < g.K) {
            const int iy = iy0 + ky, ix = ix0 + kx;
            if (mok && iy >= 0 && iy < g.h && ix >= 0 && ix < g.w_)
                ra = *reinterpret_cast<const f32x4*>(ximg + ((int64_t)iy * g.w_ + ix) * g.cin + ci);
            if (cok) rb = *reinterpret_cast<const f32x4*>(wrow + k);
        }
    };
    load();

    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    f32x16 acc = {};
    const int steps = (g.K + CKS - 1) / CKS;
    for (int s = 0; s < steps; ++s) {
        if (s > 0) __syncthreads();
        *reinterpret_cast<f32x4*>(&sa[lr * CLD + lc]) = ra;
        *reinterpret_cast<f32x4*>(&sb[lr * CLD + lc]) = rb;
        __syncthreads();
        if (s + 1 < steps) {
            k += CKS;
            ci += CKS;
            while (ci >= g.cin) { ci -= g.cin; if (++kx == g.kw) { kx = 0; ++ky; } }
            load();
        }
#pragma unroll
        for (int kk = 0; kk < CKS / 8; ++kk) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&sa[(wm * 32 + fr) * CLD + kk * 8 + fh * 4]);
            const f32x4 b = *reinterpret_cast<const f32x4*>(&sb[(wn * 32 + fr) * CLD + kk * 8 + fh * 4]);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], acc, 0, 0, 0);
        }
    }
    // C/D map of 32x32: col = lane & 31 (cout), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (pixel)
    const int co = n0 + wn * 32 + fr;
    if (co >= g.cout) return;
    const float b = g.bias[co];
    float* yc = g.y + g.c_off + co;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t mm = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        if (mm < g.m) yc[mm * g.c_total] = fmaxf(acc[r] + b, 0.0f);
    }
}

// ------------------------------------------------------------------------------------------------ pools
// 3 x 3 window; mode 0: max (out-of-bounds taps skipped = -inf padding), mode 1: average over the in-bounds taps
// (count_include_pad=False).  A thread owns four channels of one output pixel; the output goes to channels
// [c_off, c_off + c) of a tensor whose pixel stride is c_total.
__global__ __launch_bounds__(256) void fid_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int h, int w,
                                                       int c, int oh, int ow, int stride, int pad, int mode, int c_total, int c_off) {
    const int c4 = c / 4;
    const int64_t total = (int64_t)n * oh * ow * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int cg = (int)(i % c4);
        const int64_t pix = i / c4;
        const int64_t img = pix / ((int64_t)oh * ow);
        const int rem = (int)(pix - img * oh * ow);
        const int oy = rem / ow, ox = rem - oy * ow;
        const float* xi = x + img * h * w * c + 4 * cg;
        float acc[4];
        const float init = mode == 0 ? -INFINITY : 0.0f;
        acc[0] = acc[1] = acc[2] = acc[3] = init;
        int cnt = 0;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * stride - pad + ky;
            if (iy < 0 || iy >= h) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * stride - pad + kx;
                if (ix < 0 || ix >= w) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(xi + ((int64_t)iy * w + ix) * c);
                if (mode == 0) {
                    acc[0] = fmaxf(acc[0], v[0]); acc[1] = fmaxf(acc[1], v[1]);
                    acc[2] = fmaxf(acc[2], v[2]); acc[3] = fmaxf(acc[3], v[3]);
                } else {
                    acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
                }
                ++cnt;
            }
        }
        if (mode == 1) {
            const float d = (float)cnt;
            acc[0] /= d; acc[1] /= d; acc[2] /= d; acc[3] /= d;
        }
        const f32x4 o = {acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<f32x4*>(y + pix * c_total + c_off + 4 * cg) = o;
    }
}

// the global mean over hw pixels: one thread per (image, channel), pixels summed in order
__global__ __launch_bounds__(256) void fid_mean_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int hw, int c) {
    const int64_t total = (int64_t)n * c;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t img = i / c;
        const int ch = (int)(i - img * c);
        const float* p = x + img * hw * c + ch;
        float s = 0.0f;
        for (int q = 0; q < hw; ++q) s += p[(int64_t)q * c];
        y[i] = s / (float)hw;
    }
}

// ------------------------------------------------------------------------------------------------ statistics
// sum[i] += sum_r f[r][i], gram[i][j] += sum_r f[r][i] f[r][j] in fp64.  One thread owns one (i, j) and adds the rows in order
// (fp32 x fp32 products are exact in fp64), so the result is bit-reproducible and G[i][j] == G[j][i] bitwise; several calls
// equal one call on the concatenated rows.
__global__ __launch_bounds__(256) void fid_stats_kernel(const float* __restrict__ f, int n, int d, double* __restrict__ sum,
                                                        double* __restrict__ gram) {
    const int j = blockIdx.x * 16 + (threadIdx.x & 15);
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (i >= d || j >= d) return;
    double* gp = gram + (int64_t)i * d + j;
    double acc = *gp;
    for (int r = 0; r < n; ++r) {
        const float* row = f + (int64_t)r * d;
        acc += (double)row[i] * (double)row[j];
    }
    *gp = acc;
    if (j == 0) {
        double s = sum[i];
        for (int r = 0; r < n; ++r) s += (double)f[(int64_t)r * d + i];
        sum[i] = s;
    }
}

int out_size(int in, int k, int stride, int pad) {
    return in + 2 * pad < k ? 0 : (in + 2 * pad - k) / stride + 1;
}

}  // namespace

extern "C" {

int vqk_fid_preprocess(const float* x, int n, int h, int w, int64_t sn, int64_t sc, int64_t sh, int64_t sw, float* y,
                       void* stream) {
    VQK_REQUIRE(n > 0 && h > 0 && w > 0 && sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0, VQK_ERR_SHAPE);
    VQK_REQUIRE(x && y, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(y), VQK_ERR_ALIGN);
    PreGeom g{n, h, w, sn, sc, sh, sw, (float)((double)h / FID_OUT), (float)((double)w / FID_OUT)};
    const int64_t total = (int64_t)n * FID_OUT * FID_OUT;
    hipLaunchKernelGGL(fid_preprocess_kernel, dim3(vqk_grid_1d(total, 256, 256 * 64)), dim3(256), 0, vqk_stream(stream), x, y, g);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_fid_conv(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int cin, int cout, int kh,
                 int kw, int stride, int ph, int pw, int oh, int ow, int c_total, int c_off, void* stream) {
    VQK_REQUIRE(n > 0 && h > 0 && wd > 0 && cin >= 4 && cin % 4 == 0 && cout > 0, VQK_ERR_SHAPE);
    VQK_REQUIRE(kh >= 1 && kh <= 7 && kw >= 1 && kw <= 7 && (stride == 1 || stride == 2), VQK_ERR_SHAPE);
    VQK_REQUIRE(ph >= 0 && ph < kh && pw >= 0 && pw < kw, VQK_ERR_SHAPE);
    VQK_REQUIRE(oh >= 1 && ow >= 1 && oh == out_size(h, kh, stride, ph) && ow == out_size(wd, kw, stride, pw), VQK_ERR_SHAPE);
    VQK_REQUIRE(c_off >= 0 && c_off + (int64_t)cout <= c_total, VQK_ERR_SHAPE);
    const int64_t K = (int64_t)kh * kw * cin, m = (int64_t)n * oh * ow;
    VQK_REQUIRE(K < (1 << 30) && (m + CBM - 1) / CBM < 0x7fffffff, VQK_ERR_SHAPE);
    VQK_REQUIRE(x && w && bias && y, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(w), VQK_ERR_ALIGN);
    ConvGeomF g{x, w, bias, y, h, wd, cin, oh, ow, cout, kh, kw, stride, ph, pw, c_total, c_off, (int)K, m};
    const dim3 grid((unsigned)((m + CBM - 1) / CBM), (unsigned)((cout + CBN - 1) / CBN));
    hipLaunchKernelGGL(fid_conv_kernel, grid, dim3(256), 0, vqk_stream(stream), g);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_fid_pool(const float* x, float* y, int n, int h, int w, int c, int mode, int stride, int pad, int oh, int ow, int c_total,
                 int c_off, void* stream) {
    VQK_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0 && (mode == 0 || mode == 1), VQK_ERR_SHAPE);
    VQK_REQUIRE((stride == 1 || stride == 2) && (pad == 0 || pad == 1), VQK_ERR_SHAPE);
    VQK_REQUIRE(oh >= 1 && ow >= 1 && oh == out_size(h, 3, stride, pad) && ow == out_size(w, 3, stride, pad), VQK_ERR_SHAPE);
    VQK_REQUIRE(c_off >= 0 && c_off % 4 == 0 && c_total % 4 == 0 && c_off + (int64_t)c <= c_total, VQK_ERR_SHAPE);
    VQK_REQUIRE(x && y, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(y), VQK_ERR_ALIGN);
    const int64_t total = (int64_t)n * oh * ow * (c / 4);
    hipLaunchKernelGGL(fid_pool_kernel, dim3(vqk_grid_1d(total, 256, 256 * 64)), dim3(256), 0, vqk_stream(stream), x, y, n, h, w,
                       c, oh, ow, stride, pad, mode, c_total, c_off);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_fid_mean(const float* x, float* y, int n, int hw, int c, void* stream) {
    VQK_REQUIRE(n > 0 && hw > 0 && c > 0, VQK_ERR_SHAPE);
    VQK_REQUIRE(x && y, VQK_ERR_ARG);
    const int64_t total = (int64_t)n * c;
    hipLaunchKernelGGL(fid_mean_kernel, dim3(vqk_grid_1d(total, 256)), dim3(256), 0, vqk_stream(stream), x, y, n, hw, c);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_fid_stats(const float* f, int n, int d, double* sum, double* gram, void* stream) {
    VQK_REQUIRE(n > 0 && d > 0 && d <= 16384, VQK_ERR_SHAPE);
    VQK_REQUIRE(f && sum && gram, VQK_ERR_ARG);
    const dim3 grid((unsigned)((d + 15) / 16), (unsigned)((d + 15) / 16));
    hipLaunchKernelGGL(fid_stats_kernel, grid, dim3(256), 0, vqk_stream(stream), f, n, d, sum, gram);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // extern "C"
