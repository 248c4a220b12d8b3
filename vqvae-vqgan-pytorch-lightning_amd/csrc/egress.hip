// Image egress: fp32 / bf16 image tensors -> one uint8 HWC RGB canvas (a make_grid panel, or a stack of plain images).
//
// The mirror image of ingest.hip.  The canvas is the thing the kernel walks: a call owns a BAND of whole canvas rows (the cell
// rows its images fill; the last band also the closing padding rows), which is one contiguous byte range.  A thread owns one
// 16-byte span of that range, aligned on its ADDRESS (image rows start 3 * pad bytes into a canvas row and a canvas row is
// 3 * W_g bytes long, so nothing about the images is dword-aligned): 16 bytes are at most 6 pixels.  For each of the 6 it works
// out where the pixel lies -- padding, an empty cell, or (image, y, x) -- reads the source pixel in place through the caller's
// element strides, quantises the three channels, and the 18-byte stream of the 6 pixels is shifted by the span's first channel
// into four dwords: ONE dwordx4 store per thread.  The spans at the two ends of the band are written byte by byte, so nothing
// outside the band is touched, whatever the canvas pointer's alignment.  A source whose channels are contiguous and whose pixels
// are 16-byte (fp32) / 8-byte (bf16) aligned with a fourth channel behind the three (the padded NHWC tensors of the step) is
// read with one vector load per pixel; anything else (plain NCHW) with three scalar loads, which are contiguous across lanes.
// Every load is unconditional (a pixel of padding reads element 0 and drops it), so the 6 loads of a thread are in flight
// together.  No LDS, no atomics.
//
// Quantisation, every operation rounded on its own (the rule of torchvision.utils.save_image):
//     t = clip(x * 0.5f + 0.5f, 0, 1)   ('sym')      t = clip(x, 0, 1)   ('unit')      q = (uint8) floorf(t * 255.0f + 0.5f)
// The rule is specified with two roundings in t * 255 + 0.5, an FMA has one: contraction is off for this file, by the pragma
// below and by -ffp-contract=off in the Makefile (check the ISA for v_fma / v_fmac after touching this file).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;

struct EgressArgs {
    const void* src;
    int64_t sn, sc, sy, sx;         // element strides of the source
    uint8_t* band;                  // first byte of the band
    int n, h, w;
    int rows, cols, row0, pad;
    int hp, wp, wg;                 // h + pad, w + pad, canvas width in pixels
    int y0;                         // first canvas row of the band
    int band_pixels, band_bytes;
    int lead;                       // band address & 15: span c covers band bytes [16 c - lead, 16 c - lead + 16)
    int chunks;
    int sym;
    uint32_t padv;                  // pad_value in the three low bytes
};

__device__ __forceinline__ uint32_t quantise(float x, int sym) {
    // plain products and sums under the pragma above (HIP's __fmul_rn / __fadd_rn are inline x * y / x + y of a header that was
    // parsed with contraction allowed: the pair would still fuse)
    float t = x;
    if (sym) {
        t = x * 0.5f;
        t = t + 0.5f;
    }
    t = fminf(fmaxf(t, 0.0f), 1.0f);                                // fmaxf(NaN, 0) = 0: NaN -> 0, -Inf -> 0, +Inf -> 255
    float u = t * 255.0f;
    u = u + 0.5f;
    return (uint32_t)floorf(u);
}

template <typename T, bool VEC> struct Pixel;
template <> struct Pixel<float, true> {
    __device__ static __forceinline__ void ld(const float* p, int64_t, float (&v)[3]) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    }
};
template <> struct Pixel<float, false> {
    __device__ static __forceinline__ void ld(const float* p, int64_t sc, float (&v)[3]) {
        v[0] = p[0]; v[1] = p[sc]; v[2] = p[2 * sc];
    }
};
template <> struct Pixel<bf16_raw, true> {
    __device__ static __forceinline__ void ld(const bf16_raw* p, int64_t, float (&v)[3]) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        v[0] = __uint_as_float(q.x << 16); v[1] = __uint_as_float(q.x & 0xffff0000u); v[2] = __uint_as_float(q.y << 16);
    }
};
template <> struct Pixel<bf16_raw, false> {
    __device__ static __forceinline__ void ld(const bf16_raw* p, int64_t sc, float (&v)[3]) {
        v[0] = bf16_to_f32(p[0]); v[1] = bf16_to_f32(p[sc]); v[2] = bf16_to_f32(p[2 * sc]);
    }
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void egress_u8_kernel(const EgressArgs a) {
    const T* __restrict__ src = reinterpret_cast<const T*>(a.src);
    for (int ch = blockIdx.x * kThreads + threadIdx.x; ch < a.chunks; ch += gridDim.x * kThreads) {
        const int rel = 16 * ch - a.lead;                           // band byte of the span's first byte: >= -15
        const int t = rel + 15;
        const int p0 = t / 3 - 5, c0 = t % 3;                       // its pixel (band-relative) and channel
        uint32_t rgb[6];
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const int p = p0 + s;
            const bool in_band = p >= 0 && p < a.band_pixels;
            const int pc = in_band ? p : 0;
            const int y = a.y0 + pc / a.wg, x = pc % a.wg;
            const int cy = y / a.hp, iy = y % a.hp - a.pad;         // cy == rows: the closing padding rows
            const int cx = x / a.wp, ix = x % a.wp - a.pad;         // cx == cols: the closing padding columns
            const int k = (cy - a.row0) * a.cols + cx;
            const bool img = in_band && cy < a.rows && cx < a.cols && iy >= 0 && ix >= 0 && k < a.n;
            const int64_t off = img ? (int64_t)k * a.sn + (int64_t)iy * a.sy + (int64_t)ix * a.sx : 0;
            float v[3];
            Pixel<T, VEC>::ld(src + off, a.sc, v);
            const uint32_t q = quantise(v[0], a.sym) | (quantise(v[1], a.sym) << 8) | (quantise(v[2], a.sym) << 16);
            rgb[s] = img ? q : a.padv;
        }
        // the 18 bytes of the 6 pixels as dwords, then the 16 from byte c0 on
        const uint32_t w0 = rgb[0] | (rgb[1] << 24), w1 = (rgb[1] >> 8) | (rgb[2] << 16), w2 = (rgb[2] >> 16) | (rgb[3] << 8);
        const uint32_t w3 = rgb[4] | (rgb[5] << 24), w4 = rgb[5] >> 8;
        const int sh = 8 * c0;
        vqk_u32x4 o;
        o[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
        o[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
        o[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
        o[3] = (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh);
        uint8_t* dst = a.band + rel;
        if (rel >= 0 && rel + 16 <= a.band_bytes) {
            *reinterpret_cast<vqk_u32x4*>(dst) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (rel + j >= 0 && rel + j < a.band_bytes) dst[j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
        }
    }
}

template <typename T, bool VEC> void launch(const EgressArgs& a, hipStream_t stream) {
    const int blocks = (a.chunks + kThreads - 1) / kThreads;
    hipLaunchKernelGGL((egress_u8_kernel<T, VEC>), dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), dim3(kThreads), 0,
                       stream, a);
}

int64_t canvas_bytes(int h, int w, int rows, int cols, int pad) {
    if (h < 1 || h > VQK_EGRESS_MAX_SIDE || w < 1 || w > VQK_EGRESS_MAX_SIDE || rows < 1 || cols < 1 || pad < 0 ||
        pad > VQK_EGRESS_MAX_SIDE)
        return -1;
    const int64_t hg = (int64_t)rows * (h + pad) + pad, wg = (int64_t)cols * (w + pad) + pad;
    if (hg >= (int64_t)1 << 31 || wg >= (int64_t)1 << 31) return -1;
    const int64_t px = hg * wg;                                     // < 2^62
    return px <= (((int64_t)1 << 31) - 1) / 3 ? 3 * px : -1;
}

}  // namespace

extern "C" int64_t vqk_egress_canvas_bytes(int h, int w, int rows, int cols, int pad) { return canvas_bytes(h, w, rows, cols, pad); }

extern "C" int vqk_egress_u8(int dtype, const void* src, int n, int c, int h, int w, int64_t stride_n, int64_t stride_c,
                             int64_t stride_y, int64_t stride_x, int value_range, uint8_t* canvas, int rows, int cols, int row0,
                             int pad, int pad_value, void* stream) {
    VQK_REQUIRE(src && canvas, VQK_ERR_ARG);
    VQK_REQUIRE(dtype == VQK_F32 || dtype == VQK_BF16, VQK_ERR_SHAPE);
    VQK_REQUIRE(value_range == VQK_RANGE_UNIT || value_range == VQK_RANGE_SYM, VQK_ERR_SHAPE);
    VQK_REQUIRE(n >= 1 && c >= 3 && pad_value >= 0 && pad_value <= 255, VQK_ERR_SHAPE);
    const int64_t total = canvas_bytes(h, w, rows, cols, pad);
    VQK_REQUIRE(total > 0, VQK_ERR_SHAPE);
    const int nr = (int)(((int64_t)n + cols - 1) / cols);           // cell rows this call fills
    VQK_REQUIRE(row0 >= 0 && row0 <= rows - nr, VQK_ERR_SHAPE);
    const size_t esize = dtype == VQK_F32 ? 4 : 2;
    VQK_REQUIRE((reinterpret_cast<uintptr_t>(src) & (esize - 1)) == 0, VQK_ERR_ALIGN);

    EgressArgs a;
    a.src = src;
    a.sn = stride_n; a.sc = stride_c; a.sy = stride_y; a.sx = stride_x;
    a.n = n; a.h = h; a.w = w;
    a.rows = rows; a.cols = cols; a.row0 = row0; a.pad = pad;
    a.hp = h + pad; a.wp = w + pad; a.wg = cols * a.wp + pad;
    a.y0 = row0 * a.hp;
    const int y1 = (row0 + nr) * a.hp + (row0 + nr == rows ? pad : 0);
    a.band_pixels = (y1 - a.y0) * a.wg;
    a.band_bytes = 3 * a.band_pixels;
    a.band = canvas + 3 * (int64_t)a.y0 * a.wg;
    a.lead = (int)(reinterpret_cast<uintptr_t>(a.band) & 15u);
    a.chunks = (int)(((int64_t)a.lead + a.band_bytes + 15) / 16);
    a.sym = value_range == VQK_RANGE_SYM;
    a.padv = (uint32_t)pad_value * 0x010101u;
    // one vector load per pixel: contiguous channels, a fourth element behind the three, every pixel on the vector's alignment
    const uintptr_t valign = 4 * esize - 1;                          // 16 bytes of fp32, 8 bytes of bf16
    const bool vec = stride_c == 1 && c >= 4 && (reinterpret_cast<uintptr_t>(src) & valign) == 0 && stride_n % 4 == 0 &&
                     stride_y % 4 == 0 && stride_x % 4 == 0;
    hipStream_t st = vqk_stream(stream);
    if (dtype == VQK_F32) {
        if (vec) launch<float, true>(a, st); else launch<float, false>(a, st);
    } else {
        if (vec) launch<bf16_raw, true>(a, st); else launch<bf16_raw, false>(a, st);
    }
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}
