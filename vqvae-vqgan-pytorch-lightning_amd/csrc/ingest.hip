// Dataset ingest: a ragged batch of packed uint8 HWC RGB images -> fp32 NCHW [N][3][S_h][S_w] in [0,1].
//
// One kernel does what the reference's standard loader does per image on the host (data/datasets.py:16,26: PIL decode ->
// ToTensor() -> Resize((S,S), antialias=True)) minus the decode: u8 / 255 (a true division), an optional crop box, ATen's
// antialiased bilinear resampling (separable triangle filter of support max(scale, 1)) and an optional mirror.
//
// Shape: a block of 256 threads owns a tile of 16 output rows x 64 output columns of ONE image.  It walks the source rows that
// tile needs in chunks of kChunk rows: the horizontal pass resamples each source row of the chunk to the tile's 64 columns
// (3 channels) into LDS, the vertical pass adds the chunk's rows into per-thread accumulators (4 output rows x 3 channels
// each).  Chunking, not a tile that shrinks with the ratio, keeps LDS constant (24 KiB + the 1 KiB u8 table) at EVERY ratio: a 16384 -> 1 reduction
// needs 32768 source rows for one output row.  Taps are added in ascending source order by one thread: no atomics, the result
// is bit-reproducible.  Weights come from the output coordinate in registers, in fp64 (c = scale (i + 0.5) reaches 16384, where
// an fp32 ulp is 1e-3 of a pixel), rounded to fp32 per tap; products and sums are fp32.  At scale == 1 the taps are exactly
// {1, 0}, so the output is float(u8) / 255.0f bit for bit.
//
// Source bytes are fetched as aligned 4-byte words (a pixel is 3 bytes: rows start at any byte) and picked apart in registers; a
// word that would straddle the end of the buffer is assembled from single bytes so no load leaves [0, pixels_bytes).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileCols = 64;
constexpr int kRowsPerThread = 4;
constexpr int kTileRows = (kThreads / kTileCols) * kRowsPerThread;      // 16
constexpr int kChunk = 32;                                              // source rows per LDS chunk: 32 * 3 * 64 * 4 B = 24 KiB
constexpr int kMaxBlocks = 2048;
static_assert(kThreads == 256, "one thread per entry of the u8 table");

// one output coordinate of one axis: the taps [lo, hi) of the box and the triangle's centre / inverse support
struct Axis {
    double c, inv;
    int lo, hi;
};

__device__ __forceinline__ Axis axis_of(int i, int len, int out) {
    const double scale = (double)len / (double)out;
    const double support = scale > 1.0 ? scale : 1.0;
    Axis a;
    a.inv = 1.0 / support;
    a.c = scale * ((double)i + 0.5);
    const int lo = (int)(a.c - support + 0.5), hi = (int)(a.c + support + 0.5);
    a.lo = lo > 0 ? lo : 0;
    a.hi = hi < len ? hi : len;
    return a;
}

__device__ __forceinline__ float tap_weight(const Axis& a, int j) {
    const double t = fabs(((double)j - a.c + 0.5) * a.inv);
    return t < 1.0 ? (float)(1.0 - t) : 0.0f;
}

// bytes of the packed buffer through aligned 32-bit words, the last fetched word kept
struct ByteReader {
    const uint8_t* base;
    int64_t nbytes, cur;
    uint32_t word;
    __device__ __forceinline__ uint32_t get(int64_t b) {
        const int64_t w = b >> 2;
        if (w != cur) {
            cur = w;
            if (4 * w + 4 <= nbytes) {
                word = *reinterpret_cast<const uint32_t*>(base + 4 * w);
            } else {
                word = 0;
                for (int k = 0; k < 4; ++k)
                    if (4 * w + k < nbytes) word |= (uint32_t)base[4 * w + k] << (8 * k);
            }
        }
        return (word >> (8 * (int)(b & 3))) & 255u;
    }
};

__global__ __launch_bounds__(kThreads) void ingest_u8_kernel(const uint8_t* __restrict__ pixels, int64_t pixels_bytes,
                                                              const vqk_ingest_desc* __restrict__ desc, int n, int out_h, int out_w,
                                                              int64_t batch_stride, float* __restrict__ out) {
    __shared__ float rows[kChunk][3][kTileCols];
    __shared__ float unit[256];                                     // u8 -> float(u8) / 255.0f: the true division, once per block
    unit[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    const int tcols = (out_w + kTileCols - 1) / kTileCols, trows = (out_h + kTileRows - 1) / kTileRows;
    const int64_t tiles = (int64_t)n * trows * tcols;
    const int col = threadIdx.x % kTileCols, rslot = threadIdx.x / kTileCols;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int img = (int)(tile / (trows * tcols));
        const int tr = (int)(tile % (trows * tcols)) / tcols, tc = (int)(tile % tcols);
        const vqk_ingest_desc d = desc[img];
        const int oc = tc * kTileCols + col;                        // output column of this thread (both passes)
        const bool col_ok = oc < out_w;
        const Axis ax = axis_of(col_ok ? (d.flip ? out_w - 1 - oc : oc) : 0, d.bw, out_w);
        float wsum_x = 0.f;
        for (int j = ax.lo; j < ax.hi; ++j) wsum_x += tap_weight(ax, j);
        // the tile's output rows and the source rows they need (lo and hi are non-decreasing in the output row)
        const int r0 = tr * kTileRows, r1 = min(r0 + kTileRows, out_h);
        const int ylo = axis_of(r0, d.bh, out_h).lo, yhi = axis_of(r1 - 1, d.bh, out_h).hi;
        Axis ay[kRowsPerThread];
        float acc[kRowsPerThread][3], wsum_y[kRowsPerThread];
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            const int r = r0 + rslot * kRowsPerThread + k;
            ay[k] = axis_of(r < out_h ? r : out_h - 1, d.bh, out_h);
            if (r >= out_h) ay[k].hi = ay[k].lo;                    // no taps: nothing is accumulated, nothing stored
            acc[k][0] = acc[k][1] = acc[k][2] = wsum_y[k] = 0.f;
        }
        ByteReader rd{pixels, pixels_bytes, -1, 0u};
        for (int cy0 = ylo; cy0 < yhi; cy0 += kChunk) {
            const int cy1 = min(cy0 + kChunk, yhi);
            // horizontal pass: source rows [cy0, cy1) of the box -> rows[][3][64]
            if (col_ok) {
                for (int y = cy0 + rslot; y < cy1; y += kThreads / kTileCols) {
                    int64_t b = d.offset + (int64_t)(d.y0 + y) * d.stride + 3 * (int64_t)(d.x0 + ax.lo);
                    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
                    for (int j = ax.lo; j < ax.hi; ++j, b += 3) {
                        const float wt = tap_weight(ax, j);
                        s0 += wt * unit[rd.get(b)];
                        s1 += wt * unit[rd.get(b + 1)];
                        s2 += wt * unit[rd.get(b + 2)];
                    }
                    rows[y - cy0][0][col] = s0 / wsum_x;
                    rows[y - cy0][1][col] = s1 / wsum_x;
                    rows[y - cy0][2][col] = s2 / wsum_x;
                }
            }
            __syncthreads();
            // vertical pass: this chunk's share of every output row of the tile
            if (col_ok) {
#pragma unroll
                for (int k = 0; k < kRowsPerThread; ++k) {
                    const int j0 = max(ay[k].lo, cy0), j1 = min(ay[k].hi, cy1);
                    for (int j = j0; j < j1; ++j) {
                        const float wt = tap_weight(ay[k], j);
                        wsum_y[k] += wt;
                        acc[k][0] += wt * rows[j - cy0][0][col];
                        acc[k][1] += wt * rows[j - cy0][1][col];
                        acc[k][2] += wt * rows[j - cy0][2][col];
                    }
                }
            }
            __syncthreads();
        }
        if (col_ok) {
            float* o = out + (int64_t)img * batch_stride;
            const int64_t plane = (int64_t)out_h * out_w;
#pragma unroll
            for (int k = 0; k < kRowsPerThread; ++k) {
                const int r = r0 + rslot * kRowsPerThread + k;
                if (r < out_h) {
                    const int64_t at = (int64_t)r * out_w + oc;
                    o[at] = acc[k][0] / wsum_y[k];
                    o[plane + at] = acc[k][1] / wsum_y[k];
                    o[2 * plane + at] = acc[k][2] / wsum_y[k];
                }
            }
        }
    }
}

}  // namespace

extern "C" int vqk_ingest_u8(const void* pixels, int64_t pixels_bytes, const vqk_ingest_desc* desc_host,
                             const vqk_ingest_desc* desc_dev, int n, int out_h, int out_w, int64_t out_batch_stride, float* out,
                             void* stream) {
    VQK_REQUIRE(pixels && desc_host && desc_dev && out, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 1 && out_h >= 1 && out_h <= VQK_INGEST_MAX_OUT && out_w >= 1 && out_w <= VQK_INGEST_MAX_OUT, VQK_ERR_SHAPE);
    VQK_REQUIRE(pixels_bytes >= 1 && out_batch_stride >= 3 * (int64_t)out_h * out_w, VQK_ERR_SHAPE);
    VQK_REQUIRE((reinterpret_cast<uintptr_t>(pixels) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(desc_dev) & 7u) == 0, VQK_ERR_ALIGN);
    for (int i = 0; i < n; ++i) {
        const vqk_ingest_desc& d = desc_host[i];
        VQK_REQUIRE(d.h >= 1 && d.h <= VQK_INGEST_MAX_SIDE && d.w >= 1 && d.w <= VQK_INGEST_MAX_SIDE, VQK_ERR_SHAPE);
        VQK_REQUIRE(d.stride >= 3 * d.w && d.offset >= 0, VQK_ERR_SHAPE);
        VQK_REQUIRE(d.x0 >= 0 && d.y0 >= 0 && d.bw >= 1 && d.bh >= 1 && d.bw <= d.w - d.x0 && d.bh <= d.h - d.y0, VQK_ERR_SHAPE);
        VQK_REQUIRE(d.offset <= pixels_bytes && (int64_t)(d.h - 1) * d.stride + 3 * (int64_t)d.w <= pixels_bytes - d.offset,
                    VQK_ERR_SHAPE);
    }
    const int64_t tiles = (int64_t)n * ((out_h + kTileRows - 1) / kTileRows) * ((out_w + kTileCols - 1) / kTileCols);
    const dim3 grid((unsigned)(tiles < kMaxBlocks ? tiles : kMaxBlocks));
    hipLaunchKernelGGL(ingest_u8_kernel, grid, dim3(kThreads), 0, vqk_stream(stream), (const uint8_t*)pixels, pixels_bytes, desc_dev, n,
                       out_h, out_w, out_batch_stride, out);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}
