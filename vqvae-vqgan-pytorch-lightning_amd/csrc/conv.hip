// Implicit-GEMM convolution for gfx950, forward pass: fprop kernels and their launchers, NHWC, bf16
// (v_mfma_f32_32x32x16_bf16) and exact fp32 (v_mfma_f32_32x32x2_f32) with fp32 accumulation.  The data gradient is the
// same kernels on repacked weights (conv_pack.hip builds every weight operand); the weight gradients are in conv_wgrad.hip.
// Replaces the F.conv2d calls of vqvae/modules/autoencoder.py:57-60, :102-105, :114, :132, :153, :170
// (3x3 / 1x1, stride 1, 'same' padding) including the nearest x2 upsample of :104-106, which is folded
// into the input addressing.
//
// conv_fprop_kernel:  C[M = N*H*W pixels][Cout] = im2col(x)[M][ks*ks*Cin] . W[Cout][ks*ks*Cin]^T
//   block 256 threads = 2x2 waves, tile 128 pixels x 128 couts, K-step = 8 chunks of 16 bytes
//   (64 bf16 / 32 fp32 channels).  Both tiles are [128 rows][128 B] in LDS, filled by
//   global_load_lds (16 B per lane, the im2col gather is done by the per-lane SOURCE address; padding
//   rows read a caller-provided zero page), XOR-swizzled on the source side so that the ds_read_b128
//   fragment reads are bank-conflict-free.  Also serves strided / padded / odd shapes (vqk_conv2d_general) and the parity
//   classes of the stride-2 data gradient; split-K partials are combined by conv_splitk_epilogue_kernel.
// conv3x3_halo_kernel / conv3x3_halo_breg_kernel / conv3x3_stream_kernel: 3x3 convs on pixel patches with a halo (weights
//   staged in LDS / held in registers from the fragment-major operand / a persistent software pipeline over tiles).
// conv3x3_thin_in_kernel: the 3-channel input conv on the padded 8-channel image.
// The launchers at the end of the file choose among these and the kernels of conv_mx.hip, conv_x3.hip, conv_thin_f32.hip and
// conv_edge.hip (vqk_conv_weight_layout tells callers which weight operand the choice wants).
#include "conv_geom.h"
#include <type_traits>
#include <stdlib.h>
#include <math.h>

namespace {

using vqkd::ConvGeom;
using vqkd::xcd_remap;
using vqkd::pack_bf16x2;

// epilogue activations: 0 none, 1 tanh, 2 relu, 3 leaky relu (slope 0.2)
__device__ __forceinline__ float epi_act(float v, int act) {
    if (act == 1) return tanhf(v);
    if (act == 2) return fmaxf(v, 0.0f);
    if (act == 3) return v > 0.0f ? v : 0.2f * v;
    return v;
}
// the non-tanh activations without control flow (act is a run-time value: a branch per element serialises an epilogue)
__device__ __forceinline__ float epi_act_sel(float v, int act) {
    const float lo = act == 2 ? 0.0f : act == 3 ? 0.2f * v : v;  // relu: max(v, 0); lrelu: max(v, 0.2 v); linear: max(v, v)
    return fmaxf(v, lo);
}


template <typename T> struct Mma;
template <> struct Mma<bf16_raw> {
    static constexpr int EPC = 8;     // elements per 16-byte chunk
    __device__ static __forceinline__ void run(const char* pa, const char* pb, f32x16& acc) {
        const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(pa);
        const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(pb);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static constexpr int EPC = 4;
    __device__ static __forceinline__ void run(const char* pa, const char* pb, f32x16& acc) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(pa);
        const f32x4 b = *reinterpret_cast<const f32x4*>(pb);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], acc, 0, 0, 0);
    }
};

template <typename T> struct Frag;
template <> struct Frag<bf16_raw> {
    typedef bf16x8_t type;
    __device__ static __forceinline__ void mma(const type& a, const type& b, f32x16& acc) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
};
template <> struct Frag<float> {
    typedef f32x4 type;
    __device__ static __forceinline__ void mma(const type& a, const type& b, f32x16& acc) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], acc, 0, 0, 0);
    }
};

__device__ __forceinline__ void store4(float* p, const float (&v)[4]) {
    f32x4 o = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = o;
}
__device__ __forceinline__ void store4(bf16_raw* p, const float (&v)[4]) {
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    const u32x2 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    *reinterpret_cast<u32x2*>(p) = o;
}
// v[0..3] += four consecutive residual elements (one 8-byte / 16-byte load)
__device__ __forceinline__ void add4(const bf16_raw* p, float (&v)[4]) {
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    const u32x2 r = *reinterpret_cast<const u32x2*>(p);
    v[0] += __uint_as_float(r[0] << 16); v[1] += __uint_as_float(r[0] & 0xffff0000u);
    v[2] += __uint_as_float(r[1] << 16); v[3] += __uint_as_float(r[1] & 0xffff0000u);
}
__device__ __forceinline__ void add4(const float* p, float (&v)[4]) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(p);
    v[0] += r[0]; v[1] += r[1]; v[2] += r[2]; v[3] += r[3];
}

__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const VQK_GLB void*)src, (VQK_LDS void*)lds_wave_base, 16, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// fprop / dgrad
// ------------------------------------------------------------------------------------------------
template <typename T, typename TO, bool FASTK>
__global__ __launch_bounds__(256, 2) void conv_fprop_kernel(const T* __restrict__ x, const T* __restrict__ wgt,
                                                            const float* __restrict__ bias, const TO* __restrict__ res,
                                                            TO* __restrict__ y, const char* __restrict__ zeros,
                                                            ConvGeom g, int act, float* __restrict__ skws = nullptr,
                                                            int steps_per_split = 0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lds_a = smem;              // [128][128 B]
    char* lds_b = smem + 16384;      // [128][128 B]
    constexpr int EPC = Mma<T>::EPC;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = xcd_remap(blockIdx.x, g.tiles_m * g.tiles_n);
    const int mt = tile / g.tiles_n, nt = tile - mt * g.tiles_n;
    const int m0 = mt * 128, n0 = nt * 128;

    // ---- per-lane load slots: 4 A rows + 4 B rows (row = 8*(4*wave+t) + lane/8), fixed over K
    int a_oh[4], a_ow[4];
    const T* a_img[4];
    const char* b_row[4];
    bool b_ok[4];
    int lchunk[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = 8 * (4 * wave + t) + (lane >> 3);
        const int m = m0 + r;
        if (m < g.m) {
            if (g.sub) {
                const int hw = g.sub_h * g.sub_w;
                const int img = m / hw, rem = m - img * hw;
                const int a = rem / g.sub_w;
                a_oh[t] = 2 * a + g.sub_py;
                a_ow[t] = 2 * (rem - a * g.sub_w) + g.sub_px;
                a_img[t] = x + (int64_t)img * g.h_in * g.w_in * g.cin;
            } else {
                const int hw = g.h * g.w;
                const int img = m / hw, rem = m - img * hw;
                a_oh[t] = rem / g.w;
                a_ow[t] = rem - a_oh[t] * g.w;
                a_img[t] = x + (int64_t)img * g.h_in * g.w_in * g.cin;
            }
        } else {
            a_oh[t] = -1000000; a_ow[t] = 0; a_img[t] = x;
        }
        const int co = n0 + r;
        b_ok[t] = co < g.cout;
        b_row[t] = reinterpret_cast<const char*>(wgt) + (int64_t)(b_ok[t] ? co : 0) * g.wrow_chunks * 16;
    }
    // logical chunk held by this lane's physical LDS slot (swizzle: phys = logical ^ ((row>>1)&7))
    lchunk[0] = (lane & 7) ^ ((lane >> 4) & 7);
    lchunk[1] = (lane & 7) ^ ((4 + (lane >> 4)) & 7);

    const int wm = wave >> 1, wn = wave & 1;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // fragment read offsets (bytes): row*128 + ((2*ks + kg) ^ ((row>>1)&7))*16
    const int frow = lane & 31, kg = lane >> 5;
    int fa[2], fb[2], fsw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ra = wm * 64 + i * 32 + frow, rb = wn * 64 + i * 32 + frow;
        fa[i] = ra * 128; fb[i] = rb * 128;
        fsw[i] = 0;
    }
    const int swz = (frow >> 1) & 7;   // identical for A and B rows (tile bases are multiples of 32)
    (void)fsw;

    const int ksteps = (g.kchunks + 7) >> 3;
    const int steps_per_tap = FASTK ? (g.cpt >> 3) : 1;
    // split-K (tiny pixel counts with a long K: the 4x4 / 8x8 maps and the fully connected layer of the discriminator run as
    // 8-32 blocks otherwise): blockIdx.y owns a range of k-steps and a private slice of the scratch `skws`
    const int s_begin = skws ? (int)blockIdx.y * steps_per_split : 0;
    const int s_end = skws ? min(ksteps, s_begin + steps_per_split) : ksteps;

    // (a second LDS stage -- loads of step s + 1 in flight under the MFMAs of step s -- was measured on the VQ-GAN layer list:
    // no gain on small grids, -15 % on large ones, where it halves the resident blocks; tools/db_sweep.sh, round 3)
    auto stage = [&](int s) {
        // ---------------- stage: 4 A + 4 B 16-byte pieces per lane
        int tap_u = 0, kh_u = 0, kw_u = 0, cbase_u = 0;
        if (FASTK) {
            tap_u = s / steps_per_tap;
            if (g.sub) { const int q = tap_u / g.nkw; kh_u = g.khl[q]; kw_u = g.kwl[tap_u - q * g.nkw]; }
            else { kh_u = tap_u / g.ks; kw_u = tap_u - kh_u * g.ks; }
            cbase_u = (s - tap_u * steps_per_tap) * 8;     // chunk offset inside the tap
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int lc = lchunk[t & 1];
            const int gch = s * 8 + lc;                      // global chunk index along K
            int kh, kw, coff;
            bool ok = true;
            if (FASTK) { kh = kh_u; kw = kw_u; coff = cbase_u + lc; }
            else {
                ok = gch < g.kchunks;
                const int tap = gch / g.cpt;
                coff = gch - tap * g.cpt;
                if (g.sub) { const int q = ok ? tap / g.nkw : 0; kh = g.khl[q]; kw = g.kwl[ok ? tap - q * g.nkw : 0]; }
                else { kh = tap / g.ks; kw = tap - kh * g.ks; }
            }
            const int ih = a_oh[t] * g.stride + kh - g.pad, iw = a_ow[t] * g.stride + kw - g.pad;
            ok = ok && ih >= 0 && ih < g.vh && iw >= 0 && iw < g.vw && !(g.zs && ((ih | iw) & 1));
            const T* src = a_img[t] + ((int64_t)(ih >> g.ups) * g.w_in + (iw >> g.ups)) * g.cin + coff * EPC;
            const void* sa = ok ? reinterpret_cast<const void*>(src) : reinterpret_cast<const void*>(zeros);
            glds16(sa, lds_a + (4 * wave + t) * 1024);
            const bool okb = b_ok[t] && gch < g.kchunks;
            const int wch = g.sub ? (kh * g.ks + kw) * g.cpt + coff : gch;       // chunk inside the full weight row
            const void* sb = okb ? reinterpret_cast<const void*>(b_row[t] + (int64_t)wch * 16)
                                 : reinterpret_cast<const void*>(zeros);
            glds16(sb, lds_b + (4 * wave + t) * 1024);
        }
    };
    for (int s = s_begin; s < s_end; ++s) {
        stage(s);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // ---------------- compute: 4 k-substeps of two 16-byte chunks
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int poff = ((2 * ks + kg) ^ swz) * 16;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    Mma<T>::run(lds_b + fb[j] + poff, lds_a + fa[i] + poff, acc[i][j]);   // D[cout][pixel]
        }
        __syncthreads();
    }

    // ---------------- epilogue: bias, residual, activation, store.  D[cout][pixel]: a lane owns one pixel (column)
    // and, per MFMA tile, four runs of 4 consecutive couts -> 8 / 16-byte stores
    const int opix = lane & 31, okg = lane >> 5;
    const bool bias16 = (reinterpret_cast<uintptr_t>(bias) & 15) == 0;
    auto epilogue = [&](auto TANH) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 64 + i * 32 + opix;
        if (m >= g.m) continue;
        int64_t orow = (int64_t)m * g.cout;
        if (g.sub) {
            const int hw = g.sub_h * g.sub_w;
            const int img = m / hw, rem = m - img * hw;
            const int a = rem / g.sub_w, b = rem - a * g.sub_w;
            orow = (((int64_t)img * g.h + 2 * a + g.sub_py) * g.w + 2 * b + g.sub_px) * g.cout;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int co = n0 + wn * 64 + j * 32 + 8 * rq + 4 * okg;
                if (co >= g.cout) continue;
                if (skws) {                                      // split-K partial -> this split's private slice (plain stores;
                    float* sl = skws + ((int64_t)blockIdx.y * g.m + m) * g.cout + co;    // conv_splitk_epilogue_kernel sums them)
                    if (co + 3 < g.cout && (g.cout & 3) == 0) {
                        const f32x4 pv = {acc[i][j][4 * rq], acc[i][j][4 * rq + 1], acc[i][j][4 * rq + 2], acc[i][j][4 * rq + 3]};
                        *reinterpret_cast<f32x4*>(sl) = pv;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (co + e < g.cout) sl[e] = acc[i][j][4 * rq + e];
                    }
                    continue;
                }
                float v[4], bq[4] = {0.f, 0.f, 0.f, 0.f};
                if (bias) {
                    if (co + 3 < g.cout && bias16) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + co);     // co % 4 == 0
#pragma unroll
                        for (int e = 0; e < 4; ++e) bq[e] = b4[e];
                    } else {
                        for (int e = 0; e < 4 && co + e < g.cout; ++e) bq[e] = bias[co + e];
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = acc[i][j][4 * rq + e] * g.acc_scale + bq[e];
                    v[e] = (decltype(TANH)::value ? tanhf(t) : epi_act_sel(t, act)) * g.out_gain;
                }
                const int64_t o = orow + co;
                if (co + 3 < g.cout && (g.cout & 3) == 0) {
                    if (res) add4(res + o, v);
                    store4(y + o, v);
                } else {
                    for (int e = 0; e < 4 && co + e < g.cout; ++e) {
                        float t = v[e];
                        if (res) t += Elem<TO>::ld(res + o + e);
                        Elem<TO>::st(y + o + e, t);
                    }
                }
            }
    }
    };
    if (act == 1) epilogue(std::true_type{});
    else epilogue(std::false_type{});
}

// epilogue of the split-K form: y = out_gain * act(sum_s ws[s] * acc_scale + bias) (+ residual).  Every split wrote its own
// slice of the scratch with plain stores and the slices are summed in split order here: no atomics (4.2 M device-scope
// fp32 atomics per 8x8 conv were most of its 123 us), no zero-initialised scratch, the same bits every run.
template <typename TO>
__global__ __launch_bounds__(256) void conv_splitk_epilogue_kernel(const float* __restrict__ ws, const float* __restrict__ bias,
                                                                   const TO* __restrict__ res, TO* __restrict__ y, ConvGeom g,
                                                                   int act, int splits) {
    const int64_t total = (int64_t)g.m * g.cout;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;       // 4 consecutive couts (cout % 4 == 0: launcher)
    if (i >= total) return;
    const int m = (int)(i / g.cout), co = (int)(i - (int64_t)m * g.cout);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int sidx = 0; sidx < splits; ++sidx) a += *reinterpret_cast<const f32x4*>(ws + (int64_t)sidx * total + i);
    int64_t orow = (int64_t)m * g.cout;
    if (g.sub) {                                                 // one output-parity class of a zero-stuffed conv
        const int hw = g.sub_h * g.sub_w;
        const int img = m / hw, rem = m - img * hw;
        const int pa = rem / g.sub_w, pb = rem - pa * g.sub_w;
        orow = (((int64_t)img * g.h + 2 * pa + g.sub_py) * g.w + 2 * pb + g.sub_px) * g.cout;
    }
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = epi_act(a[e] * g.acc_scale + (bias ? bias[co + e] : 0.0f), act) * g.out_gain;
    if (res) add4(res + orow + co, v);
    store4(y + orow + co, v);
}

// ------------------------------------------------------------------------------------------------
// fprop / dgrad, 3x3, "halo" variant: the block owns a TH x TW spatial patch (256 output pixels) x 128
// couts.  For every 128-byte channel chunk the (TH+2) x (TW+2) input halo is staged ONCE and all nine
// taps read it at shifted row offsets, so activation traffic into LDS drops 9x against the im2col
// variant; only the 16 KB weight tile per tap is streamed (double-buffered, prefetched one tap ahead).
// 4 waves as 2(M) x 2(N), wave tile 128 pixels x 64 couts = 4x2 MFMA 32x32 tiles (128 accumulators).
// LDS: halo 44 KB + 2 x 16 KB weights = 76 KB -> two blocks per CU.
// ------------------------------------------------------------------------------------------------
template <typename T, typename TO, int TWLOG>
__global__ __launch_bounds__(256, 2) void conv3x3_halo_kernel(const T* __restrict__ x, const T* __restrict__ wgt,
                                                              const float* __restrict__ bias,
                                                              const TO* __restrict__ res, TO* __restrict__ y,
                                                              const char* __restrict__ zeros, ConvGeom g, int act) {
    constexpr int EPC = Mma<T>::EPC;
    constexpr int TW = 1 << TWLOG, TH = 256 / TW, HW2 = TW + 2, HROWS = (TH + 2) * HW2;
    constexpr int HALO_INSTR = (HROWS + 7) / 8;                 // wave instructions (8 rows each)
    constexpr int HALO_BYTES = ((HALO_INSTR + 3) / 4) * 4 * 1024;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lds_h = smem;
    char* lds_b = smem + HALO_BYTES;                             // 2 x [128][128 B]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = g.w >> TWLOG, tiles_y = g.h / TH;
    const int total = g.n * tiles_y * tiles_x * g.tiles_n;
    int tile = xcd_remap(blockIdx.x, total);
    const int nt = tile % g.tiles_n; tile /= g.tiles_n;
    const int txi = tile % tiles_x; tile /= tiles_x;
    const int tyi = tile % tiles_y;
    const int img = tile / tiles_y;
    const int py0 = tyi * TH, px0 = txi * TW, n0 = nt * 128;
    const T* ximg = x + (int64_t)img * g.h_in * g.w_in * g.cin;

    const int wm = wave >> 1, wn = wave & 1;
    const int p = lane & 31, kg = lane >> 5;
    // halo row of this lane's pixel for MFMA row tile i (tap (0,0)); patch pixel (ty, tx)
    int hbase[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int ty, tx;
        if (TWLOG == 5) { ty = wm * 4 + i; tx = p; }
        else { ty = wm * 8 + 2 * i + (p >> 4); tx = p & 15; }
        hbase[i] = ty * HW2 + tx;
    }
    int fb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = (wn * 64 + j * 32 + p) * 128;
    const int bswz = (p >> 1) & 7;

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // B-tile load slots: row = 8*(4*wave+t) + lane/8, logical chunk as in the im2col kernel
    const char* b_row[4];
    bool b_ok[4];
    int lchunk[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int co = n0 + 8 * (4 * wave + t) + (lane >> 3);
        b_ok[t] = co < g.cout;
        b_row[t] = reinterpret_cast<const char*>(wgt) + (int64_t)(b_ok[t] ? co : 0) * g.kchunks * 16;
    }
    lchunk[0] = (lane & 7) ^ ((lane >> 4) & 7);
    lchunk[1] = (lane & 7) ^ ((4 + (lane >> 4)) & 7);

    const int nchunks = g.cpt >> 3;                              // 128-byte channel chunks
    for (int cc = 0; cc < nchunks; ++cc) {
        __syncthreads();                                         // previous chunk fully consumed
        // ---- halo: HALO_INSTR wave instructions, round-robin over the 4 waves
        for (int q = wave; q < HALO_INSTR; q += 4) {
            const int hr = q * 8 + (lane >> 3);
            const int lc = (lane & 7) ^ ((hr >> 1) & 7);
            const int hy = hr / HW2, hx = hr - hy * HW2;
            const int iy = py0 + hy - 1, ix = px0 + hx - 1;
            const bool ok = hr < HROWS && iy >= 0 && iy < g.h && ix >= 0 && ix < g.w;
            const T* src = ximg + ((int64_t)(iy >> g.ups) * g.w_in + (ix >> g.ups)) * g.cin + (cc * 8 + lc) * EPC;
            glds16(ok ? (const void*)src : (const void*)zeros, lds_h + q * 1024);
        }
        // ---- weights of tap 0
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int gch = cc * 8 + lchunk[t & 1];
            glds16(b_ok[t] ? (const void*)(b_row[t] + (int64_t)gch * 16) : (const void*)zeros,
                   lds_b + (4 * wave + t) * 1024);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const char* bcur = lds_b + (tap & 1) * 16384;
            if (tap < 8) {                                       // prefetch the next tap's weights
                char* bnext = lds_b + ((tap + 1) & 1) * 16384;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int gch = (tap + 1) * g.cpt + cc * 8 + lchunk[t & 1];
                    glds16(b_ok[t] ? (const void*)(b_row[t] + (int64_t)gch * 16) : (const void*)zeros,
                           bnext + (4 * wave + t) * 1024);
                }
            }
            const int kh = tap / 3, kw = tap - kh * 3;
            const int toff = kh * HW2 + kw;
            int ha[4], hs[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int hr = hbase[i] + toff;
                ha[i] = hr * 128;
                hs[i] = (hr >> 1) & 7;
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int lc = 2 * ks + kg;
                const int boff = (lc ^ bswz) * 16;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const char* pa = lds_h + ha[i] + ((lc ^ hs[i]) << 4);
#pragma unroll
                    for (int j = 0; j < 2; ++j) Mma<T>::run(bcur + fb[j] + boff, pa, acc[i][j]);   // D[co][pixel]
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }

    // ---------------- epilogue: lane = one pixel (p) x 4 consecutive couts per register quad
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int ty, tx;
        if (TWLOG == 5) { ty = wm * 4 + i; tx = p; }
        else { ty = wm * 8 + 2 * i + (p >> 4); tx = p & 15; }
        const int64_t pix = ((int64_t)img * g.h + py0 + ty) * g.w + px0 + tx;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int co = n0 + wn * 64 + j * 32 + 8 * rq + 4 * kg;
                if (co >= g.cout) continue;
                const int64_t o = pix * g.cout + co;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    v[e] = epi_act(acc[i][j][4 * rq + e] * g.acc_scale + (bias ? bias[co + e] : 0.0f), act) * g.out_gain;
                if (res) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += Elem<TO>::ld(res + o + e);
                }
                store4(y + o, v);
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Halo variant with the weights in REGISTERS.  Weights are pre-packed "fragment-major"
// (vqk_conv_pack_weights, layout 1): for (cout tile of 32, tap, channel chunk, k-substep) the 64 lanes'
// 16-byte MFMA operands are 1 KiB contiguous, so one coalesced global_load_dwordx4 per fragment, prefetched
// one tap ahead.  LDS holds only the input halo => no barrier inside the nine taps; the block
// synchronises once per 128-byte channel chunk.  4 waves as 2(M) x 2(N), wave tile 128 pixels x 64 couts.
// ------------------------------------------------------------------------------------------------
template <typename T, typename TO, int TWLOG>
__global__ __launch_bounds__(256, 2) void conv3x3_halo_breg_kernel(const T* __restrict__ x, const T* __restrict__ wp,
                                                                   const float* __restrict__ bias,
                                                                   const TO* __restrict__ res, TO* __restrict__ y,
                                                                   const char* __restrict__ zeros, ConvGeom g, int act) {
    constexpr int EPC = Mma<T>::EPC;
    constexpr int TW = 1 << TWLOG, TH = 256 / TW, HW2 = TW + 2, HROWS = (TH + 2) * HW2;
    constexpr int HALO_INSTR = (HROWS + 7) / 8;
    typedef typename Frag<T>::type frag_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lds_h = smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = g.w >> TWLOG, tiles_y = g.h / TH;
    const int total = g.n * tiles_y * tiles_x * g.tiles_n;
    int tile = xcd_remap(blockIdx.x, total);
    const int nt = tile % g.tiles_n; tile /= g.tiles_n;
    const int txi = tile % tiles_x; tile /= tiles_x;
    const int tyi = tile % tiles_y;
    const int img = tile / tiles_y;
    const int py0 = tyi * TH, px0 = txi * TW, n0 = nt * 128;
    const T* ximg = x + (int64_t)img * g.h_in * g.w_in * g.cin;

    const int wm = wave >> 1, wn = wave & 1;
    const int p = lane & 31, kg = lane >> 5;
    int hbase[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int ty, tx;
        if (TWLOG == 5) { ty = wm * 4 + i; tx = p; }
        else { ty = wm * 8 + 2 * i + (p >> 4); tx = p & 15; }
        hbase[i] = ty * HW2 + tx;
    }
    const int nchunks = g.cpt >> 3;
    // fragment (j, tap, cc, ks) of this wave in the [cot][cc32][tap][ks2] layout: cc32 = 2*cc + ks/2, ks2 = ks & 1
    const char* wbase = reinterpret_cast<const char*>(wp) + (int64_t)lane * 16;
    const int cot0 = (n0 + wn * 64) >> 5;
    auto wfrag = [&](int j, int tap, int cc, int ks) -> frag_t {
        const int64_t f = (((int64_t)(cot0 + j) * (2 * nchunks) + 2 * cc + (ks >> 1)) * 9 + tap) * 2 + (ks & 1);
        return *reinterpret_cast<const frag_t*>(wbase + f * 1024);
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    frag_t bw[2][4];                                             // this tap's weight fragments
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) bw[j][ks] = wfrag(j, 0, 0, ks);

    for (int cc = 0; cc < nchunks; ++cc) {
        __syncthreads();                                         // previous chunk's halo fully consumed
        for (int q = wave; q < HALO_INSTR; q += 4) {
            const int hr = q * 8 + (lane >> 3);
            const int lc = (lane & 7) ^ ((hr >> 1) & 7);
            const int hy = hr / HW2, hx = hr - hy * HW2;
            const int iy = py0 + hy - 1, ix = px0 + hx - 1;
            const bool ok = hr < HROWS && iy >= 0 && iy < g.h && ix >= 0 && ix < g.w;
            const T* src = ximg + ((int64_t)(iy >> g.ups) * g.w_in + (ix >> g.ups)) * g.cin + (cc * 8 + lc) * EPC;
            glds16(ok ? (const void*)src : (const void*)zeros, lds_h + q * 1024);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            // next (tap, chunk) whose weights get prefetched; past the end the loads are redundant but stay
            // UNCONDITIONAL so that the compiler's vmcnt bookkeeping stays exact (a branch around them makes it
            // wait for the youngest load at the top of every tap).
            int ntap = tap + 1, ncc = cc;
            if (ntap == 9) { ntap = 0; ncc = (cc + 1 < nchunks) ? cc + 1 : 0; }
            const int kh = tap / 3, kw = tap - kh * 3;
            const int toff = kh * HW2 + kw;
            const char* prow[4];
            int hs[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int hr = hbase[i] + toff;
                prow[i] = lds_h + hr * 128;
                hs[i] = (hr >> 1) & 7;
            }
            frag_t a[2][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[0][i] = *reinterpret_cast<const frag_t*>(prow[i] + ((kg ^ hs[i]) << 4));
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks < 3) {                                    // next k-substep's pixel fragments
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        a[(ks + 1) & 1][i] = *reinterpret_cast<const frag_t*>(prow[i] + (((2 * ks + 2 + kg) ^ hs[i]) << 4));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) Frag<T>::mma(bw[j][ks], a[ks & 1][i], acc[i][j]);       // D[co][pixel]
                // rolling prefetch: these registers are dead until the next tap's k-substep ks
#pragma unroll
                for (int j = 0; j < 2; ++j) bw[j][ks] = wfrag(j, ntap, ncc, ks);
                __builtin_amdgcn_sched_barrier(0);               // keep the prefetch here (hipcc sinks it to the loop end)
            }
        }
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int ty, tx;
        if (TWLOG == 5) { ty = wm * 4 + i; tx = p; }
        else { ty = wm * 8 + 2 * i + (p >> 4); tx = p & 15; }
        const int64_t pix = ((int64_t)img * g.h + py0 + ty) * g.w + px0 + tx;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int co = n0 + wn * 64 + j * 32 + 8 * rq + 4 * kg;
                if (co >= g.cout) continue;
                const int64_t o = pix * g.cout + co;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    v[e] = epi_act(acc[i][j][4 * rq + e] * g.acc_scale + (bias ? bias[co + e] : 0.0f), act) * g.out_gain;
                if (res) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += Elem<TO>::ld(res + o + e);
                }
                store4(y + o, v);
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Persistent "stream" variant of the register-weight halo kernel (bf16).  Each block walks a strided list of
// (patch, cout-tile) tiles; inside a tile it walks 64-byte (32-channel) chunks.  The (tile, chunk) units form
// one continuous software pipeline: while unit u is computed out of LDS buffer u&1, the halo of unit u+1 is in
// flight from HBM into REGISTERS (ordinary loads, so hipcc's counted vmcnt keeps the rolling weight prefetch
// un-drained) and is written to buffer (u+1)&1 after the compute; one barrier per unit.
//
// The inner loop is address-arithmetic free: LDS rows are padded to 80 B (16 consecutive rows -> 16 distinct
// 16-byte bank slots, no XOR swizzle), so a pixel fragment is `lane base + compile-time immediate` for every
// (tap, k-substep); the nine taps are fully unrolled; the weights of one unit are 18 contiguous 1 KiB fragments
// read as `uniform base + lane*16`.  (PMC on the previous version: 4.4 VALU + 4.3 SALU per MFMA, issue-bound.)
// ------------------------------------------------------------------------------------------------
// THIN: couts fit ONE 32-wide MFMA tile (the decoder's 3-channel head, autoencoder.py:170): the four waves split the
// 256 pixels four ways (wave tile 64 pixels x 32 couts) instead of 2 x 2 (128 x 64), cout tiles are 32 wide.
// MODE 2 (half tile): 128-pixel patches (4x32 / 8x16), wave tile 64 pixels x 64 couts -- twice as many tiles for the
// 16^2 / 32^2 maps whose 256-pixel tiling leaves most CUs idle.
template <typename TO, int TWLOG, int MODE>
__global__ __launch_bounds__(256, 2) void conv3x3_stream_kernel(const bf16_raw* __restrict__ x,
                                                                const bf16_raw* __restrict__ wp,
                                                                const float* __restrict__ bias,
                                                                const TO* __restrict__ res, TO* __restrict__ y,
                                                                const char* __restrict__ zeros, ConvGeom g, int act) {
    constexpr bool THIN = MODE == 1;
    constexpr int PIX = MODE == 2 ? 128 : 256;                   // output pixels per tile
    constexpr int TW = 1 << TWLOG, TH = PIX / TW, HW2 = TW + 2, HROWS = (TH + 2) * HW2;
    constexpr int RS = 80;                                       // padded LDS row stride (64 B payload)
    constexpr int HALO_INSTR = (HROWS + 15) / 16;                // register pieces: 16 rows x 64 B per wave load
    constexpr int BUF = 28 * 1024;
    constexpr int NSLOT = (HALO_INSTR + 3) / 4;
    constexpr int NI = MODE == 0 ? 4 : 2, NJ = THIN ? 1 : 2, COT = THIN ? 32 : 128;
    typedef bf16x8_t frag_t;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = g.w >> TWLOG, tiles_y = g.h / TH;
    const int total_tiles = g.n * tiles_y * tiles_x * g.tiles_n;
    const int nch = g.cpt >> 2;                                  // 32-channel chunks
    // consecutive virtual block ids sit on ONE XCD (hardware block b runs on XCD b % 8): the cout tiles of a patch and
    // its neighbouring patches share that XCD's L2 instead of each fetching the halo from HBM
    const int vbid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int my_tiles = (total_tiles - vbid + (int)gridDim.x - 1) / (int)gridDim.x;
    const int units = my_tiles * nch;
    if (units <= 0) return;

    const int wm = THIN ? wave : wave >> 1, wn = THIN ? 0 : wave & 1;
    const int p = lane & 31, kg = lane >> 5;
    auto pix_of = [&](int i, int& ty, int& tx) {                 // patch pixel of this lane in the wave's MFMA tile i
        if (TWLOG == 5) { ty = wm * NI + i; tx = p; }
        else { ty = wm * 2 * NI + 2 * i + (p >> 4); tx = p & 15; }
    };
    unsigned abase[NI];                                          // LDS byte offset of tile i's pixel, tap (0,0), ks 0
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        int ty, tx;
        pix_of(i, ty, tx);
        abase[i] = (unsigned)((ty * HW2 + tx) * RS + kg * 16);
    }
    int slot_hy[NSLOT], slot_hx[NSLOT];
    unsigned slot_dst[NSLOT];
    bool slot_ok[NSLOT];
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) {
        const int q = wave + 4 * sl;
        const int hr = q * 16 + (lane >> 2);
        slot_ok[sl] = q < HALO_INSTR && hr < HROWS;
        slot_hy[sl] = hr / HW2;
        slot_hx[sl] = hr - slot_hy[sl] * HW2;
        slot_dst[sl] = (unsigned)(hr * RS + (lane & 3) * 16);
    }
    const int lchan = (lane & 3) * 8;

    struct TilePos { int img, py0, px0, nt; };
    auto tile_pos = [&](int j) -> TilePos {
        int t = vbid + j * (int)gridDim.x;
        TilePos tp;
        tp.nt = t % g.tiles_n; t /= g.tiles_n;
        const int txi = t % tiles_x; t /= tiles_x;
        const int tyi = t % tiles_y;
        tp.img = t / tiles_y; tp.py0 = tyi * TH; tp.px0 = txi * TW;
        return tp;
    };
    u32x4 hreg[NSLOT];
    auto load_halo = [&](const TilePos& tp, int c) {
        const bf16_raw* ximg = x + (int64_t)tp.img * g.h_in * g.w_in * g.cin + c * 32 + lchan;
#pragma unroll
        for (int sl = 0; sl < NSLOT; ++sl) {
            const int iy = tp.py0 + slot_hy[sl] - 1, ix = tp.px0 + slot_hx[sl] - 1;
            const bool ok = slot_ok[sl] && iy >= 0 && iy < g.h && ix >= 0 && ix < g.w;
            const bf16_raw* src = ximg + ((int64_t)(iy >> g.ups) * g.w_in + (ix >> g.ups)) * g.cin;
            const void* sp = ok ? (const void*)src : (const void*)zeros;      // select, not branch
            hreg[sl] = *reinterpret_cast<const u32x4*>(sp);
        }
    };
    auto store_halo = [&](char* buf) {
#pragma unroll
        for (int sl = 0; sl < NSLOT; ++sl)
            if (wave + 4 * sl < HALO_INSTR) *reinterpret_cast<u32x4*>(buf + slot_dst[sl]) = hreg[sl];
    };
    // weights of unit (cout tile pair of this wave, chunk c): 2 x 18 contiguous 1 KiB fragments
    const unsigned lane16 = (unsigned)lane * 16;
    const char* wroot = reinterpret_cast<const char*>(wp);
    auto unit_w = [&](int nt, int c, int j) -> const char* {
        const int cot = THIN ? nt : nt * 4 + wn * 2 + j;
        return wroot + ((int64_t)cot * nch + c) * (18 * 1024);
    };

    f32x16 acc[NI][NJ];

    TilePos cur = tile_pos(0);
    load_halo(cur, 0);
    frag_t bw[NJ][2];
    const char* wcur[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) wcur[j] = unit_w(cur.nt, 0, j);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) bw[j][ks] = *reinterpret_cast<const frag_t*>(wcur[j] + ks * 1024 + lane16);
    store_halo(smem);
    __syncthreads();

    int tj = 0, c = 0;
    for (int u = 0; u < units; ++u) {
        const unsigned boff = (unsigned)((u & 1) * BUF);
        int ntj = tj, nc = c + 1;
        if (nc == nch) { nc = 0; ntj = tj + 1; }
        const bool has_next = u + 1 < units;
        if (!has_next) { ntj = tj; nc = c; }                     // clamp: loads stay unconditional
        const TilePos nxt = (ntj == tj) ? cur : tile_pos(ntj);
        load_halo(nxt, nc);                                      // in flight during this unit's MFMAs
        const char* wnxt[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) wnxt[j] = unit_w(nxt.nt, nc, j);
        const char* lbase[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) lbase[i] = smem + boff + abase[i];

        // Pixel fragments run one (tap, k-substep) phase ahead of the MFMAs that consume them (the reads of phase p+1
        // are requested at the head of phase p; hipcc then spreads them over the second half of phase p's MFMAs instead
        // of issuing each read two MFMAs before its use): -1...6 % on the 16^2...128^2 maps, neutral on 256^2.  The
        // thin-head form (one cout tile, four pixel tiles per wave) is faster with the reads at the head of each tap.
        constexpr bool APIPE = !THIN;
        frag_t a[2][NI];
        if (APIPE) {
#pragma unroll
            for (int i = 0; i < NI; ++i) a[0][i] = *reinterpret_cast<const frag_t*>(lbase[i]);
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            constexpr int dummy = 0; (void)dummy;
            const int toff = ((tap / 3) * HW2 + (tap % 3)) * RS;        // compile-time after unrolling
            if (!APIPE) {
#pragma unroll
                for (int i = 0; i < NI; ++i) a[0][i] = *reinterpret_cast<const frag_t*>(lbase[i] + toff);
#pragma unroll
                for (int i = 0; i < NI; ++i) a[1][i] = *reinterpret_cast<const frag_t*>(lbase[i] + toff + 32);
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (APIPE) {
                    if (ks == 0) {
#pragma unroll
                        for (int i = 0; i < NI; ++i) a[1][i] = *reinterpret_cast<const frag_t*>(lbase[i] + toff + 32);
                    } else if (tap < 8) {
                        const int toff1 = (((tap + 1) / 3) * HW2 + ((tap + 1) % 3)) * RS;
#pragma unroll
                        for (int i = 0; i < NI; ++i) a[0][i] = *reinterpret_cast<const frag_t*>(lbase[i] + toff1);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x100, NI, 0);      // the phase-ahead ds_reads first
                }
                if (tap == 0 && ks == 0 && c == 0) {             // first MFMA of a tile starts from C = 0: no
                    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll                                                   // accumulator clears in the epilogue
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[j][ks], a[ks][i], zero, 0, 0, 0);
                } else {
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[j][ks], a[ks][i], acc[i][j], 0, 0, 0);
                }
                // rolling prefetch of the same slot for the next tap (next unit after tap 8)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const char* src = (tap == 8) ? wnxt[j] + ks * 1024 : wcur[j] + ((tap + 1) * 2 + ks) * 1024;
                    bw[j][ks] = *reinterpret_cast<const frag_t*>(src + lane16);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (c == nch - 1) {                                        // tile finished: epilogue, accumulators reset
            const int n0 = cur.nt * COT;
            // Straight-line fast paths (no activation, unit gains, full cout tile): the epilogue runs on the same
            // SIMD as the MFMAs, so every branch / select per element is stolen from the matrix pipe.
            // The MFMA result layout gives a lane 4 consecutive couts of its pixel; lanes l and l+32 hold the two
            // halves of every 8-cout run.  One v_permlane32_swap per value pairs them up so that each lane owns 8
            // consecutive couts = ONE 16-byte store / residual load instead of two 8-byte ones (the epilogue is
            // store-issue bound).
            typedef __attribute__((ext_vector_type(4))) unsigned int u32x4e;
            auto epi_vals = [&](auto has_bias, auto has_res, int i, int j, int qp, int64_t o0, float (&v)[8]) {
                const int cw = j * 32 + 16 * qp;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned lo = __float_as_uint(acc[i][j][8 * qp + e]);
                    const unsigned hi = __float_as_uint(acc[i][j][8 * qp + 4 + e]);
                    const auto r = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
                    v[e] = __uint_as_float(r[0]); v[4 + e] = __uint_as_float(r[1]);
                }
                if constexpr (decltype(has_bias)::value) {
                    const float* bp = bias + n0 + wn * 64 + 8 * kg + cw;
                    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[e] += b0[e]; v[4 + e] += b1[e]; }
                }
                if constexpr (decltype(has_res)::value) {
                    if constexpr (sizeof(TO) == 2) {
                        const u32x4e r = *reinterpret_cast<const u32x4e*>(res + o0 + cw);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[2 * e] += __uint_as_float(r[e] << 16);
                            v[2 * e + 1] += __uint_as_float(r[e] & 0xffff0000u);
                        }
                    } else {
                        float v0[4] = {v[0], v[1], v[2], v[3]}, v1[4] = {v[4], v[5], v[6], v[7]};
                        add4(res + o0 + cw, v0); add4(res + o0 + cw + 4, v1);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v[e] = v0[e]; v[4 + e] = v1[e]; }
                    }
                }
            };
            auto epi_store = [&](TO* dst, const float (&v)[8]) {
                if constexpr (sizeof(TO) == 2) {
                    const u32x4e o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                      pack_bf16x2(v[6], v[7])};
                    *reinterpret_cast<u32x4e*>(dst) = o;
                } else {
                    const float v0[4] = {v[0], v[1], v[2], v[3]}, v1[4] = {v[4], v[5], v[6], v[7]};
                    store4(dst, v0); store4(dst + 4, v1);
                }
            };
            auto epi_plain = [&](auto has_bias, auto has_res) {
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    int ty, tx;
                    pix_of(i, ty, tx);
                    const int64_t pix = ((int64_t)cur.img * g.h + cur.py0 + ty) * g.w + cur.px0 + tx;
                    const int64_t o0 = pix * g.cout + n0 + wn * 64 + 8 * kg;
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int qp = 0; qp < 2; ++qp) {
                            float v[8];
                            epi_vals(has_bias, has_res, i, j, qp, o0, v);
                            epi_store(y + o0 + j * 32 + 16 * qp, v);
                        }
                }
            };
            // 2x2 pooled output (avg-pool of a ResBlock output, autoencoder.py:89-91, or the sum-pool that is the
            // backward of the nearest x2 upsample, :104-106): vertical partner = the next MFMA row tile (8x32 patches)
            // or lane ^ 16 (16x16 patches), horizontal partner = lane ^ 1; even lanes store at half resolution.
            auto epi_pool = [&](auto has_bias, auto has_res) {
                const int hh = g.h >> 1, wh = g.w >> 1;
#pragma unroll
                for (int i = 0; i < NI; i += (TWLOG == 5 ? 2 : 1)) {
                    int ty, tx;
                    pix_of(i, ty, tx);
                    const int64_t pix = ((int64_t)cur.img * g.h + cur.py0 + ty) * g.w + cur.px0 + tx;
                    const int64_t o0 = pix * g.cout + n0 + wn * 64 + 8 * kg;
                    const int64_t ppix = ((int64_t)cur.img * hh + ((cur.py0 + ty) >> 1)) * wh + ((cur.px0 + tx) >> 1);
                    const bool writer = TWLOG == 5 ? (p & 1) == 0 : (p & 17) == 0;
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int qp = 0; qp < 2; ++qp) {
                            float v[8];
                            epi_vals(has_bias, has_res, i, j, qp, o0, v);
                            if (TWLOG == 5) {
                                float v2[8];
                                epi_vals(has_bias, has_res, i + 1, j, qp, o0 + (int64_t)g.w * g.cout, v2);
#pragma unroll
                                for (int e = 0; e < 8; ++e) v[e] += v2[e];
                            } else {
#pragma unroll
                                for (int e = 0; e < 8; ++e) v[e] += __shfl_xor(v[e], 16, 64);
                            }
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] = (v[e] + __shfl_xor(v[e], 1, 64)) * g.pool_scale;
                            if (writer) epi_store(y + ppix * g.cout + n0 + wn * 64 + 8 * kg + j * 32 + 16 * qp, v);
                        }
                }
            };
            typedef std::integral_constant<bool, true> yes_t;
            typedef std::integral_constant<bool, false> no_t;
            const bool plain = !THIN && act == 0 && g.acc_scale == 1.0f && g.out_gain == 1.0f && (g.cout & 127) == 0;
            if (plain && g.pool) {
                if (!bias && !res) epi_pool(no_t{}, no_t{});
                else if (!bias) epi_pool(no_t{}, yes_t{});
                else if (!res) epi_pool(yes_t{}, no_t{});
                else epi_pool(yes_t{}, yes_t{});
            } else if (plain && !bias && !res) epi_plain(no_t{}, no_t{});
            else if (plain && !bias) epi_plain(no_t{}, yes_t{});
            else if (plain && !res) epi_plain(yes_t{}, no_t{});
            else if (plain) epi_plain(yes_t{}, yes_t{});
            else {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                int ty, tx;
                pix_of(i, ty, tx);
                const int64_t pix = ((int64_t)cur.img * g.h + cur.py0 + ty) * g.w + cur.px0 + tx;
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) {
                        const int co = n0 + wn * 64 + j * 32 + 8 * rq + 4 * kg;
                        if (co < g.cout) {
                            const int64_t o = pix * g.cout + co;
                            float v[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                v[e] = epi_act(acc[i][j][4 * rq + e] * g.acc_scale + (bias ? bias[co + e] : 0.0f), act) * g.out_gain;
                            if (res) add4(res + o, v);
                            store4(y + o, v);
                        }
                    }
            }
            }
        }
        if (has_next) store_halo(smem + ((u + 1) & 1) * BUF);
        __syncthreads();
        cur = nxt; tj = ntj; c = nc;
#pragma unroll
        for (int j = 0; j < NJ; ++j) wcur[j] = wnxt[j];
    }
}

// ------------------------------------------------------------------------------------------------
// 3x3 conv with ONE 16-byte chunk of input channels (the 3-channel image padded to 8 bf16: the encoder's first conv,
// autoencoder.py:114, and the dgrad of the decoder's last conv, :170).  HBM-write-bound: 16 B read, 2*Cout B written
// per pixel.  A wave owns 32 consecutive pixels of an image row x (up to) 128 couts: K = 9 taps x 8 channels = 72
// (padded to 80 = five 32x32x16 MFMAs per 32-cout tile), the im2col operand of k-step s is ONE 16-byte global load
// per lane (tap 2s + lane/32; neighbours hit L1/L2), the weights live in registers for the whole kernel, and the
// output tile is transposed through LDS so that every store instruction writes 1 KiB of consecutive bytes.
// ------------------------------------------------------------------------------------------------
// STATS (round 4: the encoder's first conv, autoencoder.py:132 -> the first ResBlock's GroupNorm): the GroupNorm sums of the stored
// output ride in the store loop (g.gn_ws, 4 channels per group, Cout = NJ*32).  A wave then owns tiles of ONE image (waves_per_image
// waves sweep an image together) and adds its sums once, at the end: 64 fp64 atomics per wave.
template <int NJ, bool STATS = false>
__global__ __launch_bounds__(256, 2) void conv3x3_thin_in_kernel(const bf16_raw* __restrict__ x,
                                                                 const bf16_raw* __restrict__ wgt,
                                                                 const float* __restrict__ bias,
                                                                 bf16_raw* __restrict__ y, ConvGeom g, int act,
                                                                 int cout_base) {
    constexpr int RS = NJ * 64 + 8;                              // LDS row stride in bytes (payload NJ*32 couts * 2 B)
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* lds = smem + wave * (32 * RS);
    const int p = lane & 31, kg = lane >> 5;

    // weights: fragment (j, s) = w[cout_base + j*32 + p][tap 2s+kg][0..7]; tap 9 does not exist -> zero
    bf16x8_t wf[NJ][5];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int s5 = 0; s5 < 5; ++s5) {
            const int tap = 2 * s5 + kg, co = cout_base + j * 32 + p;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (tap < 9 && co < g.cout) v = *reinterpret_cast<const u32x4*>(wgt + ((int64_t)co * 9 + tap) * 8);
            wf[j][s5] = __builtin_bit_cast(bf16x8_t, v);
        }
    const int xb = g.w >> 5;                                     // 32-pixel segments per row
    const int total = g.n * g.h * xb;
    const int nw = (int)gridDim.x * 4;
    const bool plain = act == 0 && g.acc_scale == 1.0f && g.out_gain == 1.0f && !bias;
    auto load_a = [&](int t, bf16x8_t (&a)[5]) {
        const int xs = t % xb;
        const int row = t / xb;                                   // n * h + y
        const int yy = row % g.h;
        const int px = xs * 32 + p;
        const bf16_raw* xrow = x + ((int64_t)row * g.w + px) * 8;
#pragma unroll
        for (int s5 = 0; s5 < 5; ++s5) {
            const int tap = 2 * s5 + kg;
            const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
            const bool ok = tap < 9 && (unsigned)(yy + dy) < (unsigned)g.h && (unsigned)(px + dx) < (unsigned)g.w;
            // unconditional load at a valid address + select (an `if (ok) load` is an exec-masked block with its own wait:
            // the five loads of a tile would return one after the other)
            const u32x4 ld = *reinterpret_cast<const u32x4*>(ok ? xrow + ((int64_t)dy * g.w + dx) * 8 : xrow);
            const u32x4 zero4 = {0u, 0u, 0u, 0u};
            a[s5] = __builtin_bit_cast(bf16x8_t, ok ? ld : zero4);
        }
    };
    int t = (int)blockIdx.x * 4 + wave, t_step = nw, t_end = total, img_s = 0;
    if constexpr (STATS) {                                       // (the launcher made nw a multiple of n and of the tiles of an image)
        const int wpi = nw / g.n, tpi = g.h * xb;
        img_s = t / wpi;
        t = img_s * tpi + (t - img_s * wpi); t_step = wpi; t_end = (img_s + 1) * tpi;
    }
    float sga = 0.f, sqa = 0.f, sgb = 0.f, sqb = 0.f;            // STATS: sum / sum of squares of channels 0-3 / 4-7 of this lane's slot
    float* bl = reinterpret_cast<float*>(smem + 4 * 32 * RS);     // the block's NJ*32 biases (read as float4 in the epilogue)
    if (tid < NJ * 32) bl[tid] = (bias && cout_base + tid < g.cout) ? bias[cout_base + tid] : 0.0f;
    __syncthreads();
    if (t >= t_end) return;
    bf16x8_t a[5], an[5];
    load_a(t, a);
    for (; t < t_end; t += t_step) {
        const int xs = t % xb;
        const int row = t / xb;
        const int tn = t + t_step < t_end ? t + t_step : t;      // next tile's operand in flight during this one
        load_a(tn, an);
        f32x16 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j][0], a[0], zero, 0, 0, 0);
#pragma unroll
            for (int s5 = 1; s5 < 5; ++s5) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j][s5], a[s5], acc[j], 0, 0, 0);
        }
        // epilogue -> LDS (row = pixel, 4-cout pieces); the activation is a compile-time constant of each body (a
        // run-time switch per element serialised the epilogue: 183-238 us against 65 us for the plain one)
        auto stage = [&](auto A) {
            constexpr int AC = decltype(A)::value;               // -1: plain
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v[4];
                    f32x4 bq = {0.f, 0.f, 0.f, 0.f};
                    if (AC >= 0) bq = *reinterpret_cast<const f32x4*>(bl + j * 32 + 8 * q + 4 * kg);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[e] = acc[j][4 * q + e];
                        if (AC >= 0) v[e] = epi_act(v[e] * g.acc_scale + bq[e], AC) * g.out_gain;
                    }
                    const u32x2 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
                    *reinterpret_cast<u32x2*>(lds + p * RS + (j * 32 + 8 * q + 4 * kg) * 2) = o;
                }
        };
        if (plain) stage(std::integral_constant<int, -1>{});
        else if (act == 3) stage(std::integral_constant<int, 3>{});
        else if (act == 0) stage(std::integral_constant<int, 0>{});
        else if (act == 1) stage(std::integral_constant<int, 1>{});
        else stage(std::integral_constant<int, 2>{});
        // LDS -> global: the wave's 32 pixels x NJ*64 B are consecutive rows of y
        const int cout_blk = NJ * 32;
        char* ybase = reinterpret_cast<char*>(y + ((int64_t)row * g.w + xs * 32) * g.cout + cout_base);
        if (g.cout == cout_blk) {                                // rows are back to back: 1 KiB per store instruction
#pragma unroll
            for (int it = 0; it < NJ * 2; ++it) {
                const int o = it * 1024 + lane * 16;
                const int pr = o / (NJ * 64), pb = o - pr * (NJ * 64);
                const u32x4 v = *reinterpret_cast<const u32x4*>(lds + pr * RS + pb);
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(ybase + o));   // whole lines, written once: 146 -> 105 us
                if constexpr (STATS) {
                    // the lane's slot (lane & 15: 8 channels = two groups) is the same in every iteration; packed-pair dot
                    // products against (1, 1) / against itself, as in the role-split kernel's drain (conv_mx.hip)
                    const unsigned ones2 = 0x3f803f80u;
                    const unsigned d0 = v[0], d1 = v[1], d2 = v[2], d3 = v[3];
                    asm("v_dot2c_f32_bf16 %0, %4, %8\n\tv_dot2c_f32_bf16 %1, %4, %4\n\tv_dot2c_f32_bf16 %2, %6, %8\n\t"
                        "v_dot2c_f32_bf16 %3, %6, %6\n\tv_dot2c_f32_bf16 %0, %5, %8\n\tv_dot2c_f32_bf16 %1, %5, %5\n\t"
                        "v_dot2c_f32_bf16 %2, %7, %8\n\tv_dot2c_f32_bf16 %3, %7, %7\n\ts_nop 0"
                        : "+v"(sga), "+v"(sqa), "+v"(sgb), "+v"(sqb) : "v"(d0), "v"(d1), "v"(d2), "v"(d3), "v"(ones2));
                }
            }
        } else {
#pragma unroll
            for (int it = 0; it < NJ * 2; ++it) {
                const int o = it * 1024 + lane * 16;
                const int pr = o / (NJ * 64), pb = o - pr * (NJ * 64);
                if (cout_base + pb / 2 < g.cout) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(lds + pr * RS + pb);
                    *reinterpret_cast<u32x4*>(ybase + (int64_t)pr * g.cout * 2 + pb) = v;
                }
            }
        }
#pragma unroll
        for (int s5 = 0; s5 < 5; ++s5) a[s5] = an[s5];
    }
    if constexpr (STATS) {
        asm volatile("s_nop 3" : "+v"(sga), "+v"(sqa), "+v"(sgb), "+v"(sqb));       // (the dot chain is closed before the sums are read)
        sga += __shfl_xor(sga, 16, 64); sga += __shfl_xor(sga, 32, 64);
        sqa += __shfl_xor(sqa, 16, 64); sqa += __shfl_xor(sqa, 32, 64);
        sgb += __shfl_xor(sgb, 16, 64); sgb += __shfl_xor(sgb, 32, 64);
        sqb += __shfl_xor(sqb, 16, 64); sqb += __shfl_xor(sqb, 32, 64);
        if (lane < 16) {
            const int groups = g.cout >> 2;
            double* dst = g.gn_ws + ((int64_t)img_s * groups + ((cout_base >> 2) + 2 * lane)) * 2;
            atomicAdd(dst, (double)sga); atomicAdd(dst + 1, (double)sqa);
            atomicAdd(dst + 2, (double)sgb); atomicAdd(dst + 3, (double)sqb);
        }
    }
}

static thread_local int g_force_variant = CONV_VARIANT_AUTO;   // test hook (conv_geom.h: ConvVariant), per host thread: the library
                                                               // keeps no process-global mutable state
// deterministic mode (vqk_set_deterministic; the reference trains with deterministic=True, vqvae/train.py:130): split-K partials
// go through this workspace and are summed in a fixed order, kernels without a workspace form run unsplit
#define g_det (vqkd::det_state().on)
#define g_det_ws (vqkd::det_state().ws)
#define g_det_ws_bytes (vqkd::det_state().bytes)
static thread_local int g_stream_blocks = 0;    // persistent-grid caps (0 = default 2 blocks per CU): 256 leaves half of every CU to a
static thread_local int g_wgrad_blocks = 0;     // kernel running concurrently on another stream (dgrad || wgrad || GroupNorm)

// shapes of the matrix/auxiliary-wave kernel (conv_mx.hip): bf16, whole 128-cout tiles, at least two 32-channel chunks, 32-bit
// buffer offsets
inline bool mx_shape_ok(const ConvGeom& g, int variant) {
    return VQK_TUNE("MX", 1) && variant != CONV_VARIANT_NO_MX && (g.cout & 127) == 0 && (g.cpt >> 2) >= 2 &&
           (int64_t)g.n * g.h_in * g.w_in * g.cin * 2 < 0x7fffffffLL && (int64_t)g.m * g.cout * 2 < 0x7fffffffLL;
}

// its 2x2-tap phase forms (g.ntap = 4, g.phase_mode set) on units of 64 input channels instead of 32 (conv_mx.hip: U64): whole
// 64-channel units, at least two units per tile (a tile is drained beside the NEXT tile's first unit and parked at the end of
// its last: phase_mode 2 has four phases x units, the others need 128 channels), and the patch shape's LDS must fit.  Tuning
// slot MX_PHASE_U64 = 0 forces the 32-channel form (A/B, and the bit-equality tests)
inline bool mx_phase_u64_serves(const ConvGeom& g, int tw) {
    const int units = (g.cin / 64) * (g.phase_mode == 2 ? 4 : 1);
    return VQK_TUNE("MX_PHASE_U64", 1) && g.ntap == 4 && (g.cin % 64) == 0 && units >= 2 && (tw == 4 || tw == 5) &&
           vqkd::mx_phase_u64_lds(tw) <= vqkd::MX_LDS_MAX;
}

// 1x1 convs (the ResBlock shortcuts, autoencoder.py:52-55): the NTAP = 1 form of that kernel
inline bool mx_serves_1x1(const ConvGeom& g, int variant) {
    return mx_shape_ok(g, variant) && VQK_TUNE("MX_1X1", 1) && !g.ups;
}

// 0: not eligible for the halo kernels; 5 / 4: patch width log2 (8x32 / 16x16 pixel patches)
inline int halo_twlog(const ConvGeom& g, int variant) {
    if ((g.ks != 3 && g.ks != 1) || (g.cpt % 8) != 0 || variant == CONV_VARIANT_IM2COL) return 0;
    if (g.ks == 1 && !mx_serves_1x1(g, variant)) return 0;       // 1x1: only the matrix/auxiliary-wave kernel has a pixel-tile form
    const int prefer16 = VQK_TUNE("TW16", 0);      // A/B: 16x16 patches where both fit
    if (prefer16 && (g.w % 16) == 0 && (g.h % 16) == 0) return 4;
    if ((g.w % 32) == 0 && (g.h % 8) == 0) return 5;
    if ((g.w % 16) == 0 && (g.h % 16) == 0) return 4;
    return 0;
}

// the fused epilogues (2x2 pooling, GroupNorm sums of the output: vqk_conv2d_fprop_pooled / _gnstats) exist on the fragment-major
// bf16 kernels with whole 128-cout tiles
inline bool fused_epilogue_serves(const ConvGeom& g, int variant) {
    return halo_twlog(g, variant) && (g.cout % 128) == 0 && variant != CONV_VARIANT_BREG && variant != CONV_VARIANT_PLAIN_WEIGHTS;
}

// the edge convs in the fp32 modes (conv_thin_f32.hip): 4 channels on one side -- fp32 FMAs at memory speed instead of 7/8 padding
// on the matrix pipe.  Plain 3x3 convs on plain weights
inline bool thin_f32_plain(const ConvGeom& g, int variant) {
    return g.ks == 3 && !g.ups && !g.zs && !g.sub && g.stride == 1 && g.pad == 1 && g.vh == g.h && g.vw == g.w &&
           variant != CONV_VARIANT_IM2COL;
}
inline bool thin_out_f32_serves(const ConvGeom& g, int variant) {
    return thin_f32_plain(g, variant) && g.cout == 4 && (g.cin % 16) == 0 && (g.h % 8) == 0 && (g.w % 32) == 0;
}
inline bool thin_in_f32_serves(const ConvGeom& g, int variant, bool has_res, int act) {
    return thin_f32_plain(g, variant) && g.cin == 4 && (g.cout == 64 || g.cout == 128 || g.cout == 256) && !has_res && act == 0 &&
           g.acc_scale == 1.0f && g.out_gain == 1.0f && g.w >= 4 && (g.w % 4) == 0 && (int64_t)(10) * (g.w + 2) * 16 <= 64 * 1024;
}

// ---- the forward / data-gradient dispatch: plan_fprop decides and launches nothing, launch_fprop launches what it decided ----
// The kernel forms.  The ids are part of the C-ABI (vqk_conv_fprop_plan returns them): append, never renumber.
enum ConvForm : int {
    FORM_THIN_OUT_F32 = 0,   // conv_thin_f32.hip: fp32, 4 output channels
    FORM_THIN_IN_F32,        // conv_thin_f32.hip: fp32, 4 input channels
    FORM_MX,                 // conv_mx.hip: matrix/auxiliary-wave kernel, 3x3
    FORM_MX_1X1,             // ... its one-tap form (memory-bound)
    FORM_STREAM_THIN,        // stream kernel, cout <= 32: one 32-wide cout tile, the waves split the pixels
    FORM_STREAM_HALF,        // stream kernel, 128-pixel tiles (fewer 256-pixel tiles than CUs)
    FORM_STREAM_FULL,        // stream kernel, 256-pixel tiles
    FORM_HALO_BREG,          // register-weight halo kernel (fragment-major weights)
    FORM_HALO_LDS,           // LDS-weight halo kernel (plain weights)
    FORM_THIN_IN_BF16,       // bf16, one 16-byte chunk of input channels: one launch per 128 output channels (memory-bound)
    FORM_IM2COL,             // the general kernel
    FORM_IM2COL_SPLITK,      // ... with K split through the caller's scratch, then the epilogue kernel
    FORM_X3,                 // conv_x3.hip: split-product kernel (layout 5; chosen by the caller, launched by conv_general)
    FORM_X3_1X1,             // ... its one-tap form (memory-bound)
    FORM_COUNT
};

struct FpropPlan {
    int status;     // VQK_OK, or what the launcher returns instead of launching
    int form;       // ConvForm
    int tw;         // patch width log2 of the halo forms (5 / 4), else 0
    int blocks;     // grid of the (first) launch; 0 where the form's own launcher sizes it (conv_mx / conv_x3 / conv_thin_f32.hip)
    int splits;     // split-K parts (1: unsplit) ...
    int sps;        // ... and k-steps per part
    int launches;
};

// g carries the pooled epilogue / fused GroupNorm sums (g.pool, g.gn_ws) and the general-conv fields; `variant`: the calling
// thread's hook, or CONV_VARIANT_IM2COL from a caller that needs the general kernel.  Reads the block caps, the tuning slots and
// the thread's scratch; touches no device.
FpropPlan plan_fprop(const ConvGeom& g, int dtype, int out_dtype, int act, int wlayout, bool has_res, int variant) {
    FpropPlan p = {VQK_OK, FORM_IM2COL, 0, 0, 1, 0, 1};
    auto refuse = [&](int status) { p.status = status; return p; };
    auto take = [&](int form, int64_t blocks) { p.form = form; p.blocks = (int)blocks; return p; };
    const bool bf_in = dtype == VQK_BF16, bf_out = out_dtype == VQK_BF16;
    if (!bf_in && !bf_out && wlayout == 0) {
        if (thin_out_f32_serves(g, variant)) return take(FORM_THIN_OUT_F32, 0);
        if (thin_in_f32_serves(g, variant, has_res, act)) return take(FORM_THIN_IN_F32, 0);
    }
    const int tw = p.tw = halo_twlog(g, variant);
    const int tiles = tw ? g.n * (g.h / (256 >> tw)) * (g.w >> tw) * g.tiles_n : 0;      // 256-pixel patches x cout tiles
    if (wlayout == 1 && bf_in && variant != CONV_VARIANT_BREG) {
        if (!tw) return refuse(VQK_ERR_SHAPE);
        // matrix-wave / auxiliary-wave kernel (conv_mx.hip): whole 128-cout tiles, plain epilogue (bias / residual / pooling;
        // relu or leaky relu with the StyleGAN2 gains: the VGG and discriminator convs).  The choice must not depend on the
        // batch size (a step on B images has to equal the mean of the steps on its halves to bf16 noise -- the two kernels
        // round differently), hence no tile-count threshold by default
        const bool plain = act == 0 || ((act == 2 || act == 3) && !g.pool && !g.gn_ws);
        if (bf_out && plain && mx_shape_ok(g, variant) &&
            (tiles >= VQK_TUNE("MX_MIN_TILES", 1) || variant == CONV_VARIANT_MX || g.ks == 1)) {
            if (g.ks == 1 && g.pool) return refuse(VQK_ERR_ARG);    // (the one-tap form has no pooled drain)
            return take(g.ks == 1 ? FORM_MX_1X1 : FORM_MX, 0);
        }
        if (g.gn_ws || g.ks == 1) return refuse(VQK_ERR_SHAPE);     // fused statistics / 1x1 tiles exist on the matrix/auxiliary-wave kernel only
        const int persist = g_stream_blocks > 0 ? g_stream_blocks : VQK_TUNE("STREAM_BLOCKS", 512);
        const bool half_ok = tw == 5 ? (g.h % 4) == 0 : (g.h % 8) == 0;
        if (g.cout <= 32) return take(FORM_STREAM_THIN, tiles < persist ? tiles : persist);
        if (tiles < 256 && half_ok && !g.pool && bf_out && variant != CONV_VARIANT_NO_HALF)
            return take(FORM_STREAM_HALF, 2 * tiles < persist ? 2 * tiles : persist);
        return take(FORM_STREAM_FULL, tiles < persist ? tiles : persist);
    }
    if (wlayout == 1) {
        if (!tw || g.ks == 1) return refuse(VQK_ERR_SHAPE);         // fragment-major weights need a halo-eligible shape
        return take(FORM_HALO_BREG, tiles);
    }
    if (tw && g.ks == 3) return take(FORM_HALO_LDS, tiles);
    p.tw = 0;
    if (bf_in && bf_out && wlayout == 0 && g.ks == 3 && g.cpt == 1 && !has_res && !g.ups && !g.zs && g.stride == 1 && g.pad == 1 &&
        (g.w % 32) == 0 && (g.cout % 8) == 0 && g.vh == g.h && g.vw == g.w && variant != CONV_VARIANT_IM2COL) {
        const int waves = g.n * g.h * (g.w >> 5);
        p.launches = (g.cout + 127) / 128;
        return take(FORM_THIN_IN_BF16, (waves + 3) / 4 > 1024 ? 1024 : (waves + 3) / 4);
    }
    // split-K through the caller's scratch (vqk_set_scratch) when the tile grid leaves most of the chip idle
    // (this kernel runs one k-step at a time per block: below ~4 blocks per CU nothing hides its load -> LDS -> MFMA latency)
    const vqkd::DetState& sc = vqkd::scratch_state();
    const int grid = g.tiles_m * g.tiles_n, ksteps = (g.kchunks + 7) >> 3;
    const int64_t out_elems = (int64_t)g.m * g.cout;
    const int sk_blocks = VQK_TUNE("SK_BLOCKS", 2048), sk_minsteps = VQK_TUNE("SK_MINSTEPS", 4), sk_maxmb = VQK_TUNE("SK_MAXMB", 32);
    int splits = grid * 2 <= sk_blocks ? sk_blocks / grid : 1;
    if (splits > ksteps / sk_minsteps) splits = ksteps / sk_minsteps;
    if ((int64_t)splits * out_elems * 4 > ((int64_t)sk_maxmb << 20)) splits = (int)(((int64_t)sk_maxmb << 20) / (out_elems * 4));
    if (sc.ws && (int64_t)splits * out_elems * 4 > sc.bytes) splits = (int)(sc.bytes / (out_elems * 4));
    if (VQK_TUNE("FPROP_SPLITK", 1) && sc.ws && (g.cout & 3) == 0 && splits >= 2) {
        p.sps = (ksteps + splits - 1) / splits;
        p.splits = (ksteps + p.sps - 1) / p.sps;
        p.launches = 2;
        return take(FORM_IM2COL_SPLITK, grid);
    }
    return take(FORM_IM2COL, grid);
}

// one helper per kernel template: the plan's patch width (or the whole-chunk flag of the im2col kernel) picks the instantiation
template <typename TO, int MODE>
void launch_stream(const FpropPlan& p, hipStream_t st, const void* x, const void* w, const float* bias, const void* res, void* y,
                   const void* zeros, const ConvGeom& g, int act) {
    auto kernel = p.tw == 5 ? conv3x3_stream_kernel<TO, 5, MODE> : conv3x3_stream_kernel<TO, 4, MODE>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.blocks), dim3(256), 2 * 28 * 1024, st, (const bf16_raw*)x, (const bf16_raw*)w, bias,
                       (const TO*)res, (TO*)y, (const char*)zeros, g, act);
}

template <typename T, typename TO>
void launch_halo_breg(const FpropPlan& p, hipStream_t st, const void* x, const void* w, const float* bias, const void* res, void* y,
                      const void* zeros, const ConvGeom& g, int act) {
    auto kernel = p.tw == 5 ? conv3x3_halo_breg_kernel<T, TO, 5> : conv3x3_halo_breg_kernel<T, TO, 4>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.blocks), dim3(256), 11 * 4096, st, (const T*)x, (const T*)w, bias, (const TO*)res,
                       (TO*)y, (const char*)zeros, g, act);
}

template <typename T, typename TO, int TW>
void launch_halo_lds(const FpropPlan& p, hipStream_t st, const void* x, const void* w, const float* bias, const void* res, void* y,
                     const void* zeros, const ConvGeom& g, int act) {
    constexpr int lds = 11 * 4096 + 32768;
    static const hipError_t attr = hipFuncSetAttribute((const void*)conv3x3_halo_kernel<T, TO, TW>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)attr;
    hipLaunchKernelGGL((conv3x3_halo_kernel<T, TO, TW>), dim3((unsigned)p.blocks), dim3(256), lds, st, (const T*)x, (const T*)w, bias,
                       (const TO*)res, (TO*)y, (const char*)zeros, g, act);
}

template <typename T, typename TO>
void launch_im2col(const FpropPlan& p, hipStream_t st, const void* x, const void* w, const float* bias, const void* res, void* y,
                   const void* zeros, const ConvGeom& g, int act, float* skws) {
    auto kernel = (g.cpt % 8) == 0 ? conv_fprop_kernel<T, TO, true> : conv_fprop_kernel<T, TO, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.blocks, (unsigned)p.splits), dim3(256), 32768, st, (const T*)x, (const T*)w, bias,
                       (const TO*)res, (TO*)y, (const char*)zeros, g, act, skws, p.sps);
}

template <typename T, typename TO>
int launch_fprop(const void* x, const void* w, const float* bias, const void* res, void* y, const void* zeros,
                 const ConvGeom& g, int act, int wlayout, int variant, hipStream_t st) {
    const FpropPlan p = plan_fprop(g, sizeof(T) == 2 ? VQK_BF16 : VQK_F32, sizeof(TO) == 2 ? VQK_BF16 : VQK_F32, act, wlayout,
                                   res != nullptr, variant);
    if (p.status != VQK_OK) return p.status;
    switch (p.form) {
    case FORM_THIN_OUT_F32:
        return vqkd::launch_conv3x3_thin_out_f32((const float*)x, (const float*)w, bias, (const float*)res, (float*)y, g.n, g.h, g.w,
                                                 g.cin, act, g.acc_scale, g.out_gain, st);
    case FORM_THIN_IN_F32:
        return vqkd::launch_conv3x3_thin_in_f32((const float*)x, (const float*)w, bias, (float*)y, g.n, g.h, g.w, g.cout, st);
    case FORM_MX:
    case FORM_MX_1X1: {
        ConvGeom ga = g;
        ga.act = act;
        return vqkd::launch_conv3x3_mx(x, w, bias, res, y, zeros, ga, p.tw, st);
    }
    case FORM_STREAM_THIN: {
        ConvGeom gt = g;
        gt.tiles_n = 1;
        launch_stream<TO, 1>(p, st, x, w, bias, res, y, zeros, gt, act);
        break;
    }
    case FORM_STREAM_HALF: launch_stream<TO, 2>(p, st, x, w, bias, res, y, zeros, g, act); break;
    case FORM_STREAM_FULL: launch_stream<TO, 0>(p, st, x, w, bias, res, y, zeros, g, act); break;
    case FORM_HALO_BREG: launch_halo_breg<T, TO>(p, st, x, w, bias, res, y, zeros, g, act); break;
    case FORM_HALO_LDS:
        if (p.tw == 5) launch_halo_lds<T, TO, 5>(p, st, x, w, bias, res, y, zeros, g, act);
        else launch_halo_lds<T, TO, 4>(p, st, x, w, bias, res, y, zeros, g, act);
        break;
    case FORM_THIN_IN_BF16:
        for (int cb = 0; cb < g.cout; cb += 128) {
            if (g.cout - cb > 64)
                hipLaunchKernelGGL((conv3x3_thin_in_kernel<4>), dim3((unsigned)p.blocks), dim3(256), 4 * 32 * (4 * 64 + 8) + 4 * 128, st,
                                   (const bf16_raw*)x, (const bf16_raw*)w, bias, (bf16_raw*)y, g, act, cb);
            else
                hipLaunchKernelGGL((conv3x3_thin_in_kernel<2>), dim3((unsigned)p.blocks), dim3(256), 4 * 32 * (2 * 64 + 8) + 4 * 64, st,
                                   (const bf16_raw*)x, (const bf16_raw*)w, bias, (bf16_raw*)y, g, act, cb);
        }
        break;
    case FORM_IM2COL: launch_im2col<T, TO>(p, st, x, w, bias, res, y, zeros, g, act, nullptr); break;
    case FORM_IM2COL_SPLITK: {
        float* skws = vqkd::scratch_state().ws;
        launch_im2col<T, TO>(p, st, x, w, bias, res, y, zeros, g, act, skws);
        hipLaunchKernelGGL(conv_splitk_epilogue_kernel<TO>, dim3((unsigned)(((int64_t)g.m * g.cout / 4 + 255) / 256)), dim3(256), 0, st,
                           skws, bias, (const TO*)res, (TO*)y, g, act, p.splits);
        break;
    }
    default: return VQK_ERR_ARG;
    }
    if (hipGetLastError() != hipSuccess) return VQK_ERR_LAUNCH;
    return VQK_OK;
}

// the (dtype, out_dtype) pairs the kernels exist for
int launch_fprop_any(int dtype, int out_dtype, const void* x, const void* w, const float* bias, const void* res, void* y,
                     const void* zeros, const ConvGeom& g, int act, int wlayout, int variant, hipStream_t st) {
    if (dtype == VQK_F32 && out_dtype == VQK_F32) return launch_fprop<float, float>(x, w, bias, res, y, zeros, g, act, wlayout, variant, st);
    if (dtype == VQK_BF16 && out_dtype == VQK_BF16) return launch_fprop<bf16_raw, bf16_raw>(x, w, bias, res, y, zeros, g, act, wlayout, variant, st);
    if (dtype == VQK_BF16 && out_dtype == VQK_F32) return launch_fprop<bf16_raw, float>(x, w, bias, res, y, zeros, g, act, wlayout, variant, st);
    return VQK_ERR_DTYPE;
}

int make_geom(ConvGeom& g, int dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int ups) {
    if (dtype != VQK_F32 && dtype != VQK_BF16) return VQK_ERR_DTYPE;
    const int epc = dtype == VQK_F32 ? 4 : 8;
    if (n <= 0 || h_in <= 0 || w_in <= 0 || cin <= 0 || cout <= 0) return VQK_ERR_SHAPE;
    if (ksize != 1 && ksize != 3) return VQK_ERR_SHAPE;
    if (ups != 0 && ups != 1) return VQK_ERR_ARG;
    if (cin % epc) return VQK_ERR_SHAPE;
    g.n = n; g.h_in = h_in; g.w_in = w_in; g.h = h_in << ups; g.w = w_in << ups;
    g.cin = cin; g.cout = cout; g.ks = ksize; g.ups = ups;
    g.stride = 1; g.pad = ksize >> 1; g.zs = 0; g.vh = g.h; g.vw = g.w;
    g.acc_scale = 1.0f; g.out_gain = 1.0f; g.pool = 0; g.pool_scale = 1.0f;
    g.gn_ws = nullptr; g.gn_cpg = 0; g.gn_part_nblk = 0; g.gn_part_base = 0;
    g.act = 0; g.dy_pool = 0; g.tq = nullptr; g.tq_mode = 0; g.phase_rev = 0;
    g.ntap = ksize == 1 ? 1 : 9; g.tap_oy = g.tap_ox = 0; g.src_s = 1; g.src_a = g.src_b = 0; g.dst_s = 1; g.dst_a = g.dst_b = 0;
    g.tapw = 0; g.dst_h = g.dst_w = 0; g.s2 = 0; g.phase_mode = 0; g.unit64 = 0;
    g.fold = 0;
    const int64_t m = (int64_t)n * g.h * g.w;
    if (m > 0x7fffffff - 256) return VQK_ERR_SHAPE;
    g.m = (int)m;
    g.cpt = cin / epc;
    g.kchunks = ksize * ksize * g.cpt;
    g.wrow_chunks = g.kchunks; g.sub = 0;
    g.tiles_m = (g.m + 127) / 128;
    g.tiles_n = (cout + 127) / 128;
    return VQK_OK;
}

}  // namespace

// shared with conv_wgrad.hip (the weight-gradient translation unit)
namespace vqkd {
int conv_make_geom(ConvGeom& g, int dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int ups) {
    return make_geom(g, dtype, n, h_in, w_in, cin, cout, ksize, ups);
}
int& conv_force_variant() { return g_force_variant; }
int& conv_wgrad_blocks() { return g_wgrad_blocks; }
}  // namespace vqkd

extern "C" {

/* test / tuning hook: the values are conv_geom.h's ConvVariant (documented in include/vqk.h) */
int vqk_conv_set_variant(int v) { g_force_variant = v; return VQK_OK; }
int vqk_conv_set_block_caps(int stream_blocks, int wgrad_blocks) {
    g_stream_blocks = stream_blocks; g_wgrad_blocks = wgrad_blocks;
    return VQK_OK;
}

static int conv_general(int dtype, const void* x, const void* w, const float* bias, const void* residual, void* y,
                        int out_dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int stride, int pad,
                        int mode, int h_out, int w_out, int act, float acc_scale, float out_gain, int wlayout,
                        const void* zeros, void* stream) {
    VQK_REQUIRE(x && w && y && zeros, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(w) && vqk_aligned16(zeros), VQK_ERR_ALIGN);
    VQK_REQUIRE(act >= 0 && act <= 3, VQK_ERR_ARG);
    VQK_REQUIRE(wlayout == 0 || wlayout == 1 || wlayout == 5, VQK_ERR_ARG);
    VQK_REQUIRE(mode >= 0 && mode <= 2 && (stride == 1 || stride == 2) && pad >= 0, VQK_ERR_ARG);
    ConvGeom g;
    const int rc = make_geom(g, dtype, n, h_in, w_in, cin, cout, ksize, mode ? 1 : 0);
    if (rc) return rc;
    const bool plain = stride == 1 && pad == (ksize >> 1) && mode != 2 && h_out == g.h && w_out == g.w;
    if (!plain) {
        VQK_REQUIRE(wlayout == 0, VQK_ERR_ARG);             // strided / explicitly padded convs run on the im2col kernel
        g.zs = mode == 2;
        g.vh = mode == 2 ? 2 * h_in - 1 : g.h;
        g.vw = mode == 2 ? 2 * w_in - 1 : g.w;
        g.stride = stride; g.pad = pad;
        VQK_REQUIRE(h_out > 0 && w_out > 0, VQK_ERR_SHAPE);
        VQK_REQUIRE((h_out - 1) * stride + ksize - pad <= g.vh + pad + stride, VQK_ERR_SHAPE);
        g.h = h_out; g.w = w_out;
        const int64_t m = (int64_t)n * h_out * w_out;
        VQK_REQUIRE(m < 0x7fffff00, VQK_ERR_SHAPE);
        g.m = (int)m;
        g.tiles_m = (g.m + 127) / 128;
    }
    g.acc_scale = acc_scale; g.out_gain = out_gain;
    hipStream_t st = vqk_stream(stream);
    if (wlayout == 5) {
        // split-product mode: fp32 activations, three bf16 products per multiply-add (conv_x3.hip)
        VQK_REQUIRE(plain && dtype == VQK_F32 && out_dtype == VQK_F32 && (ksize == 3 || ksize == 1), VQK_ERR_ARG);
        VQK_REQUIRE(vqk_aligned16(y) && (!residual || vqk_aligned16(residual)), VQK_ERR_ALIGN);
        return vqkd::launch_conv3x3_x3(x, w, bias, residual, y, zeros, g, act, g_stream_blocks, st);
    }
    if (mode == 2 && stride == 1 && g_force_variant != CONV_VARIANT_NO_MX) {
        // zero-stuffed input: one im2col launch per output-parity class, each visiting only the taps that hit real samples
        int r = VQK_OK;
        for (int py = 0; py < 2 && r == VQK_OK; ++py)
            for (int px = 0; px < 2 && r == VQK_OK; ++px) {
                ConvGeom gs = g;
                gs.sub = 1; gs.sub_py = py; gs.sub_px = px;
                gs.sub_h = (g.h - py + 1) / 2; gs.sub_w = (g.w - px + 1) / 2;
                if (gs.sub_h <= 0 || gs.sub_w <= 0) continue;
                gs.nkh = gs.nkw = 0;
                for (int kk = 0; kk < ksize; ++kk) {
                    if (((py + kk - pad) & 1) == 0) gs.khl[gs.nkh++] = kk;
                    if (((px + kk - pad) & 1) == 0) gs.kwl[gs.nkw++] = kk;
                }
                if (gs.nkh == 0 || gs.nkw == 0) { gs.nkh = gs.nkw = 1; gs.khl[0] = gs.kwl[0] = 0; gs.kchunks = 0; }
                else gs.kchunks = gs.nkh * gs.nkw * gs.cpt;
                gs.m = n * gs.sub_h * gs.sub_w;
                gs.tiles_m = (gs.m + 127) / 128;
                r = launch_fprop_any(dtype, out_dtype, x, w, bias, residual, y, zeros, gs, act, 0, CONV_VARIANT_IM2COL, st);
            }
        return r;
    }
    // strided / explicitly padded convs: the general im2col kernel
    return launch_fprop_any(dtype, out_dtype, x, w, bias, residual, y, zeros, g, act, wlayout,
                            plain ? g_force_variant : (int)CONV_VARIANT_IM2COL, st);
}

int vqk_conv2d_fprop(int dtype, const void* x, const void* w, const float* bias, const void* residual, void* y,
                     int out_dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int ups, int act,
                     int wlayout, const void* zeros, void* stream) {
    VQK_REQUIRE(ups == 0 || ups == 1, VQK_ERR_ARG);
    return conv_general(dtype, x, w, bias, residual, y, out_dtype, n, h_in, w_in, cin, cout, ksize, 1, ksize >> 1, ups,
                        h_in << ups, w_in << ups, act, 1.0f, 1.0f, wlayout, zeros, stream);
}

int vqk_conv2d_fprop_pooled(int dtype, const void* x, const void* w, const float* bias, const void* residual, void* y,
                            int n, int h_in, int w_in, int cin, int cout, int ksize, int ups, float pool_scale,
                            const void* zeros, void* stream) {
    VQK_REQUIRE(x && w && y && zeros, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(w) && vqk_aligned16(zeros) && vqk_aligned16(y), VQK_ERR_ALIGN);
    VQK_REQUIRE(dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(ups == 0 || ups == 1, VQK_ERR_ARG);
    ConvGeom g;
    const int rc = make_geom(g, dtype, n, h_in, w_in, cin, cout, ksize, ups);
    if (rc) return rc;
    VQK_REQUIRE(fused_epilogue_serves(g, g_force_variant), VQK_ERR_SHAPE);
    g.pool = 1; g.pool_scale = pool_scale;
    return launch_fprop<bf16_raw, bf16_raw>(x, w, bias, residual, y, zeros, g, 0, 1, g_force_variant, vqk_stream(stream));
}

int vqk_conv2d_fprop_gnstats(int dtype, const void* x, const void* w, const float* bias, const void* residual, void* y,
                             int n, int h_in, int w_in, int cin, int cout, int ksize, int ups, int pool, float pool_scale,
                             double* gn_ws, int groups, const void* zeros, void* stream) {
    VQK_REQUIRE(x && w && y && zeros && gn_ws, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(w) && vqk_aligned16(zeros) && vqk_aligned16(y), VQK_ERR_ALIGN);
    VQK_REQUIRE(dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE((ups == 0 || ups == 1) && (pool == 0 || pool == 1), VQK_ERR_ARG);
    VQK_REQUIRE(ksize == 3 && groups > 0 && cout % groups == 0 && (cout / groups) % 4 == 0, VQK_ERR_SHAPE);
    ConvGeom g;
    const int rc = make_geom(g, dtype, n, h_in, w_in, cin, cout, ksize, ups);
    if (rc) return rc;
    VQK_REQUIRE(fused_epilogue_serves(g, g_force_variant), VQK_ERR_SHAPE);
    g.pool = pool; g.pool_scale = pool ? pool_scale : 1.0f;
    g.gn_ws = gn_ws; g.gn_cpg = cout / groups;
    if (g_det) g.gn_part_nblk = (g.h * g.w) / 256;          // deterministic mode: one slot per 256-pixel tile of the image
    return launch_fprop<bf16_raw, bf16_raw>(x, w, bias, residual, y, zeros, g, 0, 1, g_force_variant, vqk_stream(stream));
}

int vqk_conv2d_fprop_x3_gnstats(const float* x, const void* w5, const float* bias, const float* residual, float* y, int n, int h_in,
                                int w_in, int cin, int cout, int ups, double* gn_ws, int groups, const void* zeros, void* stream) {
    // the split-product 3x3 conv (wlayout 5) with the GroupNorm sums of its fp32 output left in gn_ws (csrc/conv_x3.hip)
    VQK_REQUIRE(x && w5 && y && zeros && gn_ws, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(w5) && vqk_aligned16(zeros) && vqk_aligned16(y) && (!residual || vqk_aligned16(residual)),
                VQK_ERR_ALIGN);
    VQK_REQUIRE(ups == 0 || ups == 1, VQK_ERR_ARG);
    VQK_REQUIRE(groups > 0 && cout % groups == 0 && (cout % 128) == 0, VQK_ERR_SHAPE);
    const int cpg = cout / groups;
    VQK_REQUIRE((cpg == 4 || cpg == 8 || cpg == 16) && !g_det, VQK_ERR_SHAPE);     // (atomics: the deterministic mode keeps its statistics pass)
    ConvGeom g;
    const int rc = make_geom(g, VQK_F32, n, h_in, w_in, cin, cout, 3, ups);
    if (rc) return rc;
    g.gn_ws = gn_ws; g.gn_cpg = cpg;
    return vqkd::launch_conv3x3_x3(x, w5, bias, residual, y, zeros, g, 0, g_stream_blocks, vqk_stream(stream));
}

int vqk_conv2d_thin_in_gnstats(int dtype, const void* x, const void* w, const float* bias, void* y, int n, int h, int wd, int cout,
                               double* gn_ws, int groups, void* stream) {
    VQK_REQUIRE(x && w && y && gn_ws, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(w) && vqk_aligned16(y), VQK_ERR_ALIGN);
    VQK_REQUIRE(dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(n > 0 && h > 0 && wd > 0, VQK_ERR_SHAPE);
    // served: 128 output channels in 32 groups (4 channels per group), whole 32-pixel row segments, not in deterministic mode
    // (its per-tile slots exist on the role-split kernel only), and a wave count that splits evenly over images and over an image's tiles
    VQK_REQUIRE(cout == 128 && groups == 32 && (wd % 32) == 0 && !g_det && g_force_variant != CONV_VARIANT_IM2COL, VQK_ERR_SHAPE);
    ConvGeom g;
    const int rc = make_geom(g, dtype, n, h, wd, 8, cout, 3, 0);
    if (rc) return rc;
    const int tpi = h * (wd >> 5);
    int wpi = 0;
    for (int c = 4096 / n; c >= 1; --c)
        if (tpi % c == 0 && ((n * c) & 3) == 0) { wpi = c; break; }
    VQK_REQUIRE(wpi > 0, VQK_ERR_SHAPE);
    g.gn_ws = gn_ws; g.gn_cpg = 4;
    hipLaunchKernelGGL((conv3x3_thin_in_kernel<4, true>), dim3((unsigned)(n * wpi / 4)), dim3(256), 4 * 32 * (4 * 64 + 8) + 4 * 128,
                       vqk_stream(stream), (const bf16_raw*)x, (const bf16_raw*)w, bias, (bf16_raw*)y, g, 0, 0);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

static int ups_phase_impl(int dtype, const void* x, const void* w4, const float* bias, void* y, int n, int h, int w, int cin,
                          int cout, int backward, double* gn_ws, int groups, const void* zeros, void* stream, int phase_rev,
                          float acc_scale, const void* res = nullptr);

int vqk_conv2d_ups_phase(int dtype, const void* x, const void* w4, const float* bias, void* y, int n, int h, int w,
                         int cin, int cout, int backward, double* gn_ws, int groups, const void* zeros, void* stream) {
    return ups_phase_impl(dtype, x, w4, bias, y, n, h, w, cin, cout, backward, gn_ws, groups, zeros, stream, 0, 1.0f);
}

int vqk_conv2d_pooled_dgrad_phase(int dtype, const void* dy_pooled, const void* w4t, void* dx, int n, int h, int w, int cin,
                                  int cout, float scale, const void* zeros, void* stream) {
    // dx [n, 2h, 2w, cout] = scale * (nearest-x2(dy_pooled) * flip(W)^T): forward-type phase launch on the pooled gradient with
    // the conv's data-gradient operand, phase blocks reversed (conv_geom.h: phase_rev).  cin = channels of dy_pooled (the conv's
    // output channels), cout = channels of dx (its input channels).  One launch (UPS_MERGE) only.
    VQK_REQUIRE(VQK_TUNE("UPS_MERGE", 1) != 0, VQK_ERR_SHAPE);
    return ups_phase_impl(dtype, dy_pooled, w4t, nullptr, dx, n, h, w, cin, cout, 0, nullptr, 0, zeros, stream, 1, scale);
}

int vqk_conv2d_pooled_fprop_phase(int dtype, const void* x, const void* w4, const void* res_pooled, void* y, int n, int h, int w,
                                  int cin, int cout, float scale, double* gn_ws, int groups, const void* zeros, void* stream) {
    // y [n, h, w, cout] = scale * sum over each 2x2 block of conv3x3(x)  (+ res_pooled), x [n, 2h, 2w, cin]: a 4x4 stride-2 conv =
    // the DATA-GRADIENT-type phase launch (phase = a unit dimension, the tile accumulates the four input phases in registers)
    // with the conv's FORWARD phase operand, phase blocks reversed: scale * sum_{2x2} conv(x, W) == dgrad_ups(x; V = scale flip(W)^T)
    // and the phase pack of V^T = flip(W) is the pack of W with phase (a, b) <-> (1-a, 1-b).
    VQK_REQUIRE(VQK_TUNE("UPS_MERGE", 1) != 0, VQK_ERR_SHAPE);
    VQK_REQUIRE(!gn_ws || (groups > 0 && cout % groups == 0 && (cout / groups) % 4 == 0), VQK_ERR_SHAPE);
    return ups_phase_impl(dtype, x, w4, nullptr, y, n, h, w, cin, cout, 1, gn_ws, groups, zeros, stream, 1, scale, res_pooled);
}

static int ups_phase_impl(int dtype, const void* x, const void* w4, const float* bias, void* y, int n, int h, int w, int cin,
                          int cout, int backward, double* gn_ws, int groups, const void* zeros, void* stream, int phase_rev,
                          float acc_scale, const void* res) {
    VQK_REQUIRE(x && w4 && y && zeros, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(w4) && vqk_aligned16(y), VQK_ERR_ALIGN);
    VQK_REQUIRE(dtype == VQK_BF16 || dtype == VQK_F32, VQK_ERR_DTYPE);
    VQK_REQUIRE(backward == 0 || backward == 1, VQK_ERR_ARG);
    if (dtype == VQK_F32) {
        // the split-product mode (conv_x3.hip NTAP = 4; w4 in layout 6): fp32 tensors, one launch for the four phases
        VQK_REQUIRE(!gn_ws || ((!backward || phase_rev) && groups > 0 && cout % groups == 0), VQK_ERR_SHAPE);
        const int cpg = gn_ws ? cout / groups : 0;
        VQK_REQUIRE(!gn_ws || cpg == 4 || cpg == 8 || cpg == 16, VQK_ERR_SHAPE);
        VQK_REQUIRE(!res || (backward && phase_rev && vqk_aligned16(res)), VQK_ERR_ARG);
        VQK_REQUIRE(!g_det || !gn_ws, VQK_ERR_SHAPE);                        // (its GroupNorm sums are atomic)
        ConvGeom gx;
        const int rcx = make_geom(gx, dtype, n, h, w, cin, cout, 3, 0);      // tiles over the LOW-resolution h x w grid
        if (rcx) return rcx;
        VQK_REQUIRE((cin % 32) == 0 && (cout % 128) == 0 && (h % 8) == 0 && (w % 16) == 0 && VQK_TUNE("UPS_PHASE", 1), VQK_ERR_SHAPE);
        gx.ntap = 4;
        gx.phase_mode = backward ? 2 : 1;
        if (backward) { gx.h_in = 2 * h; gx.w_in = 2 * w; }
        gx.phase_rev = phase_rev; gx.acc_scale = acc_scale;
        gx.gn_ws = gn_ws; gx.gn_cpg = cpg;
        return vqkd::launch_conv3x3_x3(x, w4, backward ? nullptr : bias, res, y, zeros, gx, 0, 0, vqk_stream(stream));
    }
    VQK_REQUIRE(!gn_ws || ((!backward || phase_rev) && groups > 0 && cout % groups == 0 && (cout / groups) % 4 == 0), VQK_ERR_SHAPE);
    VQK_REQUIRE(!res || (backward && phase_rev && vqk_aligned16(res)), VQK_ERR_ARG);
    ConvGeom g;
    const int rc = make_geom(g, dtype, n, h, w, cin, cout, 3, 0);            // tiles over the LOW-resolution h x w grid
    if (rc) return rc;
    const int tw = halo_twlog(g, g_force_variant);
    const int mx_on = VQK_TUNE("MX", 1);
    const int ph_on = VQK_TUNE("UPS_PHASE", 1);
    VQK_REQUIRE(tw && mx_on && ph_on && (cout % 128) == 0 && (g.cpt >> 2) >= 2 && g_force_variant != CONV_VARIANT_NO_MX, VQK_ERR_SHAPE);
    VQK_REQUIRE((int64_t)4 * g.m * (backward ? cin : cout) * 2 < 0x7fffffffLL && (int64_t)g.m * (backward ? cout : cin) * 2 < 0x7fffffffLL,
                VQK_ERR_SHAPE);
    g.ntap = 4;
    const int64_t phase_elems = (int64_t)((cout + 127) / 128) * 128 * cin * 4;
    hipStream_t st = vqk_stream(stream);
    if (VQK_TUNE("UPS_MERGE", 1)) {
        // one launch for the four phases (conv_mx.hip: ConvGeom::phase_mode)
        ConvGeom gp = g;
        if (!backward) {
            gp.phase_mode = 1;
            gp.dst_s = 2;
            gp.phase_rev = phase_rev; gp.acc_scale = acc_scale;
            gp.gn_ws = gn_ws; gp.gn_cpg = gn_ws ? cout / groups : 0;
            if (gn_ws && g_det) { gp.gn_part_nblk = 4 * ((g.h * g.w) / 256); gp.gn_part_base = 0; }
        } else {
            gp.phase_mode = 2;
            gp.src_s = 2;
            gp.h_in = 2 * h; gp.w_in = 2 * w;
            gp.phase_rev = phase_rev; gp.acc_scale = acc_scale;              // (the pooled FORWARD: vqk_conv2d_pooled_fprop_phase)
            gp.gn_ws = gn_ws; gp.gn_cpg = gn_ws ? cout / groups : 0;
            if (gn_ws && g_det) { gp.gn_part_nblk = (g.h * g.w) / 256; gp.gn_part_base = 0; }
        }
        gp.unit64 = mx_phase_u64_serves(gp, tw);
        return vqkd::launch_conv3x3_mx(x, w4, backward ? nullptr : bias, res, y, zeros, gp, tw, st);
    }
    for (int ph = 0; ph < 4; ++ph) {
        const int a = ph >> 1, b = ph & 1;
        ConvGeom gp = g;
        const void* res = nullptr;
        if (!backward) {                                     // y[2i+a][2j+b] = 2x2 window of x at rows i+a-1.., columns j+b-1..
            gp.tap_oy = a; gp.tap_ox = b;
            gp.dst_s = 2; gp.dst_a = a; gp.dst_b = b;
            gp.gn_ws = gn_ws; gp.gn_cpg = gn_ws ? cout / groups : 0;
            if (gn_ws && g_det) { gp.gn_part_nblk = 4 * ((g.h * g.w) / 256); gp.gn_part_base = ph * ((g.h * g.w) / 256); }
        } else {                                             // dx[i][j] += mirrored 2x2 window of the phase (a, b) of dy
            gp.tap_oy = 1 - a; gp.tap_ox = 1 - b;
            gp.src_s = 2; gp.src_a = a; gp.src_b = b;
            gp.h_in = 2 * h; gp.w_in = 2 * w;                // the source tensor is dy at full resolution
            res = ph ? y : nullptr;                          // later phases accumulate in place
        }
        gp.unit64 = mx_phase_u64_serves(gp, tw);
        const int r = vqkd::launch_conv3x3_mx(x, (const bf16_raw*)w4 + ph * phase_elems, backward ? nullptr : bias, res, y, zeros, gp, tw, st);
        if (r != VQK_OK) return r;
    }
    return VQK_OK;
}

// ---- the stride-2 3x3 conv without padding of the StyleGAN2 discriminator (conv2d_resample.py:119-122: blur, then
// F.conv2d(stride=2)) on the matrix/auxiliary-wave kernel.  Input (2 h_out + 1) x (2 w_out + 1), output h_out x w_out.
static int s2_twlog(int h_out, int w_out, int pix) {
    if ((w_out % 32) == 0 && (h_out % (pix / 32)) == 0) return 5;
    if ((w_out % 16) == 0 && (h_out % (pix / 16)) == 0) return 4;
    return 0;
}

int vqk_conv2d_s2_supported(int dtype, int n, int h_out, int w_out, int cin, int cout, int backward) {
    if (dtype != VQK_BF16 || n <= 0 || h_out <= 0 || w_out <= 0 || cin <= 0 || cout <= 0) return 0;
    if (!VQK_TUNE("MX", 1) || !VQK_TUNE("MX_S2", 1) || g_force_variant == CONV_VARIANT_IM2COL || g_force_variant == CONV_VARIANT_NO_MX) return 0;
    const int64_t big = (int64_t)n * (2 * h_out + 1) * (2 * w_out + 1) * cin * 2, small = (int64_t)n * h_out * w_out * cout * 2;
    if (big >= 0x7fffffffLL || small >= 0x7fffffffLL) return 0;
    if (!backward) return (cin % 64) == 0 && (cout % 128) == 0 && s2_twlog(h_out, w_out, 128) != 0;
    // the data gradient: dy's channels are the reduction, the layer's input channels the output tile; 32x32 maps and larger
    // (below, the four phases are a handful of tiles each and the im2col kernel's parity classes do as well)
    return (cout % 64) == 0 && (cin % 128) == 0 && s2_twlog(h_out, w_out, 256) != 0 && w_out >= VQK_TUNE("MX_S2_DGRAD_MIN", 32);
}

int vqk_conv2d_s2_fprop(int dtype, const void* x, const void* wq, const float* bias, void* y, int n, int h_out, int w_out,
                        int cin, int cout, int act, float acc_scale, float out_gain, const void* zeros, void* stream) {
    VQK_REQUIRE(x && wq && y && zeros, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(x) && vqk_aligned16(wq) && vqk_aligned16(y), VQK_ERR_ALIGN);
    VQK_REQUIRE(act == 0 || act == 2 || act == 3, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_conv2d_s2_supported(dtype, n, h_out, w_out, cin, cout, 0), VQK_ERR_SHAPE);
    ConvGeom g;
    const int rc = make_geom(g, dtype, n, h_out, w_out, cin, cout, 3, 0);      // tiles over the OUTPUT grid
    if (rc) return rc;
    g.h_in = 2 * h_out + 1; g.w_in = 2 * w_out + 1;
    g.src_s = 2; g.s2 = 1;
    g.act = act; g.acc_scale = acc_scale; g.out_gain = out_gain;
    return vqkd::launch_conv3x3_mx(x, wq, bias, nullptr, y, zeros, g, s2_twlog(h_out, w_out, 128), vqk_stream(stream));
}

int vqk_conv2d_s2_dgrad(int dtype, const void* dy, const void* w3, const void* wt0, void* dx, int n, int h_out, int w_out,
                        int cin, int cout, float acc_scale, const void* zeros, void* stream) {
    VQK_REQUIRE(dy && w3 && wt0 && dx && zeros, VQK_ERR_ARG);
    VQK_REQUIRE(vqk_aligned16(dy) && vqk_aligned16(w3) && vqk_aligned16(wt0) && vqk_aligned16(dx) && vqk_aligned16(zeros), VQK_ERR_ALIGN);
    VQK_REQUIRE(vqk_conv2d_s2_supported(dtype, n, h_out, w_out, cin, cout, 1), VQK_ERR_SHAPE);
    hipStream_t st = vqk_stream(stream);
    const int H = 2 * h_out + 1, W = 2 * w_out + 1;
    // (1) the h_out x w_out interior of every output parity: whole tiles on the matrix/auxiliary-wave kernel
    ConvGeom g;
    int rc = make_geom(g, dtype, n, h_out, w_out, cout, cin, 3, 0);
    if (rc) return rc;
    const int tw = s2_twlog(h_out, w_out, 256);
    g.acc_scale = acc_scale;
    g.dst_s = 2; g.dst_h = H; g.dst_w = W;
    const int64_t tap_elems = (int64_t)((cin + 127) / 128) * 128 * cout;
    const int tap0[4] = {0, 4, 6, 8};
    for (int ph = 0; ph < 4; ++ph) {
        const int a = ph >> 1, b = ph & 1, na = a ? 1 : 2, nb = b ? 1 : 2;
        ConvGeom gp = g;
        gp.ntap = na * nb; gp.tapw = gp.ntap == 2 ? nb : 0;
        gp.tap_oy = (gp.ntap > 1 && a) ? 1 : 0;                   // a one-row window sits on the halo's centre row
        gp.tap_ox = (gp.ntap > 1 && b) ? 1 : 0;
        gp.dst_a = a; gp.dst_b = b;
        rc = vqkd::launch_conv3x3_mx(dy, (const bf16_raw*)w3 + tap0[ph] * tap_elems, nullptr, nullptr, dx, zeros, gp, tw, st);
        if (rc != VQK_OK) return rc;
    }
    // (2) the last row (2 h_out) and the last column (2 w_out) of the gradient: the im2col kernel's parity classes, cut down to them
    ConvGeom e;
    rc = make_geom(e, dtype, n, h_out, w_out, cout, cin, 3, 1);
    if (rc) return rc;
    e.zs = 1; e.vh = 2 * h_out - 1; e.vw = 2 * w_out - 1; e.stride = 1; e.pad = 2;
    e.h = H; e.w = W; e.m = n * H * W; e.tiles_m = (e.m + 127) / 128;
    e.acc_scale = acc_scale;
    const int edge[4][4] = {{2 * h_out, 1, 0, w_out + 1},        // {sub_py, sub_h, sub_px, sub_w}: row 2h, every even column
                            {0, h_out, 2 * w_out, 1},            // column 2w, the even rows above the corner
                            {2 * h_out, 1, 1, w_out},            // row 2h, odd columns
                            {1, h_out, 2 * w_out, 1}};           // column 2w, odd rows
    for (int k = 0; k < 4 && rc == VQK_OK; ++k) {
        ConvGeom gs = e;
        gs.sub = 1; gs.sub_py = edge[k][0]; gs.sub_h = edge[k][1]; gs.sub_px = edge[k][2]; gs.sub_w = edge[k][3];
        gs.nkh = gs.nkw = 0;
        for (int kk = 0; kk < 3; ++kk) {
            if (((gs.sub_py + kk - 2) & 1) == 0) gs.khl[gs.nkh++] = kk;
            if (((gs.sub_px + kk - 2) & 1) == 0) gs.kwl[gs.nkw++] = kk;
        }
        gs.kchunks = gs.nkh * gs.nkw * gs.cpt;
        gs.m = n * gs.sub_h * gs.sub_w;
        gs.tiles_m = (gs.m + 127) / 128;
        rc = launch_fprop<bf16_raw, bf16_raw>(dy, wt0, nullptr, nullptr, dx, zeros, gs, 0, 0, CONV_VARIANT_IM2COL, st);
    }
    return rc;
}

int vqk_conv2d_general(int dtype, const void* x, const void* w, const float* bias, const void* residual, void* y,
                       int out_dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int stride, int pad,
                       int mode, int h_out, int w_out, int act, float acc_scale, float out_gain, int wlayout,
                       const void* zeros, void* stream) {
    return conv_general(dtype, x, w, bias, residual, y, out_dtype, n, h_in, w_in, cin, cout, ksize, stride, pad, mode,
                        h_out, w_out, act, acc_scale, out_gain, wlayout, zeros, stream);
}

int vqk_conv_weight_layout(int dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int ups) {
    ConvGeom g;
    const int rc = make_geom(g, dtype, n, h_in, w_in, cin, cout, ksize, ups);
    if (rc) return rc;
    if (ksize == 1 && dtype != VQK_BF16) return 0;
    if (dtype == VQK_F32 && thin_out_f32_serves(g, g_force_variant))
        return 0;                                                // the 3-channel head in the fp32 modes: conv_thin_f32.hip (plain weights)
    return (halo_twlog(g, g_force_variant) && g_force_variant != CONV_VARIANT_PLAIN_WEIGHTS) ? 1 : 0;
}

int vqk_conv_fprop_plan(int dtype, int out_dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int ups, int act,
                        int wlayout, int flags, int* details) {
    VQK_REQUIRE(act >= 0 && act <= 3 && (wlayout == 0 || wlayout == 1 || wlayout == 5) && (ups == 0 || ups == 1) &&
                flags >= 0 && flags < 16, VQK_ERR_ARG);
    const bool has_res = flags & 1, pool = flags & 2, gnstats = flags & 4, general = flags & 8;
    if (pool || gnstats) {                                       // vqk_conv2d_fprop_pooled / _gnstats
        VQK_REQUIRE(dtype == VQK_BF16 && out_dtype == VQK_BF16, VQK_ERR_DTYPE);
        VQK_REQUIRE(act == 0 && wlayout == 1 && !general, VQK_ERR_ARG);
        VQK_REQUIRE(!gnstats || ksize == 3, VQK_ERR_SHAPE);
    }
    ConvGeom g;
    const int rc = make_geom(g, dtype, n, h_in, w_in, cin, cout, ksize, ups);
    if (rc) return rc;
    FpropPlan p = {VQK_OK, FORM_X3, 0, 0, 1, 0, 1};
    if (wlayout == 5) {                                          // conv_general: the split-product kernel, plain convs only
        VQK_REQUIRE(!general && dtype == VQK_F32 && out_dtype == VQK_F32, VQK_ERR_ARG);
        VQK_REQUIRE(vqkd::conv3x3_x3_serves(g), VQK_ERR_SHAPE);
        if (ksize == 1) p.form = FORM_X3_1X1;
    } else {
        VQK_REQUIRE(!general || wlayout == 0, VQK_ERR_ARG);
        VQK_REQUIRE(out_dtype == VQK_F32 || (out_dtype == VQK_BF16 && dtype == VQK_BF16), VQK_ERR_DTYPE);
        if (pool || gnstats) {
            VQK_REQUIRE(fused_epilogue_serves(g, g_force_variant), VQK_ERR_SHAPE);
            g.pool = pool;
            if (gnstats) g.gn_ws = reinterpret_cast<double*>(sizeof(double));   // "present": a plan never dereferences it
        }
        p = plan_fprop(g, dtype, out_dtype, act, wlayout, has_res, general ? (int)CONV_VARIANT_IM2COL : g_force_variant);
        if (p.status != VQK_OK) return p.status;
    }
    if (details) {
        const bool membound = p.form == FORM_THIN_OUT_F32 || p.form == FORM_THIN_IN_F32 || p.form == FORM_MX_1X1 ||
                              p.form == FORM_THIN_IN_BF16 || p.form == FORM_X3_1X1;
        details[0] = p.tw; details[1] = p.blocks; details[2] = p.splits; details[3] = p.launches; details[4] = membound;
    }
    return p.form;
}

const char* vqk_conv_fprop_form_name(int form, int dtype) {
    static const char* const names[FORM_COUNT][2] = {
        {"conv3x3_thin_out_f32_kernel (HBM)", "conv3x3_thin_out_f32_kernel (HBM)"},
        {"conv3x3_thin_in_f32_kernel (HBM)", "conv3x3_thin_in_f32_kernel (HBM)"},
        {"conv3x3_mx_kernel<bf16>", "conv3x3_mx_kernel<bf16>"},
        {"conv1x1_mx_kernel<bf16> (HBM)", "conv1x1_mx_kernel<bf16> (HBM)"},
        {"conv3x3_stream_kernel<bf16>", "conv3x3_stream_kernel<bf16>"},
        {"conv3x3_stream_kernel<bf16>", "conv3x3_stream_kernel<bf16>"},
        {"conv3x3_stream_kernel<bf16>", "conv3x3_stream_kernel<bf16>"},
        {"conv3x3_halo_breg_kernel<f32>", "conv3x3_halo_breg_kernel<bf16>"},
        {"conv3x3_halo_kernel<f32>", "conv3x3_halo_kernel<bf16>"},
        {"conv3x3_thin_in_kernel<bf16> (HBM)", "conv3x3_thin_in_kernel<bf16> (HBM)"},
        {"conv_fprop_kernel<f32>", "conv_fprop_kernel<bf16>"},
        {"conv_fprop_kernel<f32>", "conv_fprop_kernel<bf16>"},
        {"conv3x3_x3_kernel<f32 as 3 x bf16>", "conv3x3_x3_kernel<f32 as 3 x bf16>"},
        {"conv1x1_x3_kernel<f32 as 3 x bf16> (HBM)", "conv1x1_x3_kernel<f32 as 3 x bf16> (HBM)"},
    };
    if (form < 0 || form >= FORM_COUNT || (dtype != VQK_F32 && dtype != VQK_BF16)) return "?";
    return names[form][dtype == VQK_BF16];
}

}  // extern "C"
