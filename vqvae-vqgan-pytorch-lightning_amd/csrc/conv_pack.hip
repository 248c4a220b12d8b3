// Weight operands of the conv kernels for gfx950, built from the fp32 [Cout][taps][Cin] master (typically a view into the
// AdamW arena): the layouts of include/vqk.h ("Weight operand layouts").  ONE implementation serves the single-operand entry
// (vqk_conv_pack_weights, pack_one_kernel) and the once-per-step table launch (vqk_conv_pack_multi, pack_multi_kernel).
//   0        [Cout][taps][Cin], one element per thread; transpose: [Cin][taps flipped][Cout], the dgrad operand
//   1        fragment-major [cot][cc][tap][ks][kg][co32][E]: cot = tile of 32 output channels (Cout padded to 128 with zeros),
//            cc = chunk of 4 x 16 bytes of input channels, E = elements per 16 bytes, channel = ((cc*2 + ks)*2 + kg)*E + e.
//            All 18 (tap, ks) fragments of one (cot, cc) are contiguous (18 KiB), which is what one pipeline unit reads.
//   2        four upsample phases (a, b) x fragment-major blocks of FOUR taps (r, s) (conv_mx.hip, ConvGeom::ntap == 4): a tap is
//            the SUM of the 3x3 taps that land on the same low-resolution pixel; transpose: the 2x2 taps mirrored
//   3        data gradient of a STRIDE-2 3x3 conv without padding, by output parity (vqk_conv2d_s2_dgrad): dx[2i+a][2j+b] sums
//            the taps ky = a, kx = b (mod 2) -- fragment-major blocks of 4 / 2 / 2 / 1 taps for (a, b) = (0,0) / (0,1) / (1,0) /
//            (1,1), always transposed; window tap (wy, wx) reads dy[i - 1 + wy] when the phase has two rows (wy = 0: ky = 2,
//            wy = 1: ky = 0), dy[i] (ky = 1) otherwise
//   5, 6     split-product mode (conv_x3.hip): layouts 1 and 2 in bf16 with every fragment TWICE, hi = bf16_rne(w), lo =
//            bf16_rne(w - hi): [..][tap][ks][hi | lo][kg][co32][8].  Byte size of the fp32 operand (4 B per weight)
// In the fragment-major layouts one thread builds one 16-byte piece (E consecutive input channels of one output channel) and
// is its only writer, so the result does not depend on the grid.  They differ only in how a piece is gathered and stored.
#include "common.h"

namespace {

template <typename TD>
__global__ void cast_kernel(const float* __restrict__ s, TD* __restrict__ d, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        Elem<TD>::st(d + i, s[i]);
}

// piece index within a block of `ntap` taps -> position in [phase][cot][cc][tap][ks][kg][co32] (phases only when `phased`)
__device__ __forceinline__ void frag_decode(int64_t r, int ntap, int ncc, int cot_tiles, bool phased, int& co32, int& kg, int& ks,
                                            int& tap, int& cc, int& cot, int& ph) {
    co32 = (int)(r & 31); r >>= 5;
    kg = (int)(r & 1); r >>= 1;
    ks = (int)(r & 1); r >>= 1;
    tap = (int)(r % ntap); r /= ntap;
    cc = (int)(r % ncc); r /= ncc;
    cot = phased ? (int)(r % cot_tiles) : (int)r;
    ph = phased ? (int)(r / cot_tiles) : 0;
}

// the 3x3 taps k0..k1 (one axis) that fall on tap t of upsample phase p: {0}, {1,2} for p = 0 and {0,1}, {2} for p = 1
__device__ __forceinline__ void phase_taps(int p, int t, int& k0, int& k1) {
    k0 = t == 0 ? 0 : 1 + p;
    k1 = t == 0 ? p : 2;
}

// the E source values of a piece: input channels ci .. ci+E-1 of output channel co at tap `tap` of `taps`; transpose: the
// roles of the master's Cout / Cin swapped (a strided gather)
template <int E>
__device__ __forceinline__ void gather(const float* __restrict__ w, int cin, int taps, int co, int ci, int tap, int transpose,
                                       float (&v)[E]) {
    if (!transpose) {
        const float* src = w + ((int64_t)co * taps + tap) * cin + ci;
#pragma unroll
        for (int q = 0; q < E / 4; ++q) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(src + 4 * q);
            v[4 * q] = t[0]; v[4 * q + 1] = t[1]; v[4 * q + 2] = t[2]; v[4 * q + 3] = t[3];
        }
    } else {
        const float* src = w + ((int64_t)ci * taps + tap) * cin + co;
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = src[(int64_t)e * taps * cin];
    }
}

// hi = bf16(v) at dst, lo = bf16(v - hi) one fragment (64 pieces) later
__device__ __forceinline__ void store_hi_lo(bf16_raw* __restrict__ dst, const float (&v)[8]) {
    const vqk_u32x4 hi = vqk_pack_bf16x8(v);
    float lo[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        lo[2 * q] = v[2 * q] - __uint_as_float(hi[q] << 16);
        lo[2 * q + 1] = v[2 * q + 1] - __uint_as_float(hi[q] & 0xffff0000u);
    }
    *reinterpret_cast<vqk_u32x4*>(dst) = hi;
    *reinterpret_cast<vqk_u32x4*>(dst + 64 * 8) = vqk_pack_bf16x8(lo);
}

template <typename TD>
__device__ __forceinline__ void pack_plain(const float* __restrict__ w, TD* __restrict__ out, int cout, int cin, int taps,
                                           int transpose) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const int64_t total = (int64_t)cout * taps * cin;
    if (!transpose) {
        for (int64_t o = tid; o < total; o += nthr) Elem<TD>::st(out + o, w[o]);
    } else {
        for (int64_t o = tid; o < total; o += nthr) {                   // o indexes the destination [ci][tap][co]
            const int co = (int)(o % cout);
            const int64_t r = o / cout;
            const int tap = (int)(r % taps), ci = (int)(r / taps);
            Elem<TD>::st(out + o, w[((int64_t)co * taps + (taps - 1 - tap)) * cin + ci]);
        }
    }
}

// the fragment-major layouts.  form 1: the taps as they are; 2: phase-summed (fp32 sums from 0.0f, ky outer, kx inner); 3: stride-2
// parity blocks.  split: (hi | lo) bf16 pairs (TD = bf16_raw).  form and split are literals at every call site.
template <typename TD>
__device__ __forceinline__ void pack_frag(const float* __restrict__ w, TD* __restrict__ out, int cout, int cin, int taps, int transpose,
                                          int form, bool split) {
    constexpr int E = Elem<TD>::kPer16B;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    if (form == 3) transpose = 1;
    const int dcout = transpose ? cin : cout, dcin = transpose ? cout : cin;
    const int cot_tiles = ((dcout + 127) / 128) * 4;
    const int ncc = dcin / (4 * E);
    const int64_t per_tap = (int64_t)cot_tiles * ncc * 2 * 64;              // 16-byte pieces ((hi, lo) pairs of them when split)
    const int64_t total = per_tap * (form == 1 ? taps : form == 2 ? 16 : 9);
    for (int64_t o = tid; o < total; o += nthr) {
        int co32, kg, ks, tap, cc, cot, ph;
        if (form == 3) {
            const int p = o < 4 * per_tap ? 0 : o < 6 * per_tap ? 1 : o < 8 * per_tap ? 2 : 3;
            const int nt = (p & 2 ? 1 : 2) * (p & 1 ? 1 : 2);
            frag_decode(o - (p == 0 ? 0 : p == 1 ? 4 : p == 2 ? 6 : 8) * per_tap, nt, ncc, cot_tiles, false, co32, kg, ks, tap, cc, cot, ph);
            ph = p;
        } else {
            frag_decode(o, form == 2 ? 4 : taps, ncc, cot_tiles, form == 2, co32, kg, ks, tap, cc, cot, ph);
        }
        const int co = cot * 32 + co32;
        const int ci = ((cc * 2 + ks) * 2 + kg) * E;
        float v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = 0.0f;
        if (co < dcout) {
            if (form == 2) {
                const int t = transpose ? 3 - tap : tap;
                int ky0, ky1, kx0, kx1;
                phase_taps(ph >> 1, t >> 1, ky0, ky1);
                phase_taps(ph & 1, t & 1, kx0, kx1);
                for (int ky = ky0; ky <= ky1; ++ky)
                    for (int kx = kx0; kx <= kx1; ++kx) {
                        float s[E];
                        gather<E>(w, cin, 9, co, ci, ky * 3 + kx, transpose, s);
#pragma unroll
                        for (int e = 0; e < E; ++e) v[e] += s[e];
                    }
            } else if (form == 3) {
                const int nb = ph & 1 ? 1 : 2, wy = tap / nb, wx = tap - wy * nb;
                gather<E>(w, cin, 9, co, ci, (ph & 2 ? 1 : (wy == 0 ? 2 : 0)) * 3 + (ph & 1 ? 1 : (wx == 0 ? 2 : 0)), 1, v);
            } else {
                gather<E>(w, cin, taps, co, ci, transpose ? taps - 1 - tap : tap, transpose, v);
            }
        }
        if constexpr (E == 8) {
            if (split) { store_hi_lo(out + (((o >> 6) << 7) + (o & 63)) * 8, v); continue; }     // fragment o >> 6 is pair o >> 6
        }
        Vec16<TD>::store(out + o * E, v);
    }
}

template <typename TD>
__device__ __forceinline__ void pack_layout(const float* __restrict__ w, TD* __restrict__ out, int cout, int cin, int taps, int tr,
                                            int lay) {
    if (lay == 0) pack_plain<TD>(w, out, cout, cin, taps, tr);
    else if (lay == 2) pack_frag<TD>(w, out, cout, cin, taps, tr, 2, false);
    else if (lay == 3) pack_frag<TD>(w, out, cout, cin, taps, tr, 3, false);
    else pack_frag<TD>(w, out, cout, cin, taps, tr, 1, false);
}

// one operand; the arguments of vqk_conv_pack_weights
__device__ __forceinline__ void pack_operand(const float* __restrict__ src, void* __restrict__ dst, int dtype, int cout, int cin, int ks,
                                             int tr, int lay) {
    if (lay == 5) pack_frag<bf16_raw>(src, reinterpret_cast<bf16_raw*>(dst), cout, cin, ks * ks, tr, 1, true);
    else if (lay == 6) pack_frag<bf16_raw>(src, reinterpret_cast<bf16_raw*>(dst), cout, cin, ks * ks, tr, 2, true);
    else if (dtype == VQK_F32) pack_layout<float>(src, reinterpret_cast<float*>(dst), cout, cin, ks * ks, tr, lay);
    else pack_layout<bf16_raw>(src, reinterpret_cast<bf16_raw*>(dst), cout, cin, ks * ks, tr, lay);
}

// One launch for every conv operand of the model: desc d is packed by blocks (blockIdx.y == d).  The descriptor
// is eight int64 words {src, dst, dtype, cout, cin, ksize, transpose, layout} with the meaning of the arguments of
// vqk_conv_pack_weights.
__global__ __launch_bounds__(256) void pack_multi_kernel(const int64_t* __restrict__ descs) {
    const int64_t* d = descs + (int64_t)blockIdx.y * 8;
    pack_operand(reinterpret_cast<const float*>(d[0]), reinterpret_cast<void*>(d[1]), (int)d[2], (int)d[3], (int)d[4], (int)d[5],
                 (int)d[6], (int)d[7]);
}

// the same packing for ONE operand, descriptor by value (no device table: usable under stream capture)
__global__ __launch_bounds__(256) void pack_one_kernel(const float* __restrict__ src, void* __restrict__ dst, int dtype, int cout,
                                                       int cin, int ks, int tr, int lay) {
    pack_operand(src, dst, dtype, cout, cin, ks, tr, lay);
}

}  // namespace

extern "C" {

int64_t vqk_conv_packed_elems(int cout, int cin, int ksize, int layout) {
    if (layout == 0) return (int64_t)cout * cin * ksize * ksize;
    if (layout == 2 || layout == 6) return (int64_t)4 * ((cout + 127) / 128) * 128 * cin * 4;      // four phases x four taps (6: fp32-sized (hi, lo) pairs)
    if (layout == 3) return (int64_t)((cout + 127) / 128) * 128 * cin * 9;          // four phases, 4 + 2 + 2 + 1 taps
    return (int64_t)((cout + 127) / 128) * 128 * cin * ksize * ksize;
}

int vqk_conv_pack_weights(const float* w, void* out, int dtype, int cout, int cin, int ksize, int transpose, int layout,
                          void* stream) {
    VQK_REQUIRE(w && out, VQK_ERR_ARG);
    VQK_REQUIRE(cout > 0 && cin > 0 && (ksize == 1 || ksize == 3), VQK_ERR_SHAPE);
    VQK_REQUIRE(dtype == VQK_F32 || dtype == VQK_BF16, VQK_ERR_DTYPE);
    VQK_REQUIRE(layout == 0 || layout == 1 || layout == 2 || layout == 3 || layout == 5 || layout == 6, VQK_ERR_ARG);
    const int dcout = transpose ? cin : cout, dcin = transpose ? cout : cin;
    const int e = dtype == VQK_F32 ? 4 : 8;
    int64_t work = vqk_conv_packed_elems(dcout, dcin, ksize, layout);            // elements (layout 0) or 16-byte pieces
    if (layout != 0) {
        VQK_REQUIRE(dcin % (8 * e) == 0, VQK_ERR_SHAPE);                         // whole channel chunks (bf16: 64, fp32 and split: 32)
        if (layout == 2 || layout == 3) VQK_REQUIRE(ksize == 3 && dtype == VQK_BF16 && (layout == 2 || transpose), VQK_ERR_SHAPE);
        if (layout == 5 || layout == 6) VQK_REQUIRE(dtype == VQK_F32 && (layout == 5 || ksize == 3), VQK_ERR_SHAPE);
        VQK_REQUIRE(vqk_aligned16(w) && vqk_aligned16(out), VQK_ERR_ALIGN);      // 16-byte loads and stores
        work /= (layout == 5 || layout == 6) ? 2 * e : e;
    }
    hipLaunchKernelGGL(pack_one_kernel, dim3(vqk_grid_1d(work, 256)), dim3(256), 0, vqk_stream(stream), w, out, dtype, cout, cin, ksize,
                       transpose, layout);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

int vqk_conv_pack_multi(const int64_t* descs_dev, int ndesc, int blocks_per_desc, void* stream) {
    VQK_REQUIRE(descs_dev && ndesc >= 0 && blocks_per_desc > 0 && blocks_per_desc <= 4096 && ndesc <= 65535, VQK_ERR_ARG);
    if (ndesc == 0) return VQK_OK;
    hipLaunchKernelGGL(pack_multi_kernel, dim3((unsigned)blocks_per_desc, (unsigned)ndesc), dim3(256), 0, vqk_stream(stream),
                       descs_dev);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

// w [Cout][taps][Cin] fp32 -> wt [Cin][taps (flipped)][Cout]
int vqk_conv_pack_dgrad(const float* w, void* wt, int dtype, int cout, int cin, int ksize, void* stream) {
    return vqk_conv_pack_weights(w, wt, dtype, cout, cin, ksize, 1, 0, stream);
}

int vqk_cast(const float* src, void* dst, int dtype, int64_t n, void* stream) {
    VQK_REQUIRE(src && dst, VQK_ERR_ARG);
    if (n <= 0) return VQK_OK;
    const dim3 grid(vqk_grid_1d(n, 256));
    if (dtype == VQK_F32) hipLaunchKernelGGL(cast_kernel<float>, grid, dim3(256), 0, vqk_stream(stream), src, (float*)dst, n);
    else if (dtype == VQK_BF16) hipLaunchKernelGGL(cast_kernel<bf16_raw>, grid, dim3(256), 0, vqk_stream(stream), src, (bf16_raw*)dst, n);
    else return VQK_ERR_DTYPE;
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // extern "C"
