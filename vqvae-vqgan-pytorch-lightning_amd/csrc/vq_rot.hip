// The rotation-trick backward of the nearest-code lookup (Fifty et al., "Restructuring Vector Quantization with the Rotation Trick",
// ICLR 2025): the decoder's gradient reaches the encoder through the rotation and rescaling that maps z onto its code q = e[idx],
// both treated as constants.  Per row, with g = dq and everything in fp32:
//   nz = max(|z|, 1e-6)   nq = max(|q|, 1e-6)   zh = z / nz   qh = q / nq   lam = nq / nz   s = zh + qh   r = s / max(|s|, 1e-12)
//   dz = lam (g - 2 r (r.g) + 2 zh (qh.g)) + cz (z - q)
// The forward, the commitment term and the codebook gradient de[idx] += ce (q - z) are those of the straight-through lookup.
// Everything a row needs follows from FIVE dot products zz, qq, zq, zg, qg:
//   |s|^2 = zz / nz^2 + qq / nq^2 + 2 zq / (nz nq)          r.g = (zg / nz + qg / nq) / |s|          qh.g = qg / nq
//   dz = lam g + A z + B q + cz (z - q),      t = 2 lam (r.g) / |s|,   A = (2 lam (qh.g) - t) / nz,   B = -t / nq
// so a row is read ONCE (z, the gathered code row and g stay in registers across the reduction) and dz is written complete; the
// sums are butterflies inside the lanes of a row, no atomics, no LDS.  A row with g = 0 (or dq == NULL) gives A = B = 0 and the last
// operation is fma(cz, z - q, 0): the bits of the straight-through kernels.
// Two kernels:
//   vq_backward_rot_fused_kernel  d == 256 outside deterministic mode: the layout of vq_backward_fused_kernel (vq_filter.hip) -- block
//                                 = 32 rows, 8 lanes per row, every load of the block in one batch -- with the three-step butterfly
//                                 of the five sums between the loads and the stores, and the same CHAINS of vq_lookup.h for de: ONE
//                                 launch, as the straight-through backward.
//   vq_backward_rot_kernel        any 0 < d <= 1024: 2^lg lanes per row, 64 >> lg rows per wave (d <= 8: 32 rows, d = 64: 8 rows --
//                                 a short row does not occupy a wave), 16-byte accesses when d % 4 == 0 and scalar ones otherwise;
//                                 de beside it by the launches of vqk_vq_backward_f32 (vqkd::vq_code_grad: in deterministic mode
//                                 the ordered form, the bits of the straight-through path).
#include <type_traits>
#include "vq_lookup.h"

namespace {

constexpr int RD = 256;                                          // the fused kernel's embedding_dim

// lam, A, B of the header from the row's five sums
__device__ __forceinline__ void rot_coef(float zz, float qq, float zq, float zg, float qg, float& lam, float& a, float& b) {
    const float nz = fmaxf(sqrtf(zz), 1e-6f), nq = fmaxf(sqrtf(qq), 1e-6f);
    const float inz = 1.0f / nz, inq = 1.0f / nq;
    lam = nq * inz;
    const float ss = zz * inz * inz + qq * inq * inq + 2.0f * zq * inz * inq;      // (z = -q: rounding may leave it below zero)
    const float ins = 1.0f / fmaxf(sqrtf(fmaxf(ss, 0.0f)), 1e-12f);
    const float qhg = qg * inq;
    const float t = 2.0f * lam * ((zg * inz + qhg) * ins) * ins;
    a = (2.0f * lam * qhg - t) * inz;
    b = -t * inq;
}

// four columns of the upstream gradient as they are loaded (fp32: 16 bytes, bf16: 8) and as fp32
typedef __attribute__((ext_vector_type(2))) unsigned int rot_u32x2;
template <typename TDQ> using RotRaw = typename std::conditional<sizeof(TDQ) == 4, f32x4, rot_u32x2>::type;
__device__ __forceinline__ f32x4 rot_f32(const f32x4 v) { return v; }
__device__ __forceinline__ f32x4 rot_f32(const rot_u32x2 v) {
    return f32x4{__uint_as_float(v[0] << 16), __uint_as_float(v[0] & 0xffff0000u), __uint_as_float(v[1] << 16), __uint_as_float(v[1] & 0xffff0000u)};
}
// keeps the compiler from holding the fp32 copy of a packed gradient from its first use (the sums) to its second (the stores)
__device__ __forceinline__ void rot_keep_packed(f32x4&) {}
__device__ __forceinline__ void rot_keep_packed(rot_u32x2& v) { asm volatile("" : "+v"(v)); }

// the sum over the 2^lg neighbouring lanes that hold one row (every lane of the wave takes part)
__device__ __forceinline__ float rot_row_sum(float v, int lg) {
    for (int off = (1 << lg) >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// (with the difference tile the LDS admits four blocks per CU: four waves per SIMD are asked for, which holds the bf16 form at 128
// registers without scratch; without the tile every form stays under 128 by itself)
template <typename TDQ, bool HAS_DQ, bool HAS_DE>
__global__ __launch_bounds__(256, HAS_DE ? 4 : 1) void vq_backward_rot_fused_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                                    const int64_t* __restrict__ idx, const TDQ* __restrict__ dq,
                                                                    int64_t n, float cz, float ce, const float* __restrict__ gs,
                                                                    float* __restrict__ dz, float* __restrict__ de) {
    constexpr int ALD = RD + 32;                                 // the difference tile of vq_backward_fused_kernel
    __shared__ __attribute__((aligned(16))) float diff[HAS_DE ? 32 * ALD : 4];
    __shared__ int code_s[32], next_s[32], first_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    if (gs) { const float s = *gs; cz *= s; ce *= s; }
    if (tid < 32) code_s[tid] = n0 + tid < n ? (int)idx[n0 + tid] : -1;
    {
        // thread (row = tid / 8, sub = tid % 8): columns 4 sub + 32 jj .. + 3 -- every load of the block in one batch.  The lanes of a
        // row past n take part in the butterflies on the last row's values and store nothing.
        const int row = tid >> 3, sub = tid & 7;
        const bool live = n0 + row < n;
        const int64_t lrow = live ? n0 + row : n - 1;
        const int64_t o = lrow * RD + sub * 4;
        const float* er = e + (int64_t)idx[lrow] * RD + sub * 4;
        f32x4 zv[8], ev[8];
        RotRaw<TDQ> gr[HAS_DQ ? 8 : 1];                         // a bf16 gradient stays packed until its two uses: 16 registers fewer
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            zv[jj] = *reinterpret_cast<const f32x4*>(z + o + 32 * jj);
            ev[jj] = *reinterpret_cast<const f32x4*>(er + 32 * jj);
            if constexpr (HAS_DQ) gr[jj] = *reinterpret_cast<const RotRaw<TDQ>*>(dq + o + 32 * jj);
        }
        float lam = 0.f, a = 0.f, b = 0.f;
        if constexpr (HAS_DQ) {
            float zz = 0.f, qq = 0.f, zq = 0.f, zg = 0.f, qg = 0.f;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const f32x4 g = rot_f32(gr[jj]);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    zz = __fmaf_rn(zv[jj][t], zv[jj][t], zz); qq = __fmaf_rn(ev[jj][t], ev[jj][t], qq);
                    zq = __fmaf_rn(zv[jj][t], ev[jj][t], zq); zg = __fmaf_rn(zv[jj][t], g[t], zg);
                    qg = __fmaf_rn(ev[jj][t], g[t], qg);
                }
            }
            zz = rot_row_sum(zz, 3); qq = rot_row_sum(qq, 3); zq = rot_row_sum(zq, 3); zg = rot_row_sum(zg, 3); qg = rot_row_sum(qg, 3);
            rot_coef(zz, qq, zq, zg, qg, lam, a, b);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) rot_keep_packed(gr[jj]);
        }
        if (live) {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                f32x4 out, df, g = {0.f, 0.f, 0.f, 0.f};
                if constexpr (HAS_DQ) g = rot_f32(gr[jj]);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float rot = HAS_DQ ? lam * g[t] + a * zv[jj][t] + b * ev[jj][t] : 0.0f;
                    out[t] = __fmaf_rn(cz, zv[jj][t] - ev[jj][t], rot);
                    df[t] = ev[jj][t] - zv[jj][t];
                }
                *reinterpret_cast<f32x4*>(dz + o + 32 * jj) = out;
                if constexpr (HAS_DE) *reinterpret_cast<f32x4*>(diff + row * ALD + sub * 4 + 32 * jj) = df;
            }
        }
    }
    if constexpr (!HAS_DE) return;
    __syncthreads();
    if (tid < 32) lk_build_chains(code_s, first_s, next_s, tid);
    __syncthreads();
    lk_chain_rows(diff, ALD, code_s, first_s, next_s, lane, wave, [&](int code, const float (&acc)[4], int) {
        float* drow = de + (int64_t)code * RD;
#pragma unroll
        for (int t = 0; t < 4; ++t) atomicAdd(drow + t * 64 + lane, ce * acc[t]);
    });
}

// dz of any d <= 1024.  Lane (row = lane >> lg, sub = lane & (2^lg - 1)) of a wave holds the columns VEC (sub + 2^lg j) .. + VEC - 1,
// j < NJ (CALLER: 2^lg NJ VEC >= d, d % VEC == 0); block = 4 waves = 4 (64 >> lg) rows, grid-stride over the row groups.
template <typename TDQ, bool HAS_DQ, int VEC>
__global__ __launch_bounds__(256) void vq_backward_rot_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                              const int64_t* __restrict__ idx, const TDQ* __restrict__ dq, int64_t n,
                                                              int d, int lg, float cz, const float* __restrict__ gs,
                                                              float* __restrict__ dz) {
    constexpr int NJ = VEC == 4 ? 4 : 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lanes = 1 << lg, rpw = 64 >> lg, sub = lane & (lanes - 1);
    const int nj = (d / VEC + lanes - 1) >> lg;                   // chunks a lane holds (wave-uniform)
    if (gs) cz *= *gs;
    for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * rpw; r0 < n; r0 += (int64_t)gridDim.x * 4 * rpw) {     // wave-uniform
        const int64_t row = r0 + (lane >> lg);
        const bool live = row < n;
        const float* zr = z + row * d;
        const float* er = live ? e + idx[row] * d : e;
        float zv[NJ][VEC], ev[NJ][VEC], g[NJ][VEC];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j >= nj) break;
            const int c = (sub + lanes * j) * VEC;
            const bool on = live && c < d;
            if constexpr (VEC == 4) {
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                const f32x4 z4 = on ? *reinterpret_cast<const f32x4*>(zr + c) : zero;
                const f32x4 e4 = on ? *reinterpret_cast<const f32x4*>(er + c) : zero;
                const f32x4 g4 = on ? lk_load_dq4<TDQ, HAS_DQ>(dq + row * d + c) : zero;
#pragma unroll
                for (int t = 0; t < 4; ++t) { zv[j][t] = z4[t]; ev[j][t] = e4[t]; g[j][t] = g4[t]; }
            } else {
                zv[j][0] = on ? zr[c] : 0.f;
                ev[j][0] = on ? er[c] : 0.f;
                g[j][0] = (HAS_DQ && on) ? Elem<TDQ>::ld(dq + row * d + c) : 0.f;
            }
        }
        float lam = 0.f, a = 0.f, b = 0.f;
        if constexpr (HAS_DQ) {
            float zz = 0.f, qq = 0.f, zq = 0.f, zg = 0.f, qg = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (j >= nj) break;
#pragma unroll
                for (int t = 0; t < VEC; ++t) {
                    zz = __fmaf_rn(zv[j][t], zv[j][t], zz); qq = __fmaf_rn(ev[j][t], ev[j][t], qq);
                    zq = __fmaf_rn(zv[j][t], ev[j][t], zq); zg = __fmaf_rn(zv[j][t], g[j][t], zg);
                    qg = __fmaf_rn(ev[j][t], g[j][t], qg);
                }
            }
            zz = rot_row_sum(zz, lg); qq = rot_row_sum(qq, lg); zq = rot_row_sum(zq, lg); zg = rot_row_sum(zg, lg); qg = rot_row_sum(qg, lg);
            rot_coef(zz, qq, zq, zg, qg, lam, a, b);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j >= nj) break;
            const int c = (sub + lanes * j) * VEC;
            if (!(live && c < d)) continue;
            float out[VEC];
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                const float rot = HAS_DQ ? lam * g[j][t] + a * zv[j][t] + b * ev[j][t] : 0.0f;
                out[t] = __fmaf_rn(cz, zv[j][t] - ev[j][t], rot);
            }
            if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(dz + row * d + c) = f32x4{out[0], out[1], out[2], out[3]};
            else dz[row * d + c] = out[0];
        }
    }
}

}  // namespace

extern "C" {

int vqk_vq_backward_rot_f32(const float* z, const float* e, const int64_t* idx, const void* dq, int dq_dtype, int64_t n, int k, int d,
                            float cz, float ce, const float* gscale_dev, float* dz, float* de, void* stream) {
    VQK_REQUIRE(z && e && idx && dz, VQK_ERR_ARG);
    VQK_REQUIRE(n >= 0 && k > 0 && d > 0 && d <= 1024, VQK_ERR_SHAPE);
    VQK_REQUIRE(dq_dtype == VQK_F32 || dq_dtype == VQK_BF16, VQK_ERR_DTYPE);
    if (n == 0) return VQK_OK;
    hipStream_t st = vqk_stream(stream);
    const bool wide = (d % 4) == 0 && vqk_aligned16(z) && vqk_aligned16(e) && vqk_aligned16(dz) && (!dq || vqk_aligned16(dq));
    if (d == RD && wide && !vqkd::det_state().on) {
        const dim3 grid((unsigned)((n + 31) / 32));
#define VQR(T, Q, E) hipLaunchKernelGGL((vq_backward_rot_fused_kernel<T, Q, (E) != 0>), grid, dim3(256), 0, st, z, e, idx, (const T*)dq, n, \
                                       cz, ce, gscale_dev, dz, de)
        LK_DISPATCH_DQ_DE(VQR, dq, dq_dtype, de ? 1 : 0);
#undef VQR
        VQK_CHECK_LAUNCH();
        return VQK_OK;
    }
    // lanes per row: the fewest that leave a lane at most two 16-byte chunks (four scalar columns), at least two, a whole wave at most
    const int vec = wide ? 4 : 1, want = (d / vec + (wide ? 1 : 3)) / (wide ? 2 : 4);
    int lg = 1;
    while (lg < 6 && (1 << lg) < want) ++lg;
    const dim3 grid((unsigned)vqk_grid_1d(n, 4 * (64 >> lg)));
#define VQR(T, Q, V) hipLaunchKernelGGL((vq_backward_rot_kernel<T, Q, V>), grid, dim3(256), 0, st, z, e, idx, (const T*)dq, n, d, lg, cz, \
                                       gscale_dev, dz)
    if (!dq) { if (wide) VQR(float, false, 4); else VQR(float, false, 1); }
    else if (dq_dtype == VQK_F32) { if (wide) VQR(float, true, 4); else VQR(float, true, 1); }
    else { if (wide) VQR(bf16_raw, true, 4); else VQR(bf16_raw, true, 1); }
#undef VQR
    if (de) return vqkd::vq_code_grad(z, e, idx, n, k, d, ce, gscale_dev, de, stream);
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // extern "C"
