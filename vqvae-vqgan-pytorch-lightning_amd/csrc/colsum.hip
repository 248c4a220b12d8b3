// Column sums of [rows][c] tensors for gfx950 (vqk_colsum, vqk_colsum_lead): the bias gradients of the convs.  Atomic form and,
// in deterministic mode (vqk_set_deterministic), a two-stage form that adds a fixed set of rows in a fixed order.
#include "common.h"

namespace {

// out[c] += sum_rows x[row][c].  c*sizeof(T) a multiple of 16 (VEC): a thread owns one 16-byte channel slot and strides
// over rows (the GroupNorm kernels' mapping); otherwise one column per thread.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, int64_t rows, int c, int64_t rows_per_block,
                                                     float* __restrict__ out, int c_out, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sh = reinterpret_cast<float*>(smem);            // [c]
    for (int i = threadIdx.x; i < c; i += 256) sh[i] = 0.f;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    if (VEC) {
        constexpr int V = Vec16<T>::N;
        const int vpp = c / V;                              // slots per row
        if (vpp <= 256) {
            const int slot = threadIdx.x % vpp, rlane = threadIdx.x / vpp, rstep = 256 / vpp;
            if (rlane < rstep) {
                float a[V];
#pragma unroll
                for (int i = 0; i < V; ++i) a[i] = 0.f;
#pragma unroll 4
                for (int64_t r = r0 + rlane; r < r1; r += rstep) {
                    float v[V];
                    Vec16<T>::load(x + r * c + slot * V, v);
#pragma unroll
                    for (int i = 0; i < V; ++i) a[i] += v[i];
                }
#pragma unroll
                for (int i = 0; i < V; ++i) atomicAdd(&sh[slot * V + i], a[i]);
            }
        } else {                                            // wide rows (the [N, K] matrices of the quantizers)
            for (int slot = threadIdx.x; slot < vpp; slot += 256) {
                float a[V];
#pragma unroll
                for (int i = 0; i < V; ++i) a[i] = 0.f;
#pragma unroll 4
                for (int64_t r = r0; r < r1; ++r) {
                    float v[V];
                    Vec16<T>::load(x + r * c + slot * V, v);
#pragma unroll
                    for (int i = 0; i < V; ++i) a[i] += v[i];
                }
#pragma unroll
                for (int i = 0; i < V; ++i) sh[slot * V + i] = a[i];
            }
        }
    } else {
        for (int col = threadIdx.x & 63; col < c; col += 64) {
            float a = 0.f;
            for (int64_t r = r0 + (threadIdx.x >> 6); r < r1; r += 4) a += Elem<T>::ld(x + r * c + col);
            atomicAdd(&sh[col], a);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < c_out; i += 256) atomicAdd(out + i, sh[i] * scale);     // c_out <= c: the columns `out` has room for
}

// deterministic column sums, round 4 (the first form -- one thread per column, 2-byte loads, one reducing block -- took 1.47 ms
// per step for the seven bias gradients: 190 + 80 us for the 537-MB gradient at 128 ch @256^2).  Stage 1: a thread owns one
// 16-byte channel slot and walks rows r0 + rlane, + rstep, ... of its block (coalesced 16-byte loads, a FIXED set of rows in
// a fixed order), the row lanes of a slot are added in lane order through LDS; block partials go to the workspace.  Stage 2:
// a block owns 8 columns, 32 lanes add partial rows lane, lane + 32, ..., thread `col` adds the 32 lane sums in lane order.
template <typename T>
__global__ __launch_bounds__(256) void colsum_det_kernel(const T* __restrict__ x, int64_t rows, int c, int64_t rows_per_block,
                                                         float* __restrict__ part) {
    constexpr int V = Vec16<T>::N;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sh = reinterpret_cast<float*>(smem);                  // [rstep][c]
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    const int vpp = c / V;                                       // slots per row (<= 256: the caller checks)
    const int slot = threadIdx.x % vpp, rlane = threadIdx.x / vpp, rstep = 256 / vpp;
    if (rlane < rstep) {
        float a[V];
#pragma unroll
        for (int i = 0; i < V; ++i) a[i] = 0.f;
#pragma unroll 4
        for (int64_t r = r0 + rlane; r < r1; r += rstep) {
            float v[V];
            Vec16<T>::load(x + r * c + slot * V, v);
#pragma unroll
            for (int i = 0; i < V; ++i) a[i] += v[i];
        }
#pragma unroll
        for (int i = 0; i < V; ++i) sh[rlane * c + slot * V + i] = a[i];
    }
    __syncthreads();
    for (int col = threadIdx.x; col < c; col += 256) {
        float t = 0.f;
        for (int k = 0; k < rstep; ++k) t += sh[k * c + col];
        part[(int64_t)blockIdx.x * c + col] = t;
    }
}
// (scalar fallback: channel counts that are no whole 16-byte slots, or more than 256 slots per row)
template <typename T>
__global__ __launch_bounds__(256) void colsum_det_scalar_kernel(const T* __restrict__ x, int64_t rows, int c, int64_t rows_per_block,
                                                                float* __restrict__ part) {
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    for (int col = threadIdx.x; col < c; col += 256) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int64_t r = r0;
        for (; r + 4 <= r1; r += 4) {
            a0 += Elem<T>::ld(x + r * c + col); a1 += Elem<T>::ld(x + (r + 1) * c + col);
            a2 += Elem<T>::ld(x + (r + 2) * c + col); a3 += Elem<T>::ld(x + (r + 3) * c + col);
        }
        for (; r < r1; ++r) a0 += Elem<T>::ld(x + r * c + col);
        part[(int64_t)blockIdx.x * c + col] = (a0 + a1) + (a2 + a3);
    }
}
__global__ __launch_bounds__(256) void colsum_det_reduce_kernel(const float* __restrict__ part, int blocks, int c, float* __restrict__ out,
                                                                int c_out, float scale) {
    __shared__ float lane_sum[32][8];
    const int col = (int)blockIdx.x * 8 + (threadIdx.x & 7), rl = threadIdx.x >> 3;
    float s = 0.f;
    if (col < c)
        for (int b = rl; b < blocks; b += 32) s += part[(int64_t)b * c + col];
    lane_sum[rl][threadIdx.x & 7] = s;
    __syncthreads();
    if (threadIdx.x < 8 && col < c_out) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 32; ++k) t += lane_sum[k][threadIdx.x];
        out[col] += t * scale;
    }
}

}  // namespace

extern "C" {

int vqk_colsum(int dtype, const void* x, int64_t rows, int c, float* out, void* stream) {
    return vqk_colsum_lead(dtype, x, rows, c, c, 1.0f, out, stream);
}

int vqk_colsum_lead(int dtype, const void* x, int64_t rows, int c, int c_out, float scale, float* out, void* stream) {
    VQK_REQUIRE(x && out, VQK_ERR_ARG);
    VQK_REQUIRE(rows >= 0 && c > 0 && c <= 8192 && c_out > 0 && c_out <= c, VQK_ERR_SHAPE);
    VQK_REQUIRE(dtype == VQK_F32 || dtype == VQK_BF16, VQK_ERR_DTYPE);
    if (rows == 0) return VQK_OK;
    const vqkd::DetState& det = vqkd::det_state();
    if (det.on) {
        int64_t nb = (rows + 63) / 64; if (nb > 512) nb = 512;
        while (nb > 1 && nb * c * 4 > det.bytes) nb >>= 1;
        VQK_REQUIRE(det.ws && nb * c * 4 <= det.bytes, VQK_ERR_ARG);
        const int64_t rb = (rows + nb - 1) / nb;
        nb = (rows + rb - 1) / rb;
        hipStream_t sd = vqk_stream(stream);
        const int vd = dtype == VQK_F32 ? 4 : 8;
        const bool vecd = (c % vd) == 0 && c / vd <= 256 && (256 % (c / vd)) == 0 && vqk_aligned16(x);
        if (vecd) {
            const size_t ldsd = (size_t)(256 / (c / vd)) * c * 4;
            if (dtype == VQK_F32) hipLaunchKernelGGL(colsum_det_kernel<float>, dim3((unsigned)nb), dim3(256), ldsd, sd, (const float*)x, rows, c, rb, det.ws);
            else hipLaunchKernelGGL(colsum_det_kernel<bf16_raw>, dim3((unsigned)nb), dim3(256), ldsd, sd, (const bf16_raw*)x, rows, c, rb, det.ws);
        } else {
            if (dtype == VQK_F32) hipLaunchKernelGGL(colsum_det_scalar_kernel<float>, dim3((unsigned)nb), dim3(256), 0, sd, (const float*)x, rows, c, rb, det.ws);
            else hipLaunchKernelGGL(colsum_det_scalar_kernel<bf16_raw>, dim3((unsigned)nb), dim3(256), 0, sd, (const bf16_raw*)x, rows, c, rb, det.ws);
        }
        hipLaunchKernelGGL(colsum_det_reduce_kernel, dim3((unsigned)((c + 7) / 8)), dim3(256), 0, sd, (const float*)det.ws, (int)nb, c, out, c_out, scale);
        VQK_CHECK_LAUNCH();
        return VQK_OK;
    }
    const int v = dtype == VQK_F32 ? 4 : 8;
    const bool vec = (c % v) == 0 && vqk_aligned16(x);
    int64_t blocks = (rows + 63) / 64; if (blocks > 1024) blocks = 1024;
    const int64_t rpb = (rows + blocks - 1) / blocks;
    blocks = (rows + rpb - 1) / rpb;
    const dim3 grid((unsigned)blocks);
    const size_t lds = (size_t)c * 4;
    hipStream_t st = vqk_stream(stream);
    if (dtype == VQK_F32) {
        if (vec) hipLaunchKernelGGL((colsum_kernel<float, true>), grid, dim3(256), lds, st, (const float*)x, rows, c, rpb, out, c_out, scale);
        else hipLaunchKernelGGL((colsum_kernel<float, false>), grid, dim3(256), lds, st, (const float*)x, rows, c, rpb, out, c_out, scale);
    } else {
        if (vec) hipLaunchKernelGGL((colsum_kernel<bf16_raw, true>), grid, dim3(256), lds, st, (const bf16_raw*)x, rows, c, rpb, out, c_out, scale);
        else hipLaunchKernelGGL((colsum_kernel<bf16_raw, false>), grid, dim3(256), lds, st, (const bf16_raw*)x, rows, c, rpb, out, c_out, scale);
    }
    VQK_CHECK_LAUNCH();
    return VQK_OK;
}

}  // extern "C"
