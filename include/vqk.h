/* vqk -- C-ABI of the MI355X (gfx950) VQ-VAE / VQ-GAN train-step kernels.
 *
 * Boundary rules:
 *   - plain C: raw device pointers + sizes + scalars, no torch types;
 *   - the CALLER owns every buffer (outputs, workspaces); nothing is allocated, nothing is
 *     synchronised, and a call's RESULT depends on its arguments only.  The library reads no environment variable.
 *     What state it does keep, all of it launch POLICY (which kernel / grid / accumulation order serves a call), and its scope:
 *       THREAD-LOCAL (applies to the launches the calling host thread issues afterwards; another thread -- e.g. autograd's
 *       backward worker -- arms its own): vqk_set_deterministic (+ its workspace), vqk_set_scratch, vqk_set_tile_queue, vqk_conv_set_block_caps,
 *       vqk_conv_set_variant.  These act at LAUNCH (= graph capture) time: a hipGraph captured under them replays the
 *       captured kernels and workspace pointers from any thread, whatever that thread's own settings are
 *       (tests/test_gpu_deterministic.py::test_graph_captured_on_one_thread_replays_identically_from_another);
 *       PROCESS-WIDE: the tuning slots of vqk_set_tuning (grid sizes, kernel-choice thresholds: never the arithmetic of a
 *       kernel, except where a slot's description says it selects a differently rounding kernel);
 *   - every launch goes to the `stream` argument (a hipStream_t passed as void*; NULL = the
 *     null stream);
 *   - return value: 0 = ok, negative = vqk_status (see vqk_status_str).  There is NO fallback
 *     path: an unsupported shape/dtype is an error, never a silent detour.
 *
 * Layouts: activations are NHWC (pixel-major, channels contiguous); conv weights are
 * [Cout][kh][kw][Cin] ("KRSC" = the physical layout of a channels_last OIHW torch tensor).
 * dtype codes: VQK_F32 = 0 (parity mode), VQK_BF16 = 1 (throughput mode, fp32 accumulate).
 *
 * What each entry point replaces in the reference (paths relative to the reference checkout):
 *   vqk_bias_act / vqk_upfirdn2d : the reference's own native plugin ABI,
 *        vqvae/modules/loss/stylegan2_discriminator/utils/ops/bias_act.cpp:32-90 and
 *        .../upfirdn2d.cpp:16-94 (pybind functions `bias_act`, `upfirdn2d`);
 *   everything else: ATen/cuDNN calls made from
 *        vqvae/modules/autoencoder.py:25-39 (GroupNorm), :63-77 (ResBlock), :89-91, :104-106,
 *        vqvae/modules/vector_quantizers.py:23-61, :128-180, :290-356 (quantizers),
 *        vqvae/model.py:272 (MSE), :428 (AdamW).
 */
#ifndef VQK_H_
#define VQK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQK_F32 0
#define VQK_BF16 1

enum vqk_status {
    VQK_OK = 0,
    VQK_ERR_SHAPE = -1,       /* unsupported / inconsistent shape */
    VQK_ERR_DTYPE = -2,       /* unsupported dtype code */
    VQK_ERR_ALIGN = -3,       /* pointer not 16-byte aligned */
    VQK_ERR_LAUNCH = -4,      /* hipGetLastError() after launch */
    VQK_ERR_ARG = -5,         /* NULL / out-of-range argument */
    VQK_ERR_WORKSPACE = -6    /* workspace too small */
};

const char* vqk_status_str(int status);
int vqk_version(void);
/* name of the code-object architecture this library was built for ("gfx950") */
const char* vqk_arch(void);

/* ---------------------------------------------------------------- vector quantizer ---------
 * vector_quantizers.py:33-44 / :337-343.  z[N][D], e[K][D] fp32 row-major, D % 8 == 0.
 * (The cosine quantizer further down applies this arithmetic, assoc 0, to l2-normalised rows: fused for D in {8, 16, 32, 64} and
 * K % 32 == 0, staged on these functions for every other shape.)
 * assoc 0: d = (|z|^2 + |e|^2) - 2 z.e (Standard/EMA); assoc 1: d = (|z|^2 - 2 z.e) + |e|^2 (Entropy).
 * Products are exact fp32 (v_mfma_f32_32x32x2_f32), first minimum wins. */
int vqk_row_sqnorm_f32(const float* x, int64_t rows, int d, float* out, void* stream);
int vqk_vq_assign_f32(const float* z, const float* e, const float* z2, const float* e2,
                      int64_t n, int k, int d, int assoc, int64_t* idx, void* stream);
/* vqk_vq_assign_f32 with the same result (bit-identical indices) computed as a bf16-MFMA candidate filter + an exact fp32
 * re-rank of the candidates (csrc/vq_filter.hip states the error bound that keeps the exact winner inside the candidate
 * set); d == 256, k % 32 == 0.  ws: >= vqk_vq_filter_ws_bytes(k, d) bytes of device scratch (the bf16 codebook and the
 * per-code filter margins, rebuilt by every call).  VQK_ERR_SHAPE when not served (nothing launched). */
int64_t vqk_vq_filter_ws_bytes(int k, int d);
int vqk_vq_assign_filtered_f32(const float* z, const float* e, const float* z2, const float* e2, int64_t n, int k, int d,
                               int assoc, int64_t* idx, void* ws, int64_t ws_bytes, void* stream);
/* The quantizer FORWARD as one kernel (vector_quantizers.py:37-56): the filtered assignment above with |z|^2 computed in the
 * kernel (same bits as vqk_row_sqnorm_f32) and the gather fused into its epilogue -- idx[N]; optionally q = e[idx] as fp32
 * (q) and / or bf16 (q_lo), sse[0] += sum (q - z)^2, hist[idx] += 1 (sse / hist pre-zeroed by the caller).
 * ws = what vqk_vq_prepare_f32 built from THIS codebook (bf16 fragment-major copy, |e|^2, filter margins, max |e|^2:
 * vqk_vq_filter_ws_bytes(k, d) bytes): call it once per codebook CHANGE (optimizer step, EMA update), not per step.
 * d == 256, k % 32 == 0 (VQK_ERR_SHAPE otherwise, nothing launched). */
int vqk_vq_prepare_f32(const float* e, int k, int d, void* ws, int64_t ws_bytes, void* stream);
int vqk_vq_forward_f32(const float* z, const float* e, const void* ws, int64_t ws_bytes, int64_t n, int k, int d, int assoc,
                       int64_t* idx, float* q /* optional */, void* q_lo /* optional */, float* sse /* optional */,
                       int32_t* hist /* optional */, void* stream);
/* Same search, additionally writing the full fp32 distance matrix dmat[N][K] (Entropy quantizer).  d == 256, N % 128 == 0, K % 32 == 0
 * and a stream scratch of >= 5 * parts * N * 4 bytes (vqk_set_scratch; parts <= 16): the code tiles go through LDS once per 128 rows
 * (vq_assign_lds_kernel, blocks = N/128 x parts) and a second small launch folds the parts' (min, argmin) and log-sum-exp states;
 * otherwise every wave streams the codebook itself.  Same distances and indices, bit for bit, either way. */
int vqk_vq_distances_f32(const float* z, const float* e, const float* z2, const float* e2,
                         int64_t n, int k, int d, int assoc, int64_t* idx, float* dmat, void* stream);
/* vqk_vq_distances_f32 (d == 256) that also leaves the softmax row statistics of a = -d / temperature: lse[N], hrow[N] (sample
 * entropies) and hsum[0] += sum_i h_i (pre-zeroed) -- an online log-sum-exp under the distance MFMAs; follow it with
 * vqk_entropy_forward_presummed_f32 (column means + finalize) instead of vqk_entropy_forward_f32. */
int vqk_vq_distances_stats_f32(const float* z, const float* e, const float* z2, const float* e2, int64_t n, int k, int d,
                               int assoc, int64_t* idx, float* dmat, float temperature, float* lse, float* hrow, float* hsum,
                               void* stream);
int vqk_entropy_forward_presummed_f32(const float* dmat, int64_t n, int k, float temperature, const float* lse, float* psum,
                                      float* u, float* avg_term, void* stream);
/* Entropy loss on dmat (vector_quantizers.py:296-328, 'softmax' type): per row lse[N], hrow[N] (sample entropies),
 * hsum[0] += sum_i h_i, psum[K] += sum_i p_ik, u[K] = log(pbar+1e-5) + pbar/(pbar+1e-5), avg_term[0] += sum_k pbar
 * log(pbar+1e-5) (pbar = psum/N).  hsum, psum, avg_term pre-zeroed.  loss_ent = ratio * (hsum/N + avg_term). */
int vqk_entropy_forward_f32(const float* dmat, int64_t n, int k, float temperature, float* lse, float* hrow,
                            float* hsum, float* psum, float* u, float* avg_term, void* stream);
/* In place dmat <- dL_ent/dd (scaled by *gscale_dev): the cotangent that the two GEMMs turn into dz and dE. */
int vqk_entropy_backward_f32(float* dmat, const float* lse, const float* hrow, const float* u, int64_t n, int k,
                             float temperature, float ratio, const float* gscale_dev, void* stream);
/* The same cotangent as TWO bf16 matrices hi, lo [N][K] (hi = bf16(dd), lo = bf16(dd - hi); dmat is left untouched; K % 4 == 0):
 * the operands of split-product GEMMs on the bf16 MFMA kernels (dd E ~ hi E_hi + hi E_lo + lo E_hi, relative error ~2^-16) where the
 * reference multiplies in fp32 (vector_quantizers.py:296-356 differentiated; throughput mode only). */
int vqk_entropy_backward_split_f32(const float* dmat, const float* lse, const float* hrow, const float* u, int64_t n, int k,
                                   float temperature, float ratio, const float* gscale_dev, void* hi, void* lo, void* stream);
/* ent_loss_type == 'argmax' (vector_quantizers.py:311-315): the targets are one_hot(argmax_k a) with the gradient of p
 * (straight-through).  idx = the assignment of vqk_vq_distances_f32 (argmax a == argmin d, first wins), hist = its code
 * histogram (vqk_vq_gather_f32).  Forward: lse / hrow as above, ssum += sum_i (lse_i - a_i[idx_i]), mbuf[k] scratch,
 * u / avg_term from m = hist / N;  loss_ent = ratio * (ssum / N + avg_term).  Backward overwrites dmat with dL/dd. */
int vqk_entropy_argmax_forward_f32(const float* dmat, const int64_t* idx, const int32_t* hist, int64_t n, int k,
                                   float temperature, float* lse, float* hrow, float* hsum, float* ssum, float* mbuf,
                                   float* u, float* avg_term, void* stream);
int vqk_entropy_argmax_backward_f32(float* dmat, const int64_t* idx, const float* lse, const float* hrow, const float* u,
                                    int64_t n, int k, float temperature, float ratio, const float* gscale_dev,
                                    void* stream);
/* out[r][c] += a * scale[r] * m[r][c] */
int vqk_row_scale_add_f32(float* out, const float* m, const float* scale, int64_t rows, int c, float a, void* stream);
/* Gumbel-softmax rows (vector_quantizers.py:232-243): y = softmax((logits - log(noise))/tau) [hard: one-hot of its
 * argmax] written as `dtype`, idx = argmax y, klsum[0] += sum_i sum_n qy log(qy*K + 1e-10), qy = softmax(logits).
 * noise ~ Exp(1) is drawn by the caller (the reference's F.gumbel_softmax draws the same tensor first). */
int vqk_gumbel_forward(int dtype, const float* logits, const float* noise, int64_t n, int k, float tau, int hard,
                       void* y, int64_t* idx, float* klsum, int32_t* hist /* optional */,
                       const float* sched_dev /* optional */, void* stream);
/* dlogits = y (dy - <y,dy>)/tau + s*(kl_cost/n) qy (r - <qy,r>), s = *gscale_dev (soft sample path).
 * sched_dev (both calls, optional): device floats {tau, kl_cost} that REPLACE the scalar arguments -- the reference schedules
 * both per step (vqvae/model.py:218-225); reading them on the device lets a captured hipGraph follow the schedule. */
int vqk_gumbel_backward(int dtype, const float* logits, const float* noise, const void* dy, int64_t n, int k,
                        float tau, float kl_cost, const float* gscale_dev, float* dlogits,
                        const float* sched_dev /* optional */, void* stream);
/* q = e[idx] (written as fp32 and, if q_lo != NULL, also as bf16), sse[0] += sum (q - z)^2,
 * hist[idx] += 1 (int32, optional).  sse must be zeroed by the caller. */
int vqk_vq_gather_f32(const float* z, const float* e, const int64_t* idx, int64_t n, int k, int d,
                      float* q, void* q_lo, float* sse, int32_t* hist, void* stream);
/* dz = dq + s*cz * (z - q)   ;   de[idx] += s*ce * (q - z)   (de optional, pre-zeroed by caller)
 * s = *gscale_dev (a device scalar: the upstream gradient of the loss; NULL = 1), dq optional (NULL = 0),
 * fp32 or bf16 (dq_dtype).  vector_quantizers.py:52-56 differentiated. */
int vqk_vq_backward_f32(const float* z, const float* e, const int64_t* idx, const void* dq, int dq_dtype,
                        int64_t n, int k, int d, float cz, float ce, const float* gscale_dev, float* dz, float* de,
                        void* stream);
/* vqk_vq_backward_f32 as ONE kernel (d == 256): the rows of a 32-row block that share a code are summed in LDS, one
 * coalesced fp32 atomic row per distinct code and block goes to de (arrival order: not for deterministic mode). */
int vqk_vq_backward_fused_f32(const float* z, const float* e, const int64_t* idx, const void* dq, int dq_dtype,
                              int64_t n, int k, int d, float cz, float ce, const float* gscale_dev, float* dz, float* de,
                              void* stream);
/* vqk_vq_backward_f32 with the rotation-trick gradient (csrc/vq_rot.hip; Fifty et al., ICLR 2025) in place of the straight-through
 * copy: per row, nz = max(|z|, 1e-6), nq = max(|q|, 1e-6), zh = z / nz, qh = q / nq, lam = nq / nz, r = (zh + qh) / max(|zh + qh|, 1e-12),
 *   dz = lam * (dq - 2 r (r . dq) + 2 zh (qh . dq)) + s*cz * (z - q)   ;   de[idx] += s*ce * (q - z)   (as vqk_vq_backward_f32)
 * in fp32 from five dot products per row, one pass over z, q and dq.  Served: 0 < d <= 1024 (VQK_ERR_SHAPE otherwise), any alignment
 * (16-byte accesses when d % 4 == 0 and z, e, dq, dz are 16-byte aligned); n == 0 launches nothing.  dq == NULL or a row with
 * dq = 0: the bits of vqk_vq_backward_f32's dz.  de: d == 256 outside deterministic mode in the same launch (one atomic row per
 * distinct code and 32-row block, as vqk_vq_backward_fused_f32), otherwise by the launches of vqk_vq_backward_f32 -- in
 * deterministic mode its ordered form, the same bits.  A zero z, a zero code and z = -q give finite rows. */
int vqk_vq_backward_rot_f32(const float* z, const float* e, const int64_t* idx, const void* dq, int dq_dtype,
                            int64_t n, int k, int d, float cz, float ce, const float* gscale_dev, float* dz, float* de,
                            void* stream);
/* ---------------------------------------------------------------- finite scalar quantizer ---------
 * Mentzer et al. 2023 (csrc/fsq.hip).  z[N][D] fp32 rows, w_in[d][D], b_in[d], w_out[D][d], b_out[D] fp32; levels: d ints on the HOST
 * (they travel by value in the launch arguments).  u = W_in z + b_in; half_l = (L - 1)(1 + 1e-3) / 2, offset = 0.5 for an even L, shift =
 * atanh(offset / half_l); bounded = tanh(u + shift) half_l - offset; r = rint(bounded); idx = sum_j (r_j + L_j / 2) basis_j with basis =
 * (1, L_1, L_1 L_2, ...); q = W_out (r / (L / 2)) + b_out.  Served: 4 <= D <= 1024, D % 4 == 0, 1 <= d <= 8, every level >= 2, prod(levels)
 * < 2^31 (VQK_ERR_SHAPE otherwise); z, q, q_lo, dq, dz and ws 16-byte aligned, the parameters need no alignment.  No call allocates
 * or synchronises.
 * forward: ONE launch; idx[N]; u[N][d] (optional: what the backward needs); q as fp32 (q) and / or bf16 (q_lo), both optional;
 * hist[idx] += 1 (int32 [prod(levels)], optional, pre-zeroed by the caller). */
int vqk_fsq_forward(const float* z, const float* w_in, const float* b_in, const float* w_out, const float* b_out, int64_t n,
                    int dm, int d, const int32_t* levels, int64_t* idx, float* u /* optional */, float* q /* optional */,
                    void* q_lo /* optional */, int32_t* hist /* optional */, void* stream);
/* idx[N] -> q (fp32 and / or bf16): the digits by integer arithmetic on the index -- no table, an index outside [0, prod(levels)) reads
 * nothing out of bounds -- through the forward's own device function: the same bits of q for the same index. */
int vqk_fsq_decode(const int64_t* idx, const float* w_out, const float* b_out, int64_t n, int dm, int d, const int32_t* levels,
                   float* q /* optional */, void* q_lo /* optional */, void* stream);
/* Straight-through backward from dq (fp32 or bf16: dq_dtype) and the forward's u: dz[N][D] and the four parameter gradients
 * (accumulate = 1: added to what the targets hold).  The parameter gradients are sums over the N rows in an order that depends on
 * (n, D, d) only -- registers per lane, the waves of a block through LDS in wave order, one slab per block in ws, a second launch
 * that adds the slabs in an order fixed by their count: no atomics, the same bits every run.  ws: >= vqk_fsq_backward_ws_bytes(n, D, d) bytes
 * (VQK_ERR_WORKSPACE); that function returns VQK_ERR_SHAPE for an unserved (D, d). */
int64_t vqk_fsq_backward_ws_bytes(int64_t n, int dm, int d);
int vqk_fsq_backward(const float* z, const float* u, const void* dq, int dq_dtype, const float* w_in, const float* w_out, int64_t n,
                     int dm, int d, const int32_t* levels, float* dz, float* dw_in, float* db_in, float* dw_out, float* db_out,
                     int accumulate, void* ws, int64_t ws_bytes, void* stream);
/* ---------------------------------------------------------------- lookup-free quantizer ---------
 * Yu et al. 2023 (MAGVIT-v2) / Open-MAGVIT2 (csrc/lfq.hip).  z[N][D] fp32 rows, w_in[d][D], b_in[d], w_out[D][d], b_out[D] fp32, d = bits.
 * u = W_in z + b_in; c_j = +1 if u_j > 0 else -1 (a zero or a NaN gives -1); idx = sum_j [u_j > 0] 2^j; q = W_out c + b_out.
 * commit = sum (u - c)^2 / (N d); p_nj = sigmoid(a u_nj), a = 4 / tau; H_sample = sum_nj h(p_nj) / N (h = binary entropy: exactly the
 * entropy of softmax(2 u.c_k / tau) over the 2^d sign codes); the bits are split into ceil(d / g) groups of g consecutive bits (the last
 * may be shorter), P_n^s(m) = prod_i (bit_i(m) ? p : 1 - p) over the bits of group s, Pbar^s = mean_n P_n^s, H_batch = sum_s -sum_m
 * Pbar^s(m) log(Pbar^s(m) + 1e-10); loss = beta commit + ratio (H_sample - gamma H_batch).
 * Served: 4 <= D <= 512, D % 4 == 0, 1 <= d <= 18, 1 <= g <= 10 (VQK_ERR_SHAPE otherwise, nothing launched); tau > 0 (VQK_ERR_ARG); z, q,
 * q_lo, dq, dz and ws 16-byte aligned, the parameters need no alignment.  No call allocates or synchronises; every sum over rows is
 * ordered (per-block slabs in ws + a second launch that adds them in an order fixed by their count): the same bits every run.
 * ws: >= vqk_lfq_ws_bytes(n, D, d, g) bytes, a function of the shape only, serves forward and backward (VQK_ERR_WORKSPACE).
 * forward: idx[N]; u[N][d] (optional: what the backward needs); q as fp32 (q) and / or bf16 (q_lo), both optional; hist[idx] += 1 (int32
 * [2^d], optional, pre-zeroed by the caller).  The loss is asked for with out, ltab and ws together (all three or none): out[4] = loss,
 * commit, H_sample, H_batch; ltab[ceil(d / g) << g] = log(Pbar + 1e-10) + Pbar / (Pbar + 1e-10), what the backward reads.  Without them:
 * assignment only, ONE launch, no workspace. */
int64_t vqk_lfq_ws_bytes(int64_t n, int dm, int d, int g);
int vqk_lfq_forward(const float* z, const float* w_in, const float* b_in, const float* w_out, const float* b_out, int64_t n, int dm,
                    int d, int g, float tau, float beta, float ratio, float gamma, int64_t* idx, float* u /* optional */,
                    float* q /* optional */, void* q_lo /* optional */, int32_t* hist /* optional */, float* out /* optional */,
                    float* ltab /* optional */, void* ws /* optional */, int64_t ws_bytes, void* stream);
/* idx[N] -> q (fp32 and / or bf16): c_j from bit j of the index -- no table, any int64 reads nothing out of bounds -- through the
 * forward's own device function: the same bits of q for the same index. */
int vqk_lfq_decode(const int64_t* idx, const float* w_out, const float* b_out, int64_t n, int dm, int d, float* q /* optional */,
                   void* q_lo /* optional */, void* stream);
/* du = W_out^T dq (straight-through at u, no tanh) + s dloss/du, s = *gscale_dev (a device scalar: the upstream gradient of the loss; NULL
 * = 1), p recomputed from the forward's u, the H_batch term from the forward's ltab; dz = du W_in and the four parameter gradients
 * (accumulate = 1: added to what the targets hold).  dq fp32 or bf16 (dq_dtype). */
int vqk_lfq_backward(const float* z, const float* u, const void* dq, int dq_dtype, const float* w_in, const float* w_out,
                     const float* ltab, const float* gscale_dev, int64_t n, int dm, int d, int g, float tau, float beta, float ratio,
                     float gamma, float* dz, float* dw_in, float* db_in, float* dw_out, float* db_out, int accumulate, void* ws,
                     int64_t ws_bytes, void* stream);
/* ---------------------------------------------------------------- binary spherical quantizer ---------
 * Zhao, Xiong, Kraehenbuehl 2024 (BSQ-ViT) (csrc/bsq.hip): lfq with the projected latent on the unit sphere.  Operands as for lfq.
 * v = W_in z + b_in; r = 1 / max(|v|, 1e-12); u = v r; s = 1 / sqrt(d); c_j = +s if v_j > 0 else -s (a zero or a NaN gives -s); idx =
 * sum_j [v_j > 0] 2^j; q = W_out c + b_out.  commit = sum |u - c|^2 / N (a sum over channels, a mean over rows: < 2 for every d);
 * p_nj = sigmoid(a u_nj), a = 4 s / tau; H_sample, the groups of g bits, H_batch and the loss as for lfq.
 * Served shapes, alignment, error codes, ordering of the sums and the workspace rule are lfq's, with vqk_bsq_ws_bytes(n, D, d, g).
 * forward: as vqk_lfq_forward, plus r[N] (optional; u and r are what the backward needs).  Without out / ltab / ws: assignment only, ONE
 * launch, no workspace. */
int64_t vqk_bsq_ws_bytes(int64_t n, int dm, int d, int g);
int vqk_bsq_forward(const float* z, const float* w_in, const float* b_in, const float* w_out, const float* b_out, int64_t n, int dm,
                    int d, int g, float tau, float beta, float ratio, float gamma, int64_t* idx, float* u /* optional */,
                    float* r /* optional */, float* q /* optional */, void* q_lo /* optional */, int32_t* hist /* optional */,
                    float* out /* optional */, float* ltab /* optional */, void* ws /* optional */, int64_t ws_bytes, void* stream);
/* idx[N] -> q (fp32 and / or bf16): c_j = +-s from bit j of the index, through the forward's own device function. */
int vqk_bsq_decode(const int64_t* idx, const float* w_out, const float* b_out, int64_t n, int dm, int d, float* q /* optional */,
                   void* q_lo /* optional */, void* stream);
/* e = W_out^T dq (straight-through at u) + s dloss/du, s = *gscale_dev (NULL = 1), p recomputed from the forward's u, the H_batch term
 * from the forward's ltab; through the normalisation dv = (e - u (u.e)) r with the forward's r; dz = dv W_in and the four parameter
 * gradients (accumulate = 1: added to what the targets hold).  dq fp32 or bf16 (dq_dtype). */
int vqk_bsq_backward(const float* z, const float* u, const float* r, const void* dq, int dq_dtype, const float* w_in, const float* w_out,
                     const float* ltab, const float* gscale_dev, int64_t n, int dm, int d, int g, float tau, float beta, float ratio,
                     float gamma, float* dz, float* dw_in, float* db_in, float* dw_out, float* db_out, int accumulate, void* ws,
                     int64_t ws_bytes, void* stream);
/* ---------------------------------------------------------------- self-attention core ---------
 * csrc/attn.hip.  o[b][i][h d + c] = sum_j softmax_j(scale <q[b][i][h], k[b][j][h]>) v[b][j][h d + c], lse[b][h][i] = log sum_j
 * exp(scale <q_i, k_j>) in fp32.  Operands are [B][N][ld] rows of `dtype` (VQK_F32: exact fp32 products; VQK_BF16: bf16 products, fp32
 * accumulation and statistics, P / dS rounded to bf16 only as matrix operands); every operand has its own row stride in elements
 * (>= heads * d, a multiple of 16 bytes: VQK_ERR_SHAPE) and starts 16-byte aligned (VQK_ERR_ALIGN), so the slices of one [B][N][3C]
 * tensor are read in place.  Served: d in {64, 128, 256, 512}, any n >= 1, b and heads <= 65535 (VQK_ERR_SHAPE otherwise, nothing
 * launched).  Tail keys weigh exactly zero; nothing is read or written past row n.  No call allocates or synchronises.
 * backward: delta[b][h][i] = sum_c do o (fp32 workspace of B * heads * N floats, written first), P = exp(scale S - lse) recomputed;
 * dV = P^T dO, dS = P o (dO V^T - delta), dQ = scale dS K, dK = scale dS^T Q.  Every output element is summed by one workgroup in a
 * fixed order (one pass owns key tiles, one owns query tiles): no atomics, the same bits on every run in every mode. */
int vqk_attn_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int b, int n, int heads, int d, int64_t ldq,
                 int64_t ldk, int64_t ldv, int64_t ldo, float scale, void* stream);
int vqk_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const float* lse, const void* dout, void* dq,
                 void* dk, void* dv, float* delta, int b, int n, int heads, int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                 int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, float scale, void* stream);
/* ---------------------------------------------------------------- spatially conditioned GroupNorm ---------
 * csrc/spnorm.hip (MoVQ's spatially conditional normalisation).  f, out, dy, df [N][H][W][C] of `dtype`; m, a [N][h][w][C] fp32
 * modulation tables at the latent resolution, H = r h, W = r w:  u = GroupNorm_32(f) * gamma + beta (per (sample, group) mean and
 * UNBIASED variance, as vqk_gn_*);  out = act(u * m[n][i / r][j / r] + a[n][i / r][j / r]), act = identity or SiLU (silu != 0).
 * stats[N][32] = {mean, rstd} fp32 is written by the forward and read by the backward, which recomputes the pre-activation from f.
 * backward: dm, da [N][h][w][C] fp32 are STORED (the r x r block of a latent pixel is summed by one workgroup); dgamma, dbeta [C] are
 * ADDED onto what the targets hold; df is stored.  Group and channel sums leave their workgroups as partials in ws and are added in a
 * fixed order: no float atomics, the same bits on every run in every mode.
 * Served: groups == 32, c % 32 == 0, c <= 512, r in {1, 2, 4, 8, 16, 32}, 1 <= n <= 65535, h w < 2^24, H W < 2^31 (VQK_ERR_SHAPE
 * otherwise, also from the size query; nothing launched).  f, out, dy, df, m, a, ws 16-byte aligned (VQK_ERR_ALIGN); ws_bytes >=
 * vqk_spnorm_ws_bytes (a function of the shape; one size serves forward and backward: VQK_ERR_WORKSPACE).  ws needs no initial
 * contents.  No call allocates or synchronises. */
int64_t vqk_spnorm_ws_bytes(int dtype, int n, int h, int w, int r, int c);
int vqk_spnorm_forward(int dtype, const void* f, const float* m, const float* a, const float* gamma, const float* beta, void* out,
                       float* stats, void* ws, int64_t ws_bytes, int n, int h, int w, int r, int c, int groups, float eps, int silu,
                       void* stream);
int vqk_spnorm_backward(int dtype, const void* f, const float* stats, const float* m, const float* a, const float* gamma,
                        const float* beta, const void* dy, void* df, float* dm, float* da, float* dgamma, float* dbeta, void* ws,
                        int64_t ws_bytes, int n, int h, int w, int r, int c, int groups, int silu, void* stream);
/* ---------------------------------------------------------------- residual quantizer ---------
 * Lee et al. 2022 (RQ-VAE) / SoundStream (csrc/rvq.hip).  z[N][D] fp32 rows, ONE codebook e[K][D] shared by the `depth` stages:
 * r_0 = z; k_q = argmin_k (|r_{q-1}|^2 + |e_k|^2) - 2 r_{q-1}.e_k (the arithmetic of vqk_vq_forward_f32 with assoc 0, first minimum
 * wins); r_q = r_{q-1} - e[k_q] (one fp32 subtraction per element); zhat = ((e[k_1] + e[k_2]) + ...) + e[k_Q], added in stage order
 * (NOT z - r_Q: decoding the tokens alone gives the same bits).  Tokens are idx[N][depth] int64, stage fastest.
 * loss = (1 + beta) / (N D) sum_q sse[q], sse[q] = sum_rows |r_q|^2;  dz = dq + s cz sum_q r_q;  de[k] += -s ce sum_{(row, q): k_q = k} r_q
 * (cz = 2 beta / (N D), ce = 2 / (N D), s = *gscale_dev).  1 <= depth <= 8.  No call allocates or synchronises.
 * forward: ONE launch, a block keeps its 32 residual rows in LDS for all stages; equal to `depth` calls of vqk_vq_forward_f32 on the
 * materialised residuals, bit for bit.  ws = what vqk_vq_prepare_f32 built from THIS codebook (shared by the stages, not rebuilt here).
 * q as fp32 (q) and / or bf16 (q_lo), sse[depth] and hist[depth][K] (int32) are optional; sse and hist are pre-zeroed by the caller.
 * sse: one fp32 atomic per block and stage (arrival order); in deterministic mode the blocks' partials go through the workspace of
 * vqk_set_deterministic (>= ceil(n / 32) * depth * 4 bytes: VQK_ERR_WORKSPACE) and a second one-wave launch adds them in block order.
 * Served: d == 256, k % 32 == 0 (VQK_ERR_SHAPE otherwise, nothing launched); z, e, ws, q, q_lo 16-byte aligned (VQK_ERR_ALIGN);
 * ws_bytes >= vqk_vq_filter_ws_bytes(k, d) (VQK_ERR_WORKSPACE). */
int vqk_rvq_forward_f32(const float* z, const float* e, const void* ws, int64_t ws_bytes, int64_t n, int k, int d, int depth,
                        int64_t* idx, float* q /* optional */, void* q_lo /* optional */, float* sse /* optional */,
                        int32_t* hist /* optional */, void* stream);
/* idx[N][depth] -> zhat as fp32 (q) and / or bf16 (q_lo; at least one) through the forward's own accumulation function: the same bits
 * for the same tokens.  An index outside [0, K) reads nothing and contributes nothing.  Any d % 4 == 0; e and q 16-byte, q_lo 8-byte aligned. */
int vqk_rvq_decode_f32(const int64_t* idx, const float* e, int64_t n, int k, int d, int depth, float* q /* optional */,
                       void* q_lo /* optional */, void* stream);
/* The residuals are RECOMPUTED from z, e and idx by the forward's running subtraction (the same bits; the forward saves none).  dq:
 * optional (NULL = 0), fp32 or bf16 (dq_dtype); de: optional, pre-zeroed by the caller (or holding what it is added to).  d == 256.
 * Default: per stage the rows of a 32-row block that share a code are summed in LDS, one coalesced fp32 atomic row per distinct
 * (code, block) (arrival order).  Deterministic mode (vqk_set_deterministic) with de: the residual stack R[N][depth][256] goes to ws
 * (>= vqk_rvq_backward_ws_bytes(n, d, depth) bytes, 16-byte aligned: VQK_ERR_WORKSPACE / VQK_ERR_ALIGN) and one block per code adds its
 * rows of R in (row, stage) order: no atomics, the same bits every run.  ws is not read otherwise (NULL allowed).
 * vqk_rvq_backward_ws_bytes returns VQK_ERR_SHAPE for an unserved (d, depth). */
int64_t vqk_rvq_backward_ws_bytes(int64_t n, int d, int depth);
int vqk_rvq_backward_f32(const float* z, const float* e, const int64_t* idx, const void* dq, int dq_dtype, int64_t n, int k, int d,
                         int depth, float cz, float ce, const float* gscale_dev, float* dz, float* de /* optional */, void* ws,
                         int64_t ws_bytes, void* stream);
/* ---------------------------------------------------------------- cosine quantizer ---------
 * Yu et al. 2022 (ViT-VQGAN), the factorised l2-normalised codebook (csrc/vq_cos.hip).  z[N][D], e[K][D] fp32 rows, eps = 1e-12.
 * nrm(x): ss = |x|^2 with the bits of vqk_row_sqnorm_f32; inv = 1 / max(sqrt(ss), eps), correctly rounded; xn_j = x_j * inv -- ONE
 * device function (csrc/vq_cos.h) behind every entry point below: the same row gives the same bits everywhere.
 * zn = nrm(z), en = nrm(e); idx = vqk_vq_assign_f32(zn, en, assoc 0) with |zn|^2, |en|^2 from vqk_row_sqnorm_f32, first minimum
 * wins; q = en[idx]; sse = sum |q - zn|^2; loss = (1 + beta) / (N D) sse; hist[idx] += 1.  Backward (the straight-through
 * estimator is taken at zn): g = dq + s cz (zn - q); dz = (g - zn (zn.g)) inv_z; de[k] += s ce inv_e[k] sum_{rows: idx = k}
 * (en_k (en_k.zn) - zn), cz = 2 beta / (N D), ce = 2 / (N D), s = *gscale_dev.  A clamped row (|x| < eps) has the Jacobian I / eps.
 * No call allocates, synchronises or reads the environment.
 * vqk_l2norm_rows_f32: xn = nrm(x) row-wise, inv[rows] optional; any d % 4 == 0. */
int vqk_l2norm_rows_f32(const float* x, int64_t rows, int d, float* xn, float* inv /* optional */, void* stream);
/* The per-codebook workspace en[K][D] | |en|^2[K] | inv_e[K] (each part 16-byte aligned; vqk_cos_ws_bytes(k, d) bytes, VQK_ERR_SHAPE
 * for d % 4 != 0): built when the codebook CHANGES, not per step.  ws 16-byte aligned. */
int64_t vqk_cos_ws_bytes(int k, int d);
int vqk_cos_prepare_f32(const float* e, int k, int d, void* ws, int64_t ws_bytes, void* stream);
/* forward: ONE launch -- a block stages 32 rows in LDS, normalises them there, ranks them against en streamed from L2 with the MFMA
 * sequence and comparisons of vqk_vq_assign_f32, gathers and reduces; equal to vqk_l2norm_rows_f32 + vqk_row_sqnorm_f32 +
 * vqk_vq_assign_f32 + vqk_vq_gather_f32 on the materialised rows, bit for bit.  q as fp32 (q) and / or bf16 (q_lo), sse[1] and
 * hist[K] (int32) are optional; sse and hist are pre-zeroed by the caller.  sse: one fp32 atomic per block (arrival order); in
 * deterministic mode the blocks' partials go through the workspace of vqk_set_deterministic (>= ceil(n / 32) * 4 bytes:
 * VQK_ERR_WORKSPACE) and a second launch adds them in block order.  Served: d in {8, 16, 32, 64}, k % 32 == 0 (VQK_ERR_SHAPE
 * otherwise, nothing launched); z, ws, q 16-byte, q_lo 8-byte aligned; ws_bytes >= vqk_cos_ws_bytes(k, d). */
int vqk_cos_forward_f32(const float* z, const void* ws, int64_t ws_bytes, int64_t n, int k, int d, int64_t* idx,
                        float* q /* optional */, void* q_lo /* optional */, float* sse /* optional */, int32_t* hist /* optional */,
                        void* stream);
/* sse[0] += sum |q - zn|^2 over materialised rows with the forward's block partials and thread mapping: the staged formulation's
 * sum with the forward's bits in deterministic mode (same workspace rule).  Any d % 4 == 0; zn and q 16-byte aligned. */
int vqk_cos_sse_f32(const float* zn, const float* q, int64_t n, int d, float* sse, void* stream);
/* q = en[idx] from the prepared workspace as fp32 and / or bf16 (at least one): the forward's bits for the same tokens.  A token
 * outside [0, K) reads nothing and gives a zero row.  Any d % 4 == 0. */
int vqk_cos_decode_f32(const int64_t* idx, const void* ws, int64_t ws_bytes, int64_t n, int k, int d, float* q /* optional */,
                       void* q_lo /* optional */, void* stream);
/* backward: ONE launch in default mode -- z is re-normalised with the forward's bits, dz written once, the rows of a 32-row block
 * that share a code are summed in LDS and ONE projected, coalesced fp32 atomic row per distinct (code, block) goes to de (which may
 * be a view of the optimizer's gradient arena).  dq: optional (NULL = 0), fp32 or bf16 (dq_dtype); de: optional, pre-zeroed by the
 * caller (or holding what it is added to).  Deterministic mode with de: the per-row terms go to ws2 (>= vqk_cos_backward_ws_bytes(n,
 * d) bytes: VQK_ERR_WORKSPACE) and a second launch, one block per code, adds them in row order: no atomics, the same bits every run.
 * ws2 is not read otherwise (NULL allowed).  Served: d in {8, 16, 32, 64} (VQK_ERR_SHAPE otherwise, also from the size query). */
int64_t vqk_cos_backward_ws_bytes(int64_t n, int d);
int vqk_cos_backward_f32(const float* z, const void* ws, const int64_t* idx, const void* dq, int dq_dtype, int64_t n, int k, int d,
                         float cz, float ce, const float* gscale_dev, float* dz, float* de /* optional */, void* ws2,
                         int64_t ws2_bytes, void* stream);
/* ---------------------------------------------------------------- grouped quantizer ---------
 * Product (multi-codebook) quantization (csrc/gvq.hip): the D = G d channels of a row are cut into G contiguous groups of d, group g
 * is looked up in its OWN codebook of K codes.  z[N][D] fp32 rows; e[G K][d] fp32, row g K + k = code k of group g; tokens
 * idx[N][G] int64, group fastest.  Per (row, group): idx = argmin_k (|z_rg|^2 + |e_gk|^2) - 2 z_rg.e_gk with the arithmetic of
 * vqk_row_sqnorm_f32 / vqk_vq_assign_f32 (assoc 0) on the contiguous [N, d] slice and the [K, d] slab, first minimum wins;
 * q[r][g d .. (g + 1) d) = e[g K + idx]; sse = sum |q - z|^2; loss = (1 + beta) / (N D) sse; hist[g K + idx] += 1 (hist[G K] int32).
 * Backward: dz = dq + s cz (z - q); de[g K + k] += s ce sum_{r: idx[r, g] = k} (e_gk - z_rg), cz = 2 beta / (N D), ce = 2 / (N D),
 * s = *gscale_dev -- on the flat view [N G][d] with global code ids this is the standard quantizer's backward.  G = 1 is the standard
 * quantizer.  1 <= groups <= 16, n < 2^31, k < 2^22 (VQK_ERR_SHAPE otherwise, nothing launched).  No call allocates or synchronises.
 * forward: ONE launch, grid (ceil(n / 32), groups) -- block (b, g) stages group g's columns of its 32 rows in LDS, takes |z_rg|^2
 * there, ranks against slab g streamed from L2, gathers into the strided slot and reduces; equal to `groups` times
 * (vqk_row_sqnorm_f32 + vqk_vq_assign_f32 + vqk_vq_gather_f32) on contiguous copies of the slices in idx, q and hist, bit for bit.
 * e2 = |e|^2[G K] from vqk_row_sqnorm_f32(e, G K, d) on the CURRENT codebook (an argument: no prepared workspace to go stale).
 * q as fp32 (q) and / or bf16 (q_lo), sse[1] and hist are optional; sse and hist are pre-zeroed by the caller.  sse: one fp32 atomic
 * per block (arrival order); in deterministic mode the partials go through the workspace of vqk_set_deterministic
 * (>= ceil(n / 32) * groups * 4 bytes: VQK_ERR_WORKSPACE; slot g * ceil(n / 32) + b) and a second launch adds them in slot order.
 * Served: d in {8, 16, 32, 64}, k % 32 == 0; z, e, e2, q 16-byte, q_lo 8-byte aligned (VQK_ERR_ALIGN). */
int vqk_gvq_forward_f32(const float* z, const float* e, const float* e2, int64_t n, int k, int d, int groups, int64_t* idx,
                        float* q /* optional */, void* q_lo /* optional */, float* sse /* optional */, int32_t* hist /* optional */,
                        void* stream);
/* idx[N][G] -> q[N][G d] as fp32 and / or bf16 (at least one): the forward's bits for the same tokens.  A token outside [0, K) gives
 * a zero slice and reads nothing (never another group's rows).  Any d % 4 == 0; e and q 16-byte, q_lo 8-byte aligned. */
int vqk_gvq_decode_f32(const int64_t* idx, const float* e, int64_t n, int k, int d, int groups, float* q /* optional */,
                       void* q_lo /* optional */, void* stream);
/* backward: ONE launch in default mode -- blocks of 32 flat rows [N G][d]; dz written once; the rows of a block that share a GLOBAL
 * code id g K + k are summed in LDS and ONE coalesced fp32 atomic row per distinct (code, block) goes to de (which may be a view of
 * the optimizer's gradient arena).  dq: optional (NULL = 0), fp32 or bf16 (dq_dtype); de: optional, pre-zeroed by the caller (or
 * holding what it is added to).  A token outside [0, K) is a zero code and contributes nothing to de.  Deterministic mode with de:
 * the per-row terms and the global ids go to ws group-major (>= vqk_gvq_backward_ws_bytes(n, d, groups) bytes, 8-byte aligned:
 * VQK_ERR_WORKSPACE / VQK_ERR_ALIGN) and a second launch, one block per global code, adds its group's rows in row order: no float
 * atomics, the same bits every run.  ws is not read otherwise (NULL allowed).  Served: d in {8, 16, 32, 64} (VQK_ERR_SHAPE
 * otherwise, also from the size query). */
int64_t vqk_gvq_backward_ws_bytes(int64_t n, int d, int groups);
int vqk_gvq_backward_f32(const float* z, const float* e, const int64_t* idx, const void* dq, int dq_dtype, int64_t n, int k, int d,
                         int groups, float cz, float ce, const float* gscale_dev, float* dz, float* de /* optional */, void* ws,
                         int64_t ws_bytes, void* stream);
/* ---------------------------------------------------------------- SimVQ quantizer ---------
 * Frozen code table + one learned linear layer (Zhu et al. 2024; csrc/simvq.hip): c[K][D] fp32 is never updated, w[D][D] (nn.Linear
 * orientation: row i = output i) and bias[D] are learned, the effective codebook is e[k][i] = sum_j c[k][j] w[i][j] + bias[i].  The
 * lookup against e is vqk_vq_prepare_f32 + vqk_vq_forward_f32 (d == 256) or vqk_row_sqnorm_f32 + vqk_vq_assign_f32 +
 * vqk_vq_gather_f32 (assoc 0); loss = (1 + beta) / (N D) sse.  d in {64, 128, 256}, k < 2^26, n < 2^31 (VQK_ERR_SHAPE otherwise,
 * nothing launched); c, w, bias, e, z, dz, ws 16-byte aligned, a bf16 dq 8-byte (VQK_ERR_ALIGN).  No call allocates or synchronises.
 * project: exact fp32 products, fp32 accumulation (v_mfma_f32_32x32x2_f32), the order of the sum over j fixed for a given d; the bias
 * is added last (bias NULL: none).  k % 32 == 0.  c is read once, e written once. */
int vqk_simvq_project_f32(const float* c, const float* w, const float* bias /* optional */, int k, int d, float* e, void* stream);
/* hist[idx[r]] += 1 for the tokens inside [0, k) (int32 atomics; for tables beyond the 16384 codes vqk_vq_gather_f32 counts itself) */
int vqk_simvq_hist_i32(const int64_t* idx, int64_t n, int k, int32_t* hist, void* stream);
/* backward, straight-through, two launches: dz = fma(s cz, z - q, dq) with q = e[idx] (the bits of vqk_vq_backward_f32);
 * g_r = s ce (q_r - z_r); dw[i][j] += sum_r g_r[i] c[idx_r][j]; db[i] += sum_r g_r[i]; s = *gscale_dev (NULL: 1).  Launch 1: at most
 * 256 blocks, each walks a contiguous row range (a function of n alone) in ascending order, writes dz and leaves its D x D + D
 * partial in its own slice of ws (>= vqk_simvq_backward_ws_bytes(n, d) bytes: VQK_ERR_WORKSPACE).  Launch 2 adds the slices in block
 * order and does one read-modify-write per element of dw and db, which may hold values already (views of a gradient arena).  No
 * float atomics: the same bits in every run and every mode.  dq: optional (NULL = 0), fp32 or bf16; db optional.  A token outside
 * [0, k) is a zero code: it reads nothing from e or c and adds nothing to dw / db.  c receives no gradient. */
int64_t vqk_simvq_backward_ws_bytes(int64_t n, int d);
int vqk_simvq_backward_f32(const float* z, const float* e, const float* c, const int64_t* idx, const void* dq, int dq_dtype, int64_t n,
                           int k, int d, float cz, float ce, const float* gscale_dev, float* dz, float* dw, float* db /* optional */,
                           void* ws, int64_t ws_bytes, void* stream);
/* ---------------------------------------------------------------- IBQ quantizer ---------
 * Index backpropagation (csrc/ibq.hip): z[N][D], e[K][D] fp32 rows; S_ij = inv_t (z_i . e_j), P = softmax_j S, lse_i = logsumexp_j S,
 * ebar_i = sum_j P_ij e_j, idx_i = argmax_j S_ij on the fp32 logits (the smallest index wins a tie), q_i = e[idx_i] (a bit-exact
 * gather), sse = sum_i |q_i - z_i|^2, hist[idx_i] += 1.  Exact fp32 products (v_mfma_f32_32x32x2_f32), fp32 accumulation and
 * statistics; no N x K array is ever in memory; no call allocates or synchronises.  No float atomics: every element of ebar, lse, dz
 * and de is summed by one workgroup in a fixed order and sse by an ordered finish, so the results are the same bits on every run and in
 * every mode (hist: int32 atomics).  d in {64, 128, 256}, ANY 1 <= n < 2^31 and ANY 1 <= k < 2^31 (VQK_ERR_SHAPE otherwise, nothing
 * launched): tail rows and tail codes are zeros in LDS, never read or stored; a tail code weighs exactly zero and can never win the
 * argmax.  z, e, ebar, q32, dz, de, ws 16-byte aligned, a bf16 q / dq 8-byte (VQK_ERR_ALIGN).  inv_t = 1 / T > 0.
 * forward: one launch, plus the ordered finish when sse is asked for.  idx is always written.  lse and ebar: both or neither; with
 * neither the ARGMAX-ONLY mode runs -- the same logit arithmetic, no exponentials, no second product, the same tokens bit for bit.
 * q32, qlo (bf16), sse, hist (caller-zeroed; counts are added): each optional in both modes.  sse is ASSIGNED; it needs ws of
 * >= vqk_ibq_forward_ws_bytes(n) bytes (VQK_ERR_WORKSPACE). */
int64_t vqk_ibq_forward_ws_bytes(int64_t n);
int vqk_ibq_forward_f32(const float* z, const float* e, int64_t n, int k, int d, float inv_t, int64_t* idx, float* lse /* optional */,
                        float* ebar /* optional */, float* q32 /* optional */, void* qlo /* optional */, float* sse /* optional */,
                        int32_t* hist /* optional */, void* ws, int64_t ws_bytes, void* stream);
/* backward, three launches (a row pass, a code-owning pass, a row-owning pass), s = *gscale_dev (NULL: 1), g = dq (NULL: 0, fp32 or
 * bf16), diff_i = q_i - z_i with q_i = e[idx_i]:
 *   G_i = g_i + s ce diff_i;  delta_i = G_i . ebar_i;  dS_ij = P_ij (G_i . e_j - delta_i) with P_ij = exp(S_ij - lse_i) recomputed;
 *   dz_i = -2 s ce diff_i + inv_t sum_j dS_ij e_j;   de_j += sum_{i: idx_i = j} (G_i + s cz diff_i) + inv_t sum_i dS_ij z_i
 * (ce = 2 / (N D), cz = beta ce; there is no straight-through copy of g onto z).  de is accumulated as old + sum with one
 * read-modify-write per element, so it may be a view of a gradient arena that already holds values; de NULL: the code-owning pass
 * is skipped.  The hard term is an exact product with the tile's 0 / 1 selection matrix in the fixed row order.  A token outside
 * [0, k) has diff = 0, reads nothing from e and adds no hard term; its soft terms are intact.  ws: >= vqk_ibq_backward_ws_bytes(n, d)
 * bytes (G, G + s cz diff and delta: 2 N D + N floats). */
int64_t vqk_ibq_backward_ws_bytes(int64_t n, int d);
int vqk_ibq_backward_f32(const float* z, const float* e, const int64_t* idx, const float* lse, const float* ebar,
                         const void* dq /* optional */, int dq_dtype, int64_t n, int k, int d, float inv_t, float cz, float ce,
                         const float* gscale_dev /* optional */, float* dz, float* de /* optional */, void* ws, int64_t ws_bytes,
                         void* stream);
/* ---------------------------------------------------------------- k-means codebook initialisation ---------
 * k-means++ seeding and the centroid update of a Lloyd iteration (csrc/kmeans.hip); the assignment and the per-cluster sums of an
 * iteration are vqk_vq_assign*_f32 and vqk_ema_stats*_f32.  No call allocates, synchronises or reads anything back to the host: a
 * caller loops j = 0 .. k - 1 on one stream.
 * vqk_kmeans_seed_step_f32 = pick j of k.  x[N][D] fp32 rows, D % 4 == 0, 4 <= D <= 1024, 1 <= N <= 2^36, 0 <= j < k (VQK_ERR_SHAPE);
 * device arrays picks[k] int64, u[k] FLOAT64 draws in [0, 1), mind[N] fp32, total[k] float64 (optional); ws: >= vqk_kmeans_seed_ws_bytes(N)
 * bytes (VQK_ERR_WORKSPACE; one float64 per block of 64 rows), x and ws 16-byte aligned (VQK_ERR_ALIGN).
 *   j == 0 (one launch): picks[0] = min(floor(u[0] N), N - 1); mind[i] = +inf for every i -- the caller need not initialise it;
 *           total[0] = +inf.
 *   j >= 1 (two launches): c = x[picks[j-1]], read on the device;  mind[i] = min(mind[i], sum_d (x[i,d] - c[d])^2) -- the difference
 *           form, never |x|^2 + |c|^2 - 2 x.c: a row bit-equal to c gets exactly 0 and near rows do not cancel (one fp32 fma chain per
 *           lane, an xor tree over the lanes of the row: relative error <= (D + 3) 2^-24);  total[j] = S = sum_i mind[i] in float64;
 *           with P the float64 running sums of mind in row order and t = u[j] S:  picks[j] = the smallest i with P[i] > t;  where
 *           rounding leaves none, the largest i with mind[i] > 0;  S == 0 (fewer distinct rows than centres): min(floor(u[j] N), N - 1).
 *           A pick always has mind > 0 while S > 0, so picks are pairwise distinct rows until the distinct rows run out.
 * Every sum is added in an order fixed by (N, D): the same bits of mind, total and the same picks on every run.  P is the running sum
 * of a fixed three-level tree over the 64-row blocks (csrc/kmeans.hip), within N 2^-52 S of any other float64 prefix sum. */
int64_t vqk_kmeans_seed_ws_bytes(int64_t n);
int vqk_kmeans_seed_step_f32(const float* x, int64_t n, int d, int k, int j, const double* u, int64_t* picks, float* mind,
                             double* total /* optional */, void* ws, int64_t ws_bytes, void* stream);
/* Centroid update, ONE launch: centres[c] = sums[c] / counts[c] (correctly rounded fp32 division) where counts[c] > 0, an empty cluster
 * keeps its centre bit for bit; moved[c] = |c_new - c_old|^2 (float64 sum rounded once; 0 for an empty cluster; optional).  counts[k] and
 * sums[k][D] are what vqk_ema_stats*_f32 wrote (sums at any 4-byte alignment: the packed buffer puts it k floats in); centres[k][D]
 * 16-byte aligned (VQK_ERR_ALIGN), D % 4 == 0 (VQK_ERR_SHAPE). */
int vqk_kmeans_update_f32(const float* counts, const float* sums, int k, int d, float* centres, float* moved /* optional */, void* stream);
/* EMA statistics (vector_quantizers.py:159-169): counts[k] += 1, dw[idx] += z (both pre-zeroed) ...  fp32 atomics in arrival order;
 * in deterministic mode (this entry and the fused one): one block per code adds its rows in row order, no atomics -- the same bits every run. */
int vqk_ema_stats_f32(const float* z, const int64_t* idx, int64_t n, int k, int d,
                      float* counts, float* dw, void* stream);
/* vqk_ema_stats_f32 with the rows of a 32-row block that share a code summed in LDS first (d == 256): one coalesced atomic row
 * per distinct code and block instead of one atomic per (row, channel). */
int vqk_ema_stats_fused_f32(const float* z, const int64_t* idx, int64_t n, int k, int d, float* counts, float* dw, void* stream);
/* ... and the update: count' = smooth(decay*count + (1-decay)*n_k), weight' = decay*weight + (1-decay)*dw,
 * codebook = weight'/count'.  `batch` is the smoothing constant b (global image batch). */
int vqk_ema_update_f32(float* ema_count, float* ema_weight, float* codebook, const float* counts, const float* dw,
                       int k, int d, float decay, float eps, float batch, void* stream);

/* ---------------------------------------------------------------- convolution --------------
 * Implicit-GEMM conv, stride 1, 'same' zero padding, ksize in {1,3}.
 *   x [N][Hin][Win][Cin], w [Cout][ks][ks][Cin], y [N][H][W][Cout]; (H,W) = (Hin,Win) << ups.
 *   ups = 1 fuses a nearest x2 upsample of x into the input addressing (autoencoder.py:104-106).
 *   bias (fp32, optional), residual (same dtype/shape as y, optional) are fused into the epilogue;
 *   act: 0 none, 1 tanh, 2 relu, 3 leaky-relu(0.2).  in/w dtype = `dtype`; y/residual dtype = out_dtype.
 *   Cin must be a multiple of 16 bytes worth of elements (4 fp32 / 8 bf16).
 * dgrad is the same entry point with weights repacked by vqk_conv_pack_dgrad. */
int vqk_conv2d_fprop(int dtype, const void* x, const void* w, const float* bias, const void* residual, void* y,
                     int out_dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int ups, int act,
                     int wlayout, const void* zeros, void* stream);
/* The same conv with a 2x2 pooling of its output fused into the epilogue: y[N][H/2][W/2][Cout] = pool_scale * (sum over
 * each 2x2 block of conv(x) + bias + residual) -- pool_scale 0.25: the avg_pool2d that follows a level's last ResBlock
 * (autoencoder.py:89-91, residual = the block's skip input at full resolution); pool_scale 1: the backward of the nearest
 * x2 upsample in front of an Upsample conv (:104-106).  bf16 only, fragment-major weights (layout 1), Cout % 128 == 0;
 * VQK_ERR_SHAPE when the problem is not eligible (callers then use vqk_conv2d_fprop + vqk_pool2x2). */
int vqk_conv2d_fprop_pooled(int dtype, const void* x, const void* w, const float* bias, const void* residual, void* y,
                            int n, int h_in, int w_in, int cin, int cout, int ksize, int ups, float pool_scale,
                            const void* zeros, void* stream);
/* The 3x3 conv (optionally with the fused 2x2 pooling) that ALSO accumulates the GroupNorm statistics of its output: the
 * per-(sample, group) sums of y and y*y (y as stored: rounded to bf16) are added to gn_ws[n][group][2] (doubles), the
 * workspace of vqk_gn_forward -- the consumer then calls vqk_gn_forward_presummed and the statistics pass over y
 * (autoencoder.py:25-39 re-reads its input once for mean / variance) disappears.  bf16, fragment-major weights, Cout % 128
 * == 0, (Cout / groups) % 4 == 0; VQK_ERR_SHAPE when the problem is not served by the matrix/auxiliary-wave kernel
 * (nothing has been launched: callers fall back to vqk_conv2d_fprop[_pooled] + vqk_gn_forward). */
int vqk_conv2d_fprop_gnstats(int dtype, const void* x, const void* w, const float* bias, const void* residual, void* y,
                             int n, int h_in, int w_in, int cin, int cout, int ksize, int ups, int pool, float pool_scale,
                             double* gn_ws, int groups, const void* zeros, void* stream);
/* The 3x3 conv on the padded 3-channel image (the encoder's first conv, autoencoder.py:132; x [N][H][W][8], w [Cout][3][3][8] in the compute
 * dtype, layout 0) with the GroupNorm sums of its output left in gn_ws as vqk_conv2d_fprop_gnstats leaves them.  Served: bf16,
 * Cout = 128 in 32 groups, W % 32 == 0, not in deterministic mode; VQK_ERR_SHAPE otherwise (nothing launched: callers run
 * vqk_conv2d_fprop and vqk_gn_forward). */
int vqk_conv2d_thin_in_gnstats(int dtype, const void* x, const void* w, const float* bias, void* y, int n, int h, int wd, int cout,
                               double* gn_ws, int groups, void* stream);
/* The nearest-x2 upsample + 3x3 conv of autoencoder.py:104-106 in PHASE form: output pixel (2i+a, 2j+b) only sees a 2x2
 * window of the low-resolution input with pre-summed weights, so the conv runs as four 2x2-tap launches (4/9 of the
 * multiply-adds).  w4: the operand of vqk_conv_pack_weights(..., layout 2) -- transpose = 0 for backward = 0 (x [N][h][w][Cin]
 * -> y [N][2h][2w][Cout] (+ bias; gn_ws as in vqk_conv2d_fprop_gnstats, or NULL)), transpose = 1 for backward = 1 (x = dy
 * [N][2h][2w][Cin := conv's Cout] -> y = dx [N][h][w][Cout := conv's Cin], the four phases accumulate in place).  bf16,
 * Cout % 128 == 0, Cin % 64 == 0; VQK_ERR_SHAPE when the matrix/auxiliary-wave kernel does not serve the problem (nothing
 * launched: callers use vqk_conv2d_fprop with ups = 1 / the pooled data gradient).
 * dtype VQK_F32 (this entry and the two pooled forms below): the SPLIT-PRODUCT mode -- fp32 tensors, w4 in layout 6, every product as
 * three bf16 products (csrc/conv_x3.hip, NTAP = 4), one launch for the four phases; Cout % 128 == 0, Cin % 32 == 0, h % 8 == 0,
 * w % 16 == 0 (h, w: the LOW resolution); gn_ws: groups of 4 / 8 / 16 channels, not in deterministic mode. */
int vqk_conv2d_ups_phase(int dtype, const void* x, const void* w4, const float* bias, void* y, int n, int h, int w,
                         int cin, int cout, int backward, double* gn_ws, int groups, const void* zeros, void* stream);
/* Data gradient of a 3x3 conv that is FOLLOWED by a 2x2 average pool (the encoder's Downsample in a ResBlock's last conv,
 * vqvae/modules/autoencoder.py:89-91), from the POOLED gradient, in phase form: dx [n, 2h, 2w, cout] = scale * (nearest-x2(dy_pooled)
 * conv flip(W)^T) -- every full-resolution pixel of a 2x2 block sees the same pooled gradient, so phase (a, b) of dx reads a 2x2
 * window of dy_pooled [n, h, w, cin] with pre-summed weights: 4/9 of the multiply-adds of the tap form (vqk_conv2d_general with the
 * nearest-x2 addressing).  w4t = vqk_conv_pack_weights(..., transpose = 1, layout = 2) of the conv's weight (the operand of
 * vqk_conv2d_ups_phase(backward = 1)); scale = the pool's 0.25.  Same shape rules as vqk_conv2d_ups_phase; VQK_ERR_SHAPE when not served. */
int vqk_conv2d_pooled_dgrad_phase(int dtype, const void* dy_pooled, const void* w4t, void* dx, int n, int h, int w, int cin,
                                  int cout, float scale, const void* zeros, void* stream);
/* FORWARD of a 3x3 conv followed by a 2x2 average pool, as the 4x4 stride-2 conv it is: y [n, h, w, cout] = scale * (sum over each
 * 2x2 block of conv3x3(x, W)) + res_pooled, x [n, 2h, 2w, cin].  One data-gradient-type phase launch (the tile accumulates the four
 * input phases in registers and is stored once) with the conv's FORWARD phase operand w4 = vqk_conv_pack_weights(..., transpose = 0,
 * layout = 2), phase blocks reversed: 4/9 of the multiply-adds of the conv + pooling-drain form (vqk_conv2d_fprop_pooled).
 * res_pooled (may be NULL): the POOLED residual, [n, h, w, cout]; gn_ws / groups as in vqk_conv2d_fprop_gnstats (sums of y).
 * Same shape rules as vqk_conv2d_ups_phase; VQK_ERR_SHAPE when not served. */
int vqk_conv2d_pooled_fprop_phase(int dtype, const void* x, const void* w4, const void* res_pooled, void* y, int n, int h, int w,
                                  int cin, int cout, float scale, double* gn_ws, int groups, const void* zeros, void* stream);
/* General form (im2col kernel when not plain): stride in {1,2}, explicit zero padding `pad`, explicit output size;
 * mode 0: x as is, 1: nearest x2 upsample of x, 2: x zero-stuffed x2 (the dgrad of a stride-2 conv, with flipped /
 * transposed weights and pad = ks-1-pad_fwd).  Epilogue: y = out_gain * act(acc * acc_scale + bias) + residual, act 0
 * none, 1 tanh, 2 relu, 3 leaky-relu(0.2) -- acc_scale is the StyleGAN2 runtime weight gain (discriminator.py:165),
 * out_gain the bias_act gain (bias_act.py:55).  Strided/padded problems need weight layout 0. */
int vqk_conv2d_general(int dtype, const void* x, const void* w, const float* bias, const void* residual, void* y,
                       int out_dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int stride, int pad,
                       int mode, int h_out, int w_out, int act, float acc_scale, float out_gain, int wlayout,
                       const void* zeros, void* stream);
/* The 3x3 weight gradient when dy is the gradient of a FUSED 2x2 average pool (vqk_conv2d_fprop_pooled): dy_pooled is
 * [N][h/2][w/2][Cout], every pooled pixel stands for its 2x2 block, dW += scale * sum over the h x w pixels (scale = the
 * pool's 0.25): the full-resolution copy of the gradient is never written.  bf16, h % 8 == 0, w % 16 == 0, Cin % 64 == 0,
 * Cout % 64 == 0; VQK_ERR_SHAPE when not served (nothing launched: callers unpool and call vqk_conv2d_wgrad). */
int vqk_conv2d_wgrad_pooled_dy(int dtype, const void* x, const void* dy_pooled, float* dw, int n, int h, int w, int cin,
                               int cout, float scale, const void* zeros, void* stream);
/* Weight gradient of a nearest-x2 UPSAMPLE + 3x3 conv (vqvae/modules/autoencoder.py:102-105) in PHASE form (csrc/conv_wgmx.hip):
 * x [n, h, w, cin] is the LOW-resolution input, dy [n, 2h, 2w, cout] the gradient of the conv's output;
 * dw[Cout][3][3][Cin] += scale * the gradient, from a 2x2-window kernel per output phase (4/9 of the multiply-adds of the tap
 * form vqk_conv2d_wgrad(..., ups = 1)): the four phases as one launch, or one launch each with tuning slot UPS_MERGE = 0.  bf16, h % 8 == 0, w % 16 == 0, cin % 64 == 0, cout % 64 == 0;
 * VQK_ERR_SHAPE when not served (deterministic mode included: nothing launched, callers use the tap form). */
int vqk_conv2d_wgrad_ups_phase(int dtype, const void* x, const void* dy, float* dw, int n, int h, int w, int cin, int cout,
                               float scale, const void* zeros, void* stream);
/* Weight gradient of a 3x3 conv FOLLOWED by a 2x2 average pool from the pooled gradient, in phase form (the mirror image of
 * vqk_conv2d_wgrad_ups_phase: operands' roles swapped, csrc/conv_wgmx.hip): x [n, 2h, 2w, cin] the conv's input, dy_pooled
 * [n, h, w, cout]; dw[Cout][3][3][Cin] += scale * wgrad(x, unpool(dy_pooled)) with 4/9 of the multiply-adds of
 * vqk_conv2d_wgrad_pooled_dy.  Same shape rules; VQK_ERR_SHAPE when not served (deterministic mode included). */
int vqk_conv2d_wgrad_pooled_dy_phase(int dtype, const void* x, const void* dy_pooled, float* dw, int n, int h, int w, int cin,
                                     int cout, float scale, const void* zeros, void* stream);
int vqk_conv2d_wgrad_general(int dtype, const void* x, const void* dy, float* dw, int n, int h_in, int w_in, int cin,
                             int cout, int ksize, int stride, int pad, int mode, int h_out, int w_out,
                             const void* zeros, void* stream);
/* Split-product mode (layout 5 above), weight gradient of a 3x3 conv (optionally behind a nearest-x2 upsample, ups = 1):
 * vqk_split_pair_f32 turns an fp32 [rows][c] activation / gradient into its bf16 (hi | lo) PAIR tensor [rows][2c]
 * (hi = bf16(v), lo = bf16(v - hi); c % 8 == 0); vqk_conv2d_wgrad_x3 takes x_pair [n][h_in][w_in][2 cin] and dy_pair
 * [n][h][w][2 cout] and adds scale * (dy_hi^T x_hi + dy_hi^T x_lo + dy_lo^T x_hi) to dw fp32 [Cout][3][3][Cin]: three tile classes
 * of ONE launch of the bf16 matrix/auxiliary-wave weight-gradient kernel (csrc/conv_wgmx.hip), folded by its atomic pass.
 * cin % 64 == 0, cout % 64 == 0, h % 8 == 0, w % 16 == 0; VQK_ERR_SHAPE when not served (deterministic mode included:
 * nothing launched, callers use the exact-fp32 vqk_conv2d_wgrad). */
/* vqk_conv2d_wgrad_x3_f32: the same gradient straight from the fp32 tensors x [n][h_in][w_in][cin], dy [n][h][w][cout] -- both are
 * split in registers on their way into LDS and all three products come from one staged patch (csrc/conv_x3.hip:
 * conv3x3_wgrad_x3_kernel; no pair tensors, no split passes).  cin % 64 == 0, cout % 64 == 0, h % 8 == 0, w % 8 == 0.
 * ups = 1 with h_in % 8 == 0, w_in % 8 == 0 runs in PHASE form (four 2x2-window launches' worth of blocks on the low-resolution grid,
 * 4/9 of the MFMAs; tuning slot X3_WGRAD_PHASE = 0: the tap form).  ups = 2: the gradient of a conv that is FOLLOWED by a 2x2 average
 * pool, from the POOLED gradient -- dy [n][h_in / 2][w_in / 2][cout], x [n][h_in][w_in][cin], scale = the pool's 0.25: phase form only
 * (h_in % 16 == 0, w_in % 16 == 0; VQK_ERR_SHAPE otherwise, nothing launched). */
/* vqk_conv2d_fprop_x3_gnstats: the layout-5 3x3 conv with the GroupNorm sums of its OUTPUT (sum, sum of squares per (sample, group),
 * fp64 atomics) left in gn_ws as vqk_conv2d_fprop_gnstats leaves them for the bf16 convs -- the consuming vqk_gn_forward_presummed
 * skips its statistics pass.  Cout % 128 == 0, Cout / groups in {4, 8, 16}; VQK_ERR_SHAPE otherwise and in deterministic mode. */
int vqk_conv2d_fprop_x3_gnstats(const float* x, const void* w5, const float* bias, const float* residual, float* y, int n, int h_in,
                                int w_in, int cin, int cout, int ups, double* gn_ws, int groups, const void* zeros, void* stream);
int vqk_split_pair_f32(const float* src, void* dst, int64_t rows, int c, void* stream);
int vqk_conv2d_wgrad_x3_f32(const float* x, const float* dy, float* dw, int n, int h_in, int w_in, int cin, int cout, int ups,
                            float scale, void* stream);
int vqk_conv2d_wgrad_x3(const void* x_pair, const void* dy_pair, float* dw, int n, int h_in, int w_in, int cin, int cout, int ups,
                        float scale, const void* zeros, void* stream);
/* the same with dW += scale * (the gradient): a layer whose backward carries a scalar gain (the discriminator's linear skip convs:
 * weight gain x output gain) accumulates straight into an optimizer's gradient arena -- no zeroed temporary, scale pass and add */
int vqk_conv2d_wgrad_general_scaled(int dtype, const void* x, const void* dy, float* dw, int n, int h_in, int w_in, int cin,
                                    int cout, int ksize, int stride, int pad, int mode, int h_out, int w_out, float scale,
                                    const void* zeros, void* stream);
/* The STRIDE-2 3x3 conv without padding of the StyleGAN2 discriminator's down-sampling layers (the reference's
 * conv2d_resample.py:119-122: upfirdn2d blur with padding, then F.conv2d(stride=2)) and its data gradient on the
 * matrix/auxiliary-wave kernel (bf16).  vqk_conv2d_s2_supported: 1 when the shape is served (backward = 0: the conv, Cin % 64
 * == 0, Cout % 128 == 0, W_out % 32 == 0 && H_out % 4 == 0 or W_out % 16 == 0 && H_out % 8 == 0; backward = 1: its data gradient,
 * Cout % 64 == 0, Cin % 128 == 0, maps of 32x32 and more), 0 otherwise (callers use vqk_conv2d_general).
 * vqk_conv2d_s2_fprop: x [N][2 H_out + 1][2 W_out + 1][Cin] -> y [N][H_out][W_out][Cout] = out_gain * act(acc_scale * conv + bias);
 * wq = vqk_conv_pack_weights(..., transpose 0, layout 1).  The four parity sub-images of an input patch are staged side by
 * side in LDS, so every tap reads at unit stride.
 * vqk_conv2d_s2_dgrad: dy [N][H_out][W_out][Cout] -> dx [N][2 H_out + 1][2 W_out + 1][Cin] = acc_scale * gradient, EVERY element
 * written; w3 = vqk_conv_pack_weights(..., transpose 1, layout 3) (the four output parities' 4 / 2 / 2 / 1 taps), wt0 = the same
 * weights with transpose 1, layout 0 (the last row and the last column of dx run as parity classes of the im2col kernel). */
int vqk_conv2d_s2_supported(int dtype, int n, int h_out, int w_out, int cin, int cout, int backward);
int vqk_conv2d_s2_fprop(int dtype, const void* x, const void* wq, const float* bias, void* y, int n, int h_out, int w_out,
                        int cin, int cout, int act, float acc_scale, float out_gain, const void* zeros, void* stream);
int vqk_conv2d_s2_dgrad(int dtype, const void* dy, const void* w3, const void* wt0, void* dx, int n, int h_out, int w_out,
                        int cin, int cout, float acc_scale, const void* zeros, void* stream);
/* Weight operand layouts.  0: [Cout][ks][ks][Cin] (any shape).  1: "fragment-major" for the register-weight halo
 * kernel (3x3, Cin a whole 128-byte chunk, W%32==0 && H%8==0 or W%16==0 && H%16==0): Cout padded to a multiple of
 * 128, element order [Cout/32][64-byte Cin chunk][tap][k-substep 0..1][lane 0..63][16 bytes]: every MFMA operand
 * fragment is one coalesced 1 KiB load and the 18 fragments of a (cout tile, chunk) are contiguous.  vqk_conv_weight_layout() returns the layout the fprop launcher wants for
 * a problem (>= 0) or a negative status; vqk_conv_packed_elems() the element count of the packed buffer;
 * vqk_conv_pack_weights() builds it from the fp32 [Cout][ks][ks][Cin] master (transpose = 1: the dgrad operand,
 * i.e. Cin/Cout swapped and both taps flipped).  2: the upsample-phase operand of vqk_conv2d_ups_phase (bf16, 3x3): four
 * phases (a, b) of fragment-major blocks with FOUR taps each, tap (r, s) of a phase = the sum of the 3x3 taps that fall
 * on the same low-resolution pixel (rows {0},{1,2} for a = 0 and {0,1},{2} for a = 1; columns alike); transpose = 1:
 * channels swapped and the 2x2 taps mirrored.  5: the SPLIT-PRODUCT operand (csrc/conv_x3.hip; dtype VQK_F32, 3x3 or 1x1, Cin % 32 == 0):
 * layout 1 in bf16 with every fragment twice, hi = bf16(w) then lo = bf16(w - hi) -- [Cout/32][32-channel chunk][tap][k-substep]
 * [hi | lo][lane][16 bytes], 4 bytes per weight like the fp32 operands.  vqk_conv2d_fprop(VQK_F32, ..., out VQK_F32, wlayout 5)
 * then evaluates every product as x_hi w_hi + x_lo w_hi + x_hi w_lo on the bf16 matrix pipe with fp32 accumulation (the fp32
 * activations are split on the fly; ~2^-17 relative per product): H % 8 == 0, W % 16 == 0 at the OUTPUT resolution, Cout % 4 == 0;
 * callers choose it (vqk_conv_weight_layout never returns 5; layout 1 / dtype VQK_F32 stays the exact v_mfma_f32_32x32x2_f32 mode).
 * 6: layout 2's phase-summed four-tap operand (the sums taken in fp32) stored as layout 5's (hi | lo) fragment pairs -- the operand of the
 * phase entry points with dtype VQK_F32: [phase][Cout/32][32-channel chunk][tap 0..3][k-substep][hi | lo][lane][16 bytes]. */
int vqk_conv_weight_layout(int dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int ups);
int64_t vqk_conv_packed_elems(int cout, int cin, int ksize, int layout);
int vqk_conv_pack_weights(const float* w, void* out, int dtype, int cout, int cin, int ksize, int transpose,
                          int layout, void* stream);
/* Every conv operand of a model in ONE launch: descs_dev is a device array of ndesc descriptors of eight int64 words
 * {src, dst, dtype, cout, cin, ksize, transpose, layout}, each with the meaning of the vqk_conv_pack_weights
 * arguments.  Issued once per optimizer step (after vqk_adamw) instead of one pack launch per conv call; replaces
 * the per-call weight casts autocast performs in the reference's conv calls (vqvae/modules/autoencoder.py:57-60). */
int vqk_conv_pack_multi(const int64_t* descs_dev, int ndesc, int blocks_per_desc, void* stream);
/* test / tuning hook for the conv kernel choice of the calling thread (csrc/conv_geom.h: ConvVariant):
 *  -1 automatic;
 *   0 the general kernels only: im2col forward / data gradient (no halo, thin, matrix-wave or stride-2 form), general weight gradient;
 *   1 halo kernels when eligible (what the automatic choice does);
 *   2 vqk_conv_weight_layout answers 0, hence the halo kernel with LDS-staged plain weights instead of register weights;
 *     vqk_conv2d_fprop_pooled / _gnstats refuse;
 *   3 bf16 layout-1 convs on the one-tile-per-block register-weight halo kernel instead of the persistent stream and
 *     matrix/auxiliary-wave kernels; the pooled / gnstats entries refuse;
 *   4 stream kernel without its half-tile (128-pixel) form for maps with fewer 256-pixel tiles than CUs;
 *   5 never the matrix/auxiliary-wave kernel (forward, 1x1, phase and stride-2 forms);
 *   6 that kernel whenever the shape is eligible, below the MX_MIN_TILES tuning slot too. */
int vqk_conv_set_variant(int variant);
/* The forward launcher's PLAN for a problem, without launching (no device needed): the kernel form vqk_conv2d_fprop (flags 0 / 1),
 * vqk_conv2d_fprop_pooled (flag 2: act 0, wlayout 1) or vqk_conv2d_fprop_gnstats (flag 4, with 2 for its pooled form) would launch
 * under the calling thread's variant, block caps and scratch and the current tuning slots -- a form id >= 0 -- or the negative
 * status that call would return given valid, aligned pointers.  flags: 1 a residual is added, 2 pooled epilogue, 4 fused GroupNorm
 * sums (the groups are not checked), 8 a strided, explicitly padded or zero-stuffed conv of vqk_conv2d_general (always the im2col
 * kernel; the other arguments then only pick the label).  The epilogue gains of vqk_conv2d_general count as 1.  Form ids: 0 fp32 thin-out, 1 fp32 thin-in, 2 matrix/auxiliary-wave,
 * 3 its 1x1 form, 4 / 5 / 6 stream kernel with thin / half / full tiles, 7 register-weight halo, 8 LDS-weight halo, 9 bf16 thin-in,
 * 10 im2col, 11 im2col with split-K, 12 split-product (wlayout 5), 13 its 1x1 form.  details (may be NULL): five ints --
 * patch width log2 (5 / 4, 0: no pixel patches), blocks of the first launch (0: sized by the form's own launcher), split-K parts,
 * number of launches, 1 when the form is memory-bound (the event statistics report it by bytes, name suffix " (HBM)").
 * vqk_conv_fprop_form_name: the kernel's name for the event statistics, "?" for an unknown id. */
int vqk_conv_fprop_plan(int dtype, int out_dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int ups, int act,
                        int wlayout, int flags, int* details);
const char* vqk_conv_fprop_form_name(int form, int dtype);
/* Deterministic mode (the reference trains with `deterministic=True`, vqvae/train.py:130).  on = 1: the float accumulations of
 * the train step that are otherwise combined with atomics in arrival order -- split-K partials of the weight gradients, column
 * sums (bias gradients), the cross-block sums of the GroupNorm statistics / backward reductions and of d gamma / d beta, the
 * per-code sums of the codebook gradient -- go through `ws` (>= 64 MiB recommended; VQK_ERR_WORKSPACE when a call needs more -- vqk_colsum_lead alone answers VQK_ERR_ARG, see there)
 * as per-block partials that are added in index order, or run unsplit.  THREAD-LOCAL like the block caps; the workspace must
 * belong to the stream the following launches go to (two streams = two workspaces, re-armed on every switch).  The scalar
 * loss sums keep their atomics (values, not gradients); the EMA statistics, which the codebook is trained from, are added in row order
 * (vqk_ema_stats_f32). */
int vqk_set_deterministic(int on, void* ws, int64_t ws_bytes);
/* Optional fp32 scratch of the CURRENT stream (thread-local like the block caps; NULL = none; contents need not be
 * initialised).  With it the general conv kernel splits K for problems whose pixel x cout tile grid would leave most of the
 * chip idle (the discriminator's 4x4 / 8x8 convs and fully connected layers: 8-32 tiles with K up to 8192): every split
 * stores its partial tile into its own slice and an epilogue kernel adds the slices in split order (no atomics: the same
 * bits every run, so the split is also taken in deterministic mode).  Needs >= 2 * pixels * cout * 4 bytes to be used.
 * ws must be 16-byte aligned (VQK_ERR_ALIGN), ws_bytes >= 0 (VQK_ERR_ARG); the same checks apply to vqk_set_deterministic. */
int vqk_set_scratch(void* ws, int64_t ws_bytes);
/* DYNAMIC TILE QUEUE of the persistent matrix/auxiliary-wave conv kernel (csrc/conv_mx.hip; tuning slot TILE_QUEUE: 0 = off,
 * the static share; 1 = a block's first tile is its static one, the rest are drawn; 2 = every tile is drawn).  ws: >= 64 bytes
 * of int32 words, ZERO on the first use; the kernels leave them zero again (the last block of a launch to run out of tiles
 * resets them), so launches that follow each other on ONE stream may share them -- launches that can run CONCURRENTLY (other
 * streams) need words of their own: the pointer is THREAD-LOCAL like vqk_set_scratch and is meant to follow the caller's
 * current stream.  ws = NULL: static share.  Results do not depend on the mode (a tile's arithmetic and its destination are
 * functions of the tile index only).  VQK_ERR_WORKSPACE below 64 bytes, VQK_ERR_ALIGN unless 16-byte aligned.
 * A kernel that is KILLED mid-way leaves the words dirty: re-zero them before the next launch. */
int vqk_set_tile_queue(void* ws, int64_t ws_bytes);
/* WORKSPACE CONTEXTS (round 6): the three workspaces above as fields of an object instead of three thread-local pointers.
 * A context is plain host memory (no device allocation, no stream): create one per (device, stream, host thread) that launches,
 * give it its workspaces ONCE, and name it before a batch of launches -- vqk_ctx_make_current is one pointer store, the only
 * thread-local state left on this path (the analogue of hipSetDevice).  ctx = NULL in a vqk_ctx_set_* call addresses the calling
 * thread's current context, which is what vqk_set_scratch / vqk_set_tile_queue / vqk_set_deterministic do: they are wrappers.
 * vqk_ctx_make_current(NULL) returns to the thread's own default context.  Two models stepped from two host threads, or one
 * thread alternating between two streams, hold one context each (ops.py::_stream).  A context must not be destroyed while a
 * thread still has it current (the destroying thread's own current pointer is reset). */
typedef struct vqk_ctx vqk_ctx;
int vqk_ctx_create(vqk_ctx** ctx);
int vqk_ctx_destroy(vqk_ctx* ctx);
int vqk_ctx_make_current(vqk_ctx* ctx);
int vqk_ctx_set_scratch(vqk_ctx* ctx, void* ws, int64_t ws_bytes);
int vqk_ctx_set_tile_queue(vqk_ctx* ctx, void* ws, int64_t ws_bytes);
int vqk_ctx_set_deterministic(vqk_ctx* ctx, int on, void* ws, int64_t ws_bytes);
/* Tuning slots: the launch heuristics that tools/ sweep (formerly read-once environment variables).  name = one of
 * vqk_tuning_name(0 .. vqk_tuning_count() - 1): MX, MX_1X1, TW16, STREAM_BLOCKS, MX_MIN_TILES, FPROP_SPLITK, SK_BLOCKS, SK_MINSTEPS, SK_MAXMB, UPS_PHASE, WGRAD_BLOCKS, WGMX, WGRAD_GEN_BLOCKS, WGRAD_NO_PW16, WGRAD_NO_P16K, MX_HALF, MX_HALF_HW, UPFIRDN_TILE, GN_BLOCKS_REDUCE, GN_BLOCKS_APPLY, GN_NT_MB, GN_NO_SMALL, WGMX_COEF_E4, GN_CLUSTER_MAX_HW, COMM_CUS, MX_QUARTER, MX_S2, MX_S2_DGRAD_MIN, UPS_MERGE, TILE_QUEUE, WGRAD_GROUP_LOAD_PCT, WGRAD_GROUP_MIN_PPS, MX_PHASE_U64.
 * A set slot overrides the built-in default at the next launch; vqk_reset_tuning returns every slot to its default.
 * Process-wide (relaxed atomics); VQK_ERR_ARG for an unknown name.  The Python host maps VQK_<NAME> environment variables
 * onto these calls when it loads the library (_native.py), so the A/B scripts keep their interface. */
int vqk_set_tuning(const char* name, int value);
int vqk_reset_tuning(void);
int vqk_tuning_count(void);
const char* vqk_tuning_name(int i);
/* caps on the persistent grids of the 3x3 fprop/dgrad kernel and of the all-taps wgrad kernel (0 = default: two
 * blocks per CU).  256 = one block per CU, leaving room for a kernel that runs concurrently on another stream
 * (the host overlaps a layer's wgrad with its dgrad and GroupNorm backward).  The caps are THREAD-LOCAL: they apply to the
 * launches the calling thread issues afterwards (set, launch, reset in one place), never to another thread or device
 * context.  vqk_conv_set_variant above is a TEST hook, thread-local like the caps, and not meant for product code. */
int vqk_conv_set_block_caps(int stream_blocks, int wgrad_blocks);
/* DIAGNOSTIC (tools/comm_probe.py): a stand-in for a collective's kernel -- `blocks` persistent 256-thread blocks stream
 * dst[i] += src[i] over `bytes` (16-byte aligned, a multiple of 16) `passes` times, sleeping `sleep` x 64 cycles between
 * 4-KiB pieces, so that a chosen number of CUs stays occupied for a chosen time while the train step runs on another stream. */
int vqk_probe_stream_add(const float* src, float* dst, int64_t bytes, int blocks, int passes, int sleep, void* stream);
/* BOX CALIBRATION (bench.py `box_calibration`; csrc/calib.hip) -- not part of the train step.  vqk_calib_fill: pseudo-random bf16
 * pairs of N(0,1)-like magnitude into w.  vqk_calib_mfma: `blocks` x 256 threads (one wave per SIMD) run `iters` x 18 phases of
 * the role-split conv kernel's matrix-wave instruction mix (4 LDS fragment reads + 2 L2 weight fragments + 8 bf16 32x32x16 MFMAs)
 * on the random operands of w (w_bytes: a power of two in [64 KiB, 1 GiB]); vqk_calib_mfma_flops = the multiply-add FLOPs of one
 * such launch.  vqk_calib_copy: dst = src, 16 bytes per lane, streaming (bytes % 16 == 0): HBM read + write bandwidth. */
int vqk_calib_fill(void* w, int64_t bytes, void* stream);
int vqk_calib_mfma(const void* w, int64_t w_bytes, float* sink, int iters, int blocks, void* stream);
int64_t vqk_calib_mfma_flops(int iters, int blocks);
int vqk_calib_copy(const void* src, void* dst, int64_t bytes, void* stream);
/* w [Cout][ks][ks][Cin] -> wt [Cin][ks][ks][Cout] with both taps flipped; src fp32, dst `dtype`. */
int vqk_conv_pack_dgrad(const float* w, void* wt, int dtype, int cout, int cin, int ksize, void* stream);
/* dw[Cout][ks][ks][Cin] (fp32) += sum_pix dy[pix][co] * x[pix (+) tap][ci].  dw must be pre-zeroed
 * (split-K partials are combined with fp32 atomics). */
int vqk_conv2d_wgrad(int dtype, const void* x, const void* dy, float* dw, int n, int h_in, int w_in, int cin,
                     int cout, int ksize, int ups, const void* zeros, void* stream);
/* GROUPED 3x3 weight gradients: the layers of a backward stage whose maps are too small to fill the chip one at a time (a
 * 512 -> 512 conv at 16x16 has 64 dW tiles; alone it is split over K and pays an atomic pass per split) in ONE launch per 16
 * items.  Per item: dw[Cout][3][3][Cin] (fp32) += scale * sum_pix dy[pix][co] * x[pix (+) tap][ci], x [n][h][w][cin], dy
 * [n][h][w][cout] bf16 nhwc.  Served per item: dtype VQK_BF16, ksize 3, ups 0 (plain stride-1 3x3), h % 8 == 0, w % 16 == 0,
 * cin % 64 == 0, cout % 64 == 0 (VQK_ERR_SHAPE), x / dy / dw 16-byte aligned (VQK_ERR_ALIGN), no NULL (VQK_ERR_ARG); ONE item
 * that does not qualify refuses the call and nothing is launched.  Deterministic mode: VQK_ERR_SHAPE (callers launch
 * vqk_conv2d_wgrad per layer, whose ordered workspace sums stay as they are).
 * The work table travels in the kernel arguments (no device copy: the call can be captured into a graph); the items are
 * caller-owned and only read during the call.  Partition (tuning slots WGRAD_GROUP_LOAD_PCT, WGRAD_GROUP_MIN_PPS): a layer's K is
 * split only when one block per dW tile would run longer than the even share of the launch's work per CU.  An unsplit layer is
 * added to dw with plain loads and stores -- the same bits every run; a split one with fp32 atomics, like vqk_conv2d_wgrad.
 * vqk_conv3x3_wgrad_group_plan: the same validation, no launch; splits[i] = the K-splits item i would get, *launches = the
 * number of kernel launches. */
typedef struct vqk_wgrad_item {
    const void* x;
    const void* dy;
    float* dw;
    int dtype, n, h, w, cin, cout, ksize, ups;
    float scale;
    int reserved;
} vqk_wgrad_item;
int vqk_conv3x3_wgrad_group(const vqk_wgrad_item* items, int n_items, const void* zeros, void* stream);
int vqk_conv3x3_wgrad_group_plan(const vqk_wgrad_item* items, int n_items, int* splits, int* launches);
/* The one-layer weight-gradient launcher's PLAN for a problem, without launching (no device needed): the kernel form the entry
 * point of `op` would launch under the calling thread's variant, block cap and deterministic state and the current tuning slots
 * -- a form id >= 0 -- or the negative status that call would return given valid, aligned pointers.  cin / cout: the conv's true
 * channel counts.  op: 0 vqk_conv2d_wgrad / _general / _general_scaled (all arguments as vqk_conv2d_wgrad_general takes them, ups
 * = its mode; vqk_conv2d_wgrad: stride 1, pad ksize / 2, h_out = h_in << ups); 1 vqk_conv2d_wgrad_pooled_dy, 2 _ups_phase,
 * 3 _pooled_dy_phase ((h_in, w_in) = the entry point's (h, w)); 4 vqk_conv2d_wgrad_x3 (with ups); 5 vqk_conv2d_wgrad_x3_f32 (ups
 * 0 / 1 / 2).  Ops 1-5 ignore ksize, stride, pad, h_out and w_out; ops 4 and 5 ignore dtype.
 * Form ids: 0 matrix/auxiliary-wave kernel, 1 its pooled-dy form, 2 its upsample phase form, 3 its phase form with the roles
 * swapped, 4 its pair-operand form; 5 8x16-patch kernel, 6 / 7 halo kernel with 8x16 / 8x8 patches; 8 / 9 fp32 thin kernel with 4
 * input / 4 output channels; 10 / 11 general kernel fp32 / bf16, 12 double-buffered bf16 1x1; 13 split-product kernel, 14 / 15 its
 * phase forms for ups 1 / 2.  details (may be NULL): five ints -- dW tiles (the grid's x; forms 8 / 9: blocks), split-K parts
 * (per phase in the phase forms), patches per part (forms 10-12: pixels, 8 / 9: rows), number of kernel launches (4: one per
 * phase, tuning slot UPS_MERGE = 0; 2: deterministic mode's partial sums went through the workspace and an ordered reduce
 * follows), 1 when the form is memory-bound (name suffix " (HBM)").
 * vqk_conv_wgrad_form_name: the kernel's name for the event statistics, "?" for an unknown id. */
int vqk_conv_wgrad_plan(int op, int dtype, int n, int h_in, int w_in, int cin, int cout, int ksize, int stride, int pad, int ups,
                        int h_out, int w_out, int* details);
const char* vqk_conv_wgrad_form_name(int form, int dtype);
/* The 3x3 weight gradient of the two EDGE convs (one 16-byte chunk of channels on one side: the padded 3-channel image /
 * reconstruction; vqvae/modules/autoencoder.py:114 and :170), bf16: (cin, cout) = (8, 128) or (128, 8), h*w % 128 == 0 and
 * (w % 128 == 0 or 128 % w == 0).
 * dw[Cout][3][3][Cin] += the gradient; split-K partials go through the caller's workspace `ws` (>=
 * vqk_conv2d_wgrad_edge_ws_bytes() bytes) and are summed in a fixed order: no atomics, run-to-run deterministic.
 * VQK_ERR_SHAPE when not served (nothing launched: callers use vqk_conv2d_wgrad).
 * vqk_conv2d_wgrad_edge_serves: 1 when the three entry points below take the problem, else 0 (no device needed). */
int64_t vqk_conv2d_wgrad_edge_ws_bytes(void);
int vqk_conv2d_wgrad_edge_serves(int dtype, int n, int h, int w, int cin, int cout);
int vqk_conv2d_wgrad_edge(int dtype, const void* x, const void* dy, float* dw, void* ws, int64_t ws_bytes, int n, int h,
                          int w, int cin, int cout, const void* zeros, void* stream);
/* vqk_conv2d_wgrad_edge with the TRUE channel count of the thin side (thin_true in 1..8; 3 for the image / reconstruction): dw is
 * the parameter's own unpadded gradient -- [128][3][3][thin_true] for (cin, cout) = (8, 128), [thin_true][3][3][128] for (128, 8) --
 * the sums of the zero-padded channels are dropped.  thin_true = 8: vqk_conv2d_wgrad_edge. */
int vqk_conv2d_wgrad_edge_true(int dtype, const void* x, const void* dy, float* dw, void* ws, int64_t ws_bytes, int n, int h,
                               int w, int cin, int cout, int thin_true, const void* zeros, void* stream);
/* vqk_conv2d_wgrad_edge_true that also sums the bias gradient of the LAST conv ((cin, cout) = (128, 8); VQK_ERR_ARG otherwise):
 * db[c] += sum over pixels of dy[pixel][c] for c < thin_true, gathered from the kernel's own staged copy of dy (no second pass
 * over dy), one fp32 atomic per channel and block -- order-dependent in the last bits, so deterministic mode keeps vqk_colsum_lead.
 * db = NULL: vqk_conv2d_wgrad_edge_true.  dw is bit-identical either way. */
int vqk_conv2d_wgrad_edge_bias(int dtype, const void* x, const void* dy, float* dw, float* db, void* ws, int64_t ws_bytes, int n,
                               int h, int w, int cin, int cout, int thin_true, const void* zeros, void* stream);
/* The decoder's last conv (autoencoder.py:170): 3x3, stride 1, 'same', cin = 128 -> cout = 8 (the 3 image channels padded to
 * one 16-byte chunk), y = act(conv(x, w) + bias) with act 0 none / 1 tanh; bf16 in and out, h % 8 == 0, w % 32 == 0;
 * w: bf16 [8][3][3][128] (weight layout 0).  VQK_ERR_SHAPE when not served (nothing launched: callers use vqk_conv2d_fprop). */
int vqk_conv2d_thin_out(int dtype, const void* x, const void* w, const float* bias, void* y, int n, int h, int wd, int cin,
                        int cout, int act, const void* zeros, void* stream);
/* out[c] (+)= sum over rows of x[rows][c]  (bias gradients); out pre-zeroed. */
int vqk_colsum(int dtype, const void* x, int64_t rows, int c, float* out, void* stream);
/* out[i] += scale * sum_rows x[row][i] for the first c_out <= c columns only: `out` is the gradient of a bias whose layer carries
 * zero-padded output channels (the decoder's 3-channel head on 8) -- the sums go straight into the parameter's own (unpadded)
 * gradient; `scale` undoes a gain folded into x (the StyleGAN2 layers' runtime weight gain).  c <= 8192 (VQK_ERR_SHAPE above).
 * Deterministic mode: the block count is halved until the partial rows ([blocks][c] fp32) fit the armed workspace; a workspace
 * that cannot hold ONE partial row (c * 4 bytes) is a bad argument of vqk_set_deterministic: VQK_ERR_ARG, nothing launched. */
int vqk_colsum_lead(int dtype, const void* x, int64_t rows, int c, int c_out, float scale, float* out, void* stream);
/* elementwise fp32 -> dtype cast (weight shadow copies) */
int vqk_cast(const float* src, void* dst, int dtype, int64_t n, void* stream);

/* ---------------------------------------------------------------- GroupNorm + SiLU ----------
 * autoencoder.py:25-39: per (sample, group) mean and UNBIASED variance; y = (x-mu)*rstd*w + b,
 * optionally followed by SiLU.  stats[n][g] = {mean, rstd} fp32.  acc = N*G*2 doubles scratch (zeroed
 * by the caller). */
int vqk_gn_stats(int dtype, const void* x, int n, int64_t hw, int c, int groups, float eps,
                 double* acc, float* stats, void* stream);
int vqk_gn_apply(int dtype, const void* x, const float* stats, const float* w, const float* b, void* y,
                 int n, int64_t hw, int c, int groups, int silu, void* stream);
/* statistics + normalisation (+SiLU) as one call: two launches (sums; finalize folded into the apply pass), stats
 * are also stored for the backward.  ws = N*G*2 doubles of sums + N 8-byte counter slots (N*G*2+N doubles), ZERO on entry and
 * left ZERO on exit (the last block of each sample in the apply pass clears that sample's slots), so one persistent workspace per stream serves every call
 * with no memset in between. */
int vqk_gn_forward(int dtype, const void* x, const float* w, const float* b, void* y, float* stats, double* ws, int n,
                   int64_t hw, int c, int groups, float eps, int silu, void* stream);
/* the same when the sums of x are already in ws (vqk_conv2d_fprop_gnstats of the producing conv): one launch */
int vqk_gn_forward_presummed(int dtype, const void* x, const float* w, const float* b, void* y, float* stats, double* ws,
                             int n, int64_t hw, int c, int groups, float eps, int silu, void* stream);
/* deterministic mode: the producing conv (vqk_conv2d_fprop_gnstats / vqk_conv2d_ups_phase while vqk_set_deterministic is on)
 * left the sums as ONE SLOT PER 256-pixel TILE, parts[((n * G + g) * nblk + tile) * 2 + j], nblk = (conv-resolution H * W) / 256
 * (plain stores, no zero-on-entry protocol: `ws` handed to the conv is `parts`, >= N*G*nblk*2 doubles).  The slots are added in
 * a fixed order into sums[N*G*2] (scratch), then the apply pass runs as in vqk_gn_forward_presummed. */
int vqk_gn_forward_presummed_parts(int dtype, const void* x, const float* w, const float* b, void* y, float* stats,
                                   const double* parts, int nblk, double* sums, int n, int64_t hw, int c, int groups, float eps,
                                   int silu, void* stream);
/* vqk_gn_forward_presummed / _parts whose apply pass ALSO stores the 2x2 average of its input (the skip of a pooling ResBlock):
 * pooled[n][h/2][w/2][c] = ((x00 + x01) + (x10 + x11)) * pool_scale, bit for bit what vqk_pool2x2(x, pool_scale) stores, for one
 * quarter-size store instead of a pass of its own; y and stats are those of the unpooled call.  Blocks own whole row pairs.
 * VQK_ERR_SHAPE for an odd h or w (or a map beyond 2^30 pixels / 2^20 columns): callers then run the two launches. */
int vqk_gn_forward_presummed_pooled(int dtype, const void* x, const float* w, const float* b, void* y, float* stats, double* ws,
                                    int n, int h, int wd, int c, int groups, float eps, int silu, void* pooled, float pool_scale,
                                    void* stream);
int vqk_gn_forward_presummed_parts_pooled(int dtype, const void* x, const float* w, const float* b, void* y, float* stats,
                                          const double* parts, int nblk, double* sums, int n, int h, int wd, int c, int groups,
                                          float eps, int silu, void* pooled, float pool_scale, void* stream);
/* backward of y = act(GN(x)): needs x, stats, w, b and dy.  red = N*G*2+N doubles scratch with the vqk_gn_forward
 * workspace protocol (zero on entry, zero again on exit); dw/db [C] fp32 pre-zeroed (accumulated into).  accumulate != 0: dx += result; add != NULL: dx = result + add (the residual-branch
 * gradient of a ResBlock, fused instead of a separate add pass). */
int vqk_gn_backward(int dtype, const void* x, const float* stats, const float* w, const float* b, const void* dy,
                    void* dx, float* dw, float* db, double* red, int n, int64_t hw, int c, int groups, int silu,
                    int accumulate, const void* add, void* stream);
/* vqk_gn_backward / vqk_gn_backward_pooled_add (add_pooled != NULL) with the SIZE of the workspace stated.  With
 * ws_doubles >= N*G*2 + N + N*(C/32) the mid-size maps (H*W <= the GN_CLUSTER_MAX_HW slot, a multiple of 8 x 64 pixels in
 * bf16) run as ONE kernel: clusters of blocks per (sample, 32-channel slice) keep x and dy in registers, exchange their group
 * sums through the workspace (the extra N*(C/32) slots are the clusters' tickets) and apply from the registers -- x and dy are
 * read once.  Same workspace protocol (zero on entry, zero on exit); deterministic mode keeps the two-kernel form. */
int vqk_gn_backward_ws(int dtype, const void* x, const float* stats, const float* w, const float* b, const void* dy,
                       void* dx, float* dw, float* db, double* red, int64_t ws_doubles, int n, int h, int wd, int c, int groups,
                       int silu, int accumulate, const void* add, const void* add_pooled, float add_scale, void* stream);
/* The cluster form waits for its <= 8 partner blocks inside the kernel (an ordinary launch, no cooperative groups).  Forward
 * progress assumes that each XCD dispatches its share of a grid in block-index order (then the lowest waiting block's partners are
 * always resident or done -- csrc/norm.hip); the wait is BOUNDED (~0.2 s): a block that gives up is counted and falls through with
 * incomplete sums.  vqk_gn_cluster_timeouts reports the count (0 in a healthy run; synchronises the device).  A kernel killed
 * mid-way leaves sums / tickets dirty: re-zero the workspace.
 * CONCURRENCY RULE: the progress argument covers ONE cluster launch at a time per GPU.  Two of them in flight together (two streams, or
 * two processes sharing the device) can each occupy the slots the other's waiting blocks need -- measured: two ranks on one GPU, 600-870
 * timed-out blocks.  A caller that may run a second GroupNorm backward concurrently states a workspace WITHOUT the ticket region for it
 * (ws_doubles = N*G*2 + N: the two-kernel passes); the Python host gives the form to one host thread's models (ops.cluster_owner_ok);
 * processes that share a GPU set the GN_CLUSTER_MAX_HW slot to 0. */
int vqk_gn_cluster_timeouts(int* count);
/* vqk_gn_backward_ws (same-resolution addend) that also accumulates the per-channel sums of the dx it writes into
 * dx_colsum[C] (fp32): when x is the output of a conv with a bias, that is the conv's bias gradient -- no column-sum pass over
 * the gradient tensor.  Two-kernel form only; not in deterministic mode (VQK_ERR_ARG). */
int vqk_gn_backward_colsum(int dtype, const void* x, const float* stats, const float* w, const float* b, const void* dy,
                           void* dx, float* dw, float* db, double* red, int64_t ws_doubles, int n, int h, int wd, int c, int groups,
                           int silu, int accumulate, const void* add, float* dx_colsum, void* stream);
/* vqk_gn_backward with dx += add_scale * (add_pooled read at pixel (row/2, col/2)): the skip-branch gradient of a ResBlock
 * whose output went through a fused 2x2 average pool, still at half resolution ([N][h/2][wd/2][C]).  h * wd > 1024. */
int vqk_gn_backward_pooled_add(int dtype, const void* x, const float* stats, const float* w, const float* b, const void* dy,
                               void* dx, float* dw, float* db, double* red, int n, int h, int wd, int c, int groups, int silu,
                               const void* add_pooled, float add_scale, void* stream);

/* ---------------------------------------------------------------- pooling / pointwise -------
 * 2x2 stride-2 pooling with a scale: scale = 0.25 is avg_pool2d (autoencoder.py:89-91), scale = 1 is the
 * backward of the nearest x2 upsample.  x [N][H][W][C] -> y [N][H/2][W/2][C]. */
int vqk_pool2x2(int dtype, const void* x, void* y, int n, int h, int w, int c, float scale, void* stream);
/* y[N][2H][2W][C] = scale * x[N][H][W][C] replicated (backward of avg-pool with scale = 0.25). */
int vqk_unpool2x2(int dtype, const void* x, void* y, int n, int h, int w, int c, float scale, void* stream);
/* images [N][3][H][W] fp32 in [0,1] (NCHW) -> clamp, (x-0.5)/0.5, NHWC with C padded to cpad (zeros),
 * written as `dtype` and (optionally) as an fp32 NHWC-3 target for the loss.  base_autoencoder.py:31-50. */
int vqk_preprocess(const float* images, void* x_pad, int dtype, float* target, int n, int h, int w, int cpad,
                   void* stream);
/* The same with the reference's training augmentation (base_autoencoder.py:20-22: RandomResizedCrop(scale .7-1, ratio 1)
 * + RandomHorizontalFlip, per sample) fused in front: box[N][4] = {x0, y0, w, h} of the crop in source pixels (resampled
 * to H x W, bilinear, corner-aligned), flip[N] != 0 mirrors the output.  The random draws are the caller's (device
 * tensors: no host sync); the kornia generator itself is not in the reference tree, so its exact stream is unpinned. */
int vqk_augment_preprocess(const float* images, const float* box, const int32_t* flip, void* x_pad, int dtype, float* target,
                           int n, int h, int w, int cpad, void* stream);
/* loss[0] += sum (recon - target)^2 over n elements (recon dtype given; target fp32).  Up to 32 blocks (65536 elements) add their
 * partials to loss[0] by fp32 atomics.  Larger sums, given a stream scratch of >= 8 KiB (vqk_set_scratch), store the block partials
 * there and a second one-block launch adds them in block order in double and rounds once: the same bits every run, ~1e-7 relative
 * (2048 atomics in arrival order are a random walk of up to 2.4e-6 relative at 4M elements).  Without a scratch: the atomics.
 * vqk_pair_stats sums its out5[0] the same way. */
int vqk_sse(int dtype, const void* recon, const float* target, int64_t n, float* loss, void* stream);
/* d = s * gscale * 2 (recon - target) * (through_tanh ? 1 - recon^2 : 1), s = *gscale_dev (NULL = 1)
 * (MSE backward, optionally through the decoder's tanh head; model.py:272, autoencoder.py:179) */
int vqk_mse_tanh_backward(int dtype, const void* recon, const float* target, int64_t n, float gscale,
                          const float* gscale_dev, int through_tanh, void* d, void* stream);
/* dx = dy * (1 - y^2) */
int vqk_tanh_backward(int dtype, const void* dy, const void* y, void* dx, int64_t n, void* stream);
/* Test-loop metrics on [0,1] NCHW fp32 images (vqvae/model.py:491-553; torchmetrics MeanSquaredError, PeakSignalNoiseRatio,
 * StructuralSimilarityIndexMeasure -- the library is not in the reference tree, its published algorithm is restated).
 * pair_stats: out5[0] += sum (pred - target)^2; out5[1] / out5[2] = running min / max of target, out5[3] / out5[4] of
 * pred (initialise to +inf / -inf).  ssim_sum: out[img] += sum over channels and the valid (h-k+1) x (w-k+1) region of the
 * SSIM map with window `window` [k*k] (k = 11 or 7), c1 = (k1 R)^2, c2 = (k2 R)^2, R = max(pred range, target range) read
 * from a pair_stats record of the same batch (`stats5`, device memory). */
int vqk_pair_stats(const float* pred, const float* target, int64_t n, float* out5, void* stream);
int vqk_ssim_sum(const float* pred, const float* target, int n, int c, int h, int w, const float* window, int ksize,
                 const float* stats5, float k1, float k2, float* out, void* stream);
/* generic elementwise: y = a*x + b*y2 (y2 optional) -- residual adds in backward */
int vqk_axpby(int dtype, const void* x, const void* y2, void* y, float a, float b, int64_t n, void* stream);

/* ---------------------------------------------------------------- optimizer ----------------
 * AdamW over a flat fp32 arena (model.py:428; torch.optim.AdamW semantics, decoupled decay).
 * seg_end[i] (exclusive, element index) / seg_wd[i]: weight decay per contiguous segment;
 * grad_scale multiplies g first (1/world after a sum all-reduce).  If shadow != NULL a bf16 copy of the
 * updated parameters is written in the same pass. */
int vqk_adamw(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end, const float* seg_wd,
              int nseg, float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* shadow,
              void* stream);
/* Guarded optimizer step: the decision "skip a step whose gradients hold an Inf / NaN" (torch.amp.GradScaler's rule) and
 * "scale the gradients so that their global norm is at most max_norm" (torch.nn.utils.clip_grad_norm_) is taken AND obeyed on
 * the device, without the host waiting for it.  Per step, in stream order: vqk_arena_stats -> vqk_step_guard -> vqk_adamw_guarded.
 * None of the three allocates or synchronises; all can be captured.
 *
 * vqk_step_guard: one launch of one wave.  stats_row: a device {sum x^2, max |x|, nonfinite} row of doubles as vqk_arena_stats
 * writes it (the row "all groups", taken at scale = grad_scale).  apply = !(skip_nonfinite && nonfinite > 0);
 * coef = max_norm > 0 ? min(1, max_norm / (sqrt(sum x^2) + 1e-6)) : 1 in fp64 (the norm over the FINITE elements);
 * control block (VQK_GUARD_CTRL_BYTES, 16-byte aligned) = {int32 apply, float eff_scale = (float)((double)grad_scale * coef),
 * float step_size = (float)((double)lr / bc1(t)), float inv_sqrt_bc2 = (float)(1 / sqrt(bc2(t)))} with t = applied + 1: the
 * pair vqk_adamw derives on the host for step t, so a skipped step does not advance the bias correction.  bc1 / bc2 come from
 * bias_table[bias_len][2] (device doubles, entry t - 1 = {1 - beta1^t, 1 - beta2^t}, t clamped to bias_len), filled on the host by
 * vqk_adamw_bias_table with vqk_adamw's own pow() -- the device's pow need not round like the host's.
 * State block: VQK_GUARD_STATE_DOUBLES doubles (counts are exact integers), indexed by the VQK_GUARD_* names below; the caller
 * resets it to zeros with COEF_MIN = 1.  CLIPPED, COEF_SUM and COEF_MIN cover applied steps only; LAST_NORM is written by every
 * launch.  One lane owns both blocks and launches are stream-ordered: every field is reproducible bit for bit.
 *
 * vqk_adamw_bias_table: host only.  Returns T, the first step at which 1 - beta^t == 1.0 for both betas (from there on the pair
 * is constant), and fills min(T, capacity) entries when table != NULL; -1 for betas outside [0, 1) or T > VQK_GUARD_TABLE_MAX.
 *
 * vqk_adamw_guarded: vqk_adamw with step_size, inv_sqrt_bc2, the gradient scale and the apply flag read from `control`.  With
 * apply == 0 every block returns after reading the control block: p / m / v / shadow keep their bits.  With apply == 1 the result
 * is bit-identical to vqk_adamw(step = t, grad_scale = eff_scale): the same device function.
 * Both validate before any launch (VQK_ERR_ARG: NULL pointers, nseg <= 0, m == NULL with beta1 != 0, non-finite max_norm / lr /
 * grad_scale, bias_len < 1). */
#define VQK_GUARD_CTRL_BYTES 16
#define VQK_GUARD_STATE_DOUBLES 8
#define VQK_GUARD_APPLIED 0        /* steps taken */
#define VQK_GUARD_SKIPPED 1        /* steps left out */
#define VQK_GUARD_CLIPPED 2        /* applied steps with coef < 1 */
#define VQK_GUARD_SKIP_RUN 3       /* current run of consecutive skips */
#define VQK_GUARD_MAX_SKIP_RUN 4   /* longest such run */
#define VQK_GUARD_COEF_SUM 5       /* sum of coef over applied steps */
#define VQK_GUARD_COEF_MIN 6       /* minimum of coef over applied steps (reset value 1) */
#define VQK_GUARD_LAST_NORM 7      /* sqrt(sum x^2) of the last launch */
#define VQK_GUARD_TABLE_MAX (1 << 22)
int64_t vqk_adamw_bias_table(float beta1, float beta2, double* table, int64_t capacity);
int vqk_step_guard(const double* stats_row, int skip_nonfinite, double max_norm, float lr, float grad_scale,
                   const double* bias_table, int64_t bias_len, double* state, void* control, void* stream);
int vqk_adamw_guarded(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end, const float* seg_wd,
                      int nseg, float lr, float beta1, float beta2, float eps, const void* control, void* shadow,
                      void* stream);

/* ---------------------------------------------------------------- StyleGAN2 plugin ops ------
 * Same argument meaning as the reference's pybind functions (bias_act.cpp:32, upfirdn2d.cpp:16), with raw
 * pointers instead of tensors; NULL encodes the reference's "empty tensor".  x is contiguous NCHW fp32
 * with `inner` = elements per channel step (H*W) and `channels` = size of `dim`.
 * act: 1 linear, 3 lrelu (the reference's cuda_idx).  grad: 0 forward, 1 first-order backward. */
int vqk_bias_act(const float* x, const float* b, const float* xref, const float* yref, const float* dy, float* y,
                 int64_t numel, int64_t inner, int channels, int grad, int act, float alpha, float gain, float clamp,
                 void* stream);
int vqk_upfirdn2d(const float* x, const float* f, float* y, int n, int c, int in_h, int in_w, int fh, int fw,
                  int upx, int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip,
                  float gain, int out_h, int out_w, void* stream);

/* ---------------------------------------------------------------- VQ-GAN loss path (NHWC) ---
 * dx = dy * scale * act'(y), act' recovered from the saved OUTPUT y (bias_act.cu grad=1 semantics): 1 tanh, 2 relu,
 * 3 leaky-relu(0.2), 0 plain scaling.  `scale` carries the activation gain and the runtime weight gain. */
int vqk_act_backward(int dtype, const void* dy, const void* y, void* dx, int64_t n, int act, float scale, void* stream);
/* the same on [rows][c] tensors, plus colsum[c] += the column sums of dx (as stored): the bias gradient of the conv whose
 * output y is, without a second pass over dx (bias_act.py:196: db = dx summed over every dim but the channel).  c a whole
 * number of 16-byte vectors, at most 256 of them. */
int vqk_act_backward_colsum(int dtype, const void* dy, const void* y, void* dx, int64_t rows, int c, int act, float scale,
                            float* colsum, void* stream);
/* the same with the column sums scaled before they are ADDED to colsum (colsum += colsum_scale * sum_rows dx): the bias gradient
 * goes straight into an optimizer's gradient arena when dx carries a folded weight gain (colsum_scale = 1 / gain) */
int vqk_act_backward_colsum_scaled(int dtype, const void* dy, const void* y, void* dx, int64_t rows, int c, int act, float scale,
                                   float colsum_scale, float* colsum, void* stream);
/* upfirdn2d (upfirdn2d.cpp:16 argument meaning) on NHWC tensors of `dtype`, C a whole 16-byte chunk. */
int vqk_upfirdn2d_nhwc(int dtype, const void* x, const float* f, void* y, int n, int h, int w, int c, int fh, int fw,
                       int upx, int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip,
                       float gain, int out_h, int out_w, void* stream);
/* The backward of "relu / leaky-relu, then a 4x4 FIR blur" as ONE pass (up = down = 1; the reference runs bias_act's gradient
 * after upfirdn2d's, discriminator.py:104-120 / conv2d_resample.py:119): out = gain * act'(y_act) * upfirdn2d(x, f, pad, flip),
 * the slope taken from the sign of the activated tensor y_act [N][out_h][out_w][C] (act 2 = relu, 3 = leaky relu 0.2).
 * C a multiple of 8 sixteen-byte slots; VQK_ERR_SHAPE otherwise (callers run vqk_upfirdn2d_nhwc + vqk_act_backward). */
int vqk_upfirdn2d_act_backward(int dtype, const void* x, const float* f, const void* y_act, void* out, int n, int h, int w, int c,
                                int padx0, int padx1, int pady0, int pady1, int flip, float gain, int act, int out_h, int out_w,
                                void* stream);
/* 2x2/stride-2 max pool: backward = 0: out[N][H/2][W/2][C] = max ; backward = 1: out[N][H][W][C] = dy routed to the
 * first maximum of each window (x is the forward input). */
int vqk_maxpool2x2(int dtype, const void* x, const void* dy, void* out, int n, int h, int w, int c, int backward,
                   void* stream);
/* y[pix][c] = x[pix][c] * scale[c] + shift[c]   (LPIPS z-score, networks.py:51-52; shift may be NULL) */
int vqk_channel_affine(int dtype, const void* x, const float* scale, const float* shift, void* y, int64_t npix, int c,
                       void* stream);
/* LPIPS tap (lpips.py:31-38, utils.py:6-8): dfy == NULL: out[n] += (1/hw) sum_pix sum_c lin[c] (fx/(|fx|+1e-10) -
 * fy/(|fy|+1e-10))^2 (out pre-zeroed);  dfy != NULL: gradient w.r.t. fy for the upstream gradient gscale * gout[image]
 * (gout: n floats, one per image; NULL = 1). */
int vqk_lpips_tap(int dtype, const void* fx, const void* fy, const float* lin, int n, int64_t hw, int c, float* out,
                  const float* gout, float gscale, void* dfy, void* stream);
/* minibatch-stddev layer (discriminator.py:271-293), F = 1 feature: forward writes out[N][hw][cpad] = [x | stat | 0..]
 * and stat[N/group]; backward writes dx[N][hw][c] from dy[N][hw][cpad]. */
int vqk_mbstd(int dtype, const void* x, const void* dy, void* out, float* stat, int n, int64_t hw, int c, int cpad,
              int group, int backward, void* stream);
/* Second-order piece of the layer (R1 differentiates the backward pass): given v = cotangent of the first backward's
 * dx, writes ddy[N][hw][cpad] (cotangent of dy) and dxx[N][hw][c] (cotangent of x). */
int vqk_mbstd_double_backward(int dtype, const void* x, const void* dy, const void* v, void* ddy, void* dxx, int n,
                               int64_t hw, int c, int cpad, int group, void* stream);
/* out[0] += sum |target - recon| ;  d (+)= s * (a1 sign(recon-target) + a2 * 2 (recon-target)), s = *gscale_dev */
int vqk_l1_sum(int dtype, const void* recon, const float* target, int64_t n, float* out, void* stream);
int vqk_l1l2_backward(int dtype, const void* recon, const float* target, int64_t n, float a1, float a2,
                      const float* gscale_dev, void* d, int accumulate, void* stream);
/* loss.py:11-51 on [n] logits.  mode 0 hinge / 1 non-saturating; which 0 generator_loss(fake) / 1
 * discriminator_loss(real, fake).  loss[0] = value; dreal/dfake (optional) = gradients times *gscale_dev. */
int vqk_gan_loss(const float* logits_real, const float* logits_fake, int n, int mode, int which, float* loss,
                 float* dreal, float* dfake, const float* gscale_dev, void* stream);

/* ---------------------------------------------------------------- FID Inception-v3 (csrc/fid.hip, fid.py) ----------
 * fp32 storage, NHWC, products exact fp32 (v_mfma_f32_32x32x2_f32).  VQK_ERR_SHAPE for unsupported parameters, nothing
 * launched.
 * preprocess: x = a [n][3][h][w] view with element strides (sn, sc, sh, sw); y[n][299][299][4] = (resize(q) - 128) / 128,
 *   q = trunc(clamp(x, 0, 1) * 255.999f), resize = TF1 bilinear (src = dst * in / 299, no half-pixel offset); channel 3 = 0. */
int vqk_fid_preprocess(const float* x, int n, int h, int w, int64_t sn, int64_t sc, int64_t sh, int64_t sw, float* y,
                       void* stream);
/* y[pix][c_off + co] = relu(conv(x, w)[pix][co] + bias[co]) for co < cout, pixel stride c_total (a slice of a channel
 * concat; nothing outside the slice is written).  x[n][h][wd][cin], w[cout][kh][kw][cin] (KRSC), cin % 4 == 0,
 * 1 <= kh, kw <= 7, stride 1 or 2, 0 <= ph < kh, 0 <= pw < kw, oh / ow = the conv's output size. */
int vqk_fid_conv(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int cin, int cout, int kh,
                 int kw, int stride, int ph, int pw, int oh, int ow, int c_total, int c_off, void* stream);
/* 3 x 3 pool of x[n][h][w][c] into channels [c_off, c_off + c) of y (pixel stride c_total); mode 0 max (padding = -inf),
 * mode 1 average over the in-bounds taps (count_include_pad=False); stride 1 or 2, pad 0 or 1; c, c_off, c_total % 4 == 0. */
int vqk_fid_pool(const float* x, float* y, int n, int h, int w, int c, int mode, int stride, int pad, int oh, int ow, int c_total,
                 int c_off, void* stream);
/* y[n][c] = mean over the hw pixels of x[n][hw][c] */
int vqk_fid_mean(const float* x, float* y, int n, int hw, int c, void* stream);
/* sum[d] += sum_r f[r][:], gram[d][d] += f^T f in fp64 from f[n][d] fp32; one thread per output element, rows in order: bit-
 * reproducible, and several calls equal one call on the concatenated rows. */
int vqk_fid_stats(const float* f, int n, int d, double* sum, double* gram, void* stream);

/* ---------------------------------------------------------------- dataset ingest (csrc/ingest.hip, data.py) --------
 * The device half of the reference's standard loader (data/datasets.py:16,26: PIL decode -> ToTensor() -> Resize((S,S),
 * antialias=True)): host threads decode to uint8, ONE launch turns a ragged batch into the tensor the steps take.
 * pixels: one packed device buffer (4-byte aligned, pixels_bytes long) of uint8 HWC RGB images of any sizes; image i of the
 * OUTPUT is described by desc[i] (several entries may name the same source).  out: fp32 NCHW, out[i * out_batch_stride +
 * c * out_h * out_w + y * out_w + x] in [0,1], out_batch_stride >= 3 * out_h * out_w elements (a slice of a larger tensor is
 * written in place; nothing outside the n images' 3 * out_h * out_w elements is touched).
 * Arithmetic (ATen's antialiased bilinear, the kernel torchvision's Resize(antialias=True) runs on tensors), per axis for a box
 * of length L resampled to S outputs:
 *     scale = L / S;  support = max(scale, 1);  c = scale * (i + 0.5)
 *     lo = max(0, (int)(c - support + 0.5));  hi = min(L, (int)(c + support + 0.5))
 *     w_j = max(0, 1 - |(j - c + 0.5) / support|), j in [lo, hi), normalised to sum 1
 * applied separably (columns, then rows) to float(u8) / 255.0f; no rounding to uint8 in between; flip != 0 mirrors the output
 * columns.  Coordinates and weights are computed in fp64 and rounded to fp32 per tap, sums are fp32 in ascending source order:
 * bit-reproducible, and at scale == 1 bit-identical to float(u8) / 255.0f.
 * desc_host and desc_dev are the SAME table in host and in device memory (8-byte aligned): the host copy is checked before the
 * launch, the kernel reads the device copy.  Supported: n >= 1, source sides 1..16384, out_h / out_w 1..4096, any ratio up or
 * down, stride >= 3 * w, the box inside the image, every image inside [0, pixels_bytes); otherwise VQK_ERR_SHAPE and nothing
 * is launched.  Allocates nothing, never synchronises (graph-capturable). */
#define VQK_INGEST_MAX_SIDE 16384
#define VQK_INGEST_MAX_OUT 4096
typedef struct vqk_ingest_desc {
    int64_t offset;             /* byte offset of the image's first pixel in `pixels` */
    int32_t h, w;               /* source size in pixels */
    int32_t stride;             /* bytes between source rows (>= 3 * w) */
    int32_t x0, y0, bw, bh;     /* crop box in whole source pixels, inside the image */
    int32_t flip;               /* != 0: mirror the output columns */
} vqk_ingest_desc;              /* 40 bytes */
int vqk_ingest_u8(const void* pixels, int64_t pixels_bytes, const vqk_ingest_desc* desc_host, const vqk_ingest_desc* desc_dev,
                  int n, int out_h, int out_w, int64_t out_batch_stride, float* out, void* stream);

/* ---------------------------------------------------------------- image egress (csrc/egress.hip, imagelog.py) --------
 * The counterpart of the ingest: device image tensors out as uint8 HWC RGB, laid out as torchvision's make_grid documents it
 * (the reference's log_reconstructions, vqvae/model.py:442-456, builds its panel with make_grid(nrow=b)).  ONE launch, one pass.
 * src: n images of h x w, fp32 (VQK_F32) or bf16 (VQK_BF16), element (i, ch, y, x) at src[i * stride_n + ch * stride_c +
 * y * stride_y + x * stride_x] (strides in ELEMENTS): the padded NHWC reconstruction, the NHWC target and a plain NCHW batch --
 * or a slice of one -- are read in place.  c >= 3 is the number of channels that exist at each pixel; only channels 0..2 are
 * read (a pixel with contiguous channels, c >= 4 and 16-byte (fp32) / 8-byte (bf16) aligned pixels is fetched as one vector, the
 * fourth element dropped).
 * Quantisation, bit-exact in fp32, every operation rounded separately (no FMA); bf16 is widened exactly first:
 *     VQK_RANGE_SYM  (the model's (-1,1)):  t = clip(x * 0.5f + 0.5f, 0, 1)
 *     VQK_RANGE_UNIT ([0,1]):               t = clip(x, 0, 1)
 *     q = (uint8) floorf(t * 255.0f + 0.5f)            -- the rule of torchvision.utils.save_image
 * -Inf gives 0, +Inf gives 255, NaN gives 0.
 * Layout: the canvas is (rows * (h + pad) + pad) x (cols * (w + pad) + pad) pixels, 3 bytes each, rows contiguous.  Image k goes
 * to cell (row0 + k / cols, k % cols); a cell's top-left pixel is (pad + cell_y * (h + pad), pad + cell_x * (w + pad)).  A call
 * writes EVERY byte of the canvas rows [row0 * (h + pad), (row0 + ceil(n / cols)) * (h + pad)) -- its images, the padding
 * around them and the cells it leaves empty, as pad_value -- and, when its last cell row is the canvas's last, the closing pad
 * rows too; it writes nothing else.  Calls whose cell rows tile 0..rows-1 therefore define the whole canvas: no memset.
 * pad == 0, cols == 1, rows == n is the plain stack of n images [n][h][w][3].  The canvas pointer needs no alignment.
 * VQK_ERR_SHAPE: n < 1, c < 3, h / w outside 1..4096, pad outside 0..4096, pad_value outside 0..255, rows / cols < 1, canvas
 * bytes >= 2^31, cell rows outside the canvas, an unknown dtype or value range; VQK_ERR_ARG: NULL pointers; VQK_ERR_ALIGN: src
 * not aligned to its element.  Allocates nothing, never synchronises (graph-capturable).
 * vqk_egress_canvas_bytes: the canvas size in bytes, or -1 where vqk_egress_u8 would refuse the geometry. */
#define VQK_EGRESS_MAX_SIDE 4096
#define VQK_RANGE_UNIT 0
#define VQK_RANGE_SYM 1
int64_t vqk_egress_canvas_bytes(int h, int w, int rows, int cols, int pad);
int vqk_egress_u8(int dtype, const void* src, int n, int c, int h, int w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                  int64_t stride_x, int value_range, uint8_t* canvas, int rows, int cols, int row0, int pad, int pad_value,
                  void* stream);

/* ---------------------------------------------------------------- running statistics (csrc/runstats.hip, scalarlog.py) --------
 * The device half of the scalar log: what the reference hands to self.log(..., on_epoch=True, sync_dist=True) (vqvae/model.py:
 * 229-230, :277-286, :342-348, :365-366) is averaged over the epoch without a host synchronisation per step.  Both calls
 * allocate nothing, never synchronise and can be captured.
 * vqk_scalar_accum: n <= VQK_SCALAR_MAX device scalars into epoch accumulators, ONE launch.  src / dtype / weight / slot are
 * HOST arrays of n entries: src[k] a device pointer to one fp32 (VQK_F32) or bf16 (VQK_BF16) value -- the pointers travel as kernel
 * arguments, no device table --, weight[k] an integer in [0, 2^20) (the batch size in validation, 1 in training), slot[k] in
 * [0, nslots) the accumulator it goes to, no slot twice in one call.  acc: nslots x VQK_SCALAR_SLOT_DOUBLES doubles on the device,
 * slot = {sum += (double)x * w, wsum += w, last = x, min, max, nonfinite += !isfinite(x), calls += 1, reserved}.  A non-finite x
 * enters `sum` like any other (the mean turns NaN) and is counted; min / max skip NaN.  The caller resets a slot to
 * {0, 0, any, +Inf, -Inf, 0, 0, 0}.  One thread owns one slot and launches are ordered by the stream: `sum` is a fixed-order fp64
 * sum with exact products, bit-identical to a float64 host loop over the same values. */
#define VQK_SCALAR_MAX 16
#define VQK_SCALAR_SLOT_DOUBLES 8
int vqk_scalar_accum(const void* const* src, const int* dtype, const double* weight, const int* slot, int n, double* acc,
                     int nslots, void* stream);
/* vqk_arena_stats: one read-only pass over a FlatAdamW gradient arena g[numel] (fp32) before the optimizer step.  seg_end[nseg]:
 * the arena's ascending segment ends (the table vqk_adamw takes); seg_group[nseg]: a group id in [0, ngroups) per segment, or -1
 * for segments that belong to no group (the alignment padding: its elements never reach a result).  With x = (double)g *
 * (double)scale (exact; scale = the optimizer's grad_scale, finite) the step's result is out[ngroups + 1][3] = {sum of x^2 over the
 * finite x, max |x| over the finite x, the count of non-finite elements} per group and, in row ngroups, for all groups together
 * (the groups' rows combined in id order).  Everything accumulates in fp64: per thread, per wave by shuffles, per block in LDS,
 * the per-block partials in `ws`; a second one-block launch adds them in index order -- no float atomics, the same bits every run.
 * acc (optional): epoch accumulators [ngroups + 1][VQK_ARENA_ACC_DOUBLES] = {sum of norms, max norm, max of max |x|, sum of
 * nonfinite, steps}, norm = sqrt(sum x^2), zero-initialised by the caller.  ws: >= vqk_arena_stats_ws_bytes(numel, ngroups) bytes
 * (-1 for an unsupported size), 8-byte aligned, need not be initialised.  ngroups <= VQK_ARENA_MAX_GROUPS. */
#define VQK_ARENA_MAX_GROUPS 8
#define VQK_ARENA_ACC_DOUBLES 5
int64_t vqk_arena_stats_ws_bytes(int64_t numel, int ngroups);
int vqk_arena_stats(const float* g, int64_t numel, const int64_t* seg_end, const int32_t* seg_group, int nseg, int ngroups,
                    float scale, void* ws, int64_t ws_bytes, double* out, double* acc, void* stream);
/* ---------------------------------------------------------------- PatchGAN discriminator ---------
 * csrc/patchgan.hip: the layers of the n-layer PatchGAN (Isola et al. 2017): 4x4 convs with zero padding 1 and stride 1 or 2, and
 * BatchNorm (+ LeakyReLU 0.2).  Activations are NHWC `dtype` tensors whose channel count is a whole 16-byte chunk (4 fp32 / 8 bf16):
 * x[n][h][w][cin], y / dy[n][ho][wo][co_ld] with ho = (h + 2 - 4) / stride + 1 (floor) and co_ld = cout rounded up to a chunk; the
 * channels cout .. co_ld - 1 of y are written as zeros.  The weight is the fp32 master w[cout][4][4][cin_w], cin_w <= cin (the
 * 3-channel image arrives zero-padded to cin = one chunk), read in place: VQK_F32 multiplies exactly (fp32 MFMA), VQK_BF16 rounds
 * the weights to nearest even as they are staged and multiplies bf16 with fp32 accumulation.  Served: stride in {1, 2}, h, w >= 2,
 * cin, cout <= 4096, n h w < 2^30 (VQK_ERR_SHAPE otherwise, nothing launched); activations and workspaces 16-byte aligned
 * (VQK_ERR_ALIGN).  No call allocates or synchronises; no kernel uses float atomics: every output has the same bits on every run.
 * fprop: y = act(conv(x, w) + bias), bias[cout] fp32 or NULL, lrelu != 0: LeakyReLU(0.2).
 * dgrad: dx[n][h][w][cin] = conv^T(dy, w): stride 1 as the flipped 4x4 conv, stride 2 as four input-parity phases of 2x2 taps each.
 *   EVERY element of dx is written (channels cin_w .. cin - 1 and the rows / columns no output pixel reads get zeros).
 * wgrad: dw[co][kh][kw][ci] (+)= scale * sum_p dy[p][co] x[p s + k - 1][ci] (accumulate != 0: +=).  The pixels are split into
 *   vqk_conv4x4_wgrad_plan(...) partials (a function of the shape only) kept in ws (>= vqk_conv4x4_wgrad_ws_bytes(...) bytes:
 *   VQK_ERR_WORKSPACE); a second launch adds them in split order into dw.  Both queries return VQK_ERR_SHAPE for an unserved shape. */
int vqk_conv4x4_fprop(int dtype, const void* x, const float* w, const float* bias, void* y, int n, int h, int wd, int cin, int cin_w,
                      int cout, int co_ld, int stride, int lrelu, void* stream);
int vqk_conv4x4_dgrad(int dtype, const void* dy, const float* w, void* dx, int n, int h, int wd, int cin, int cin_w, int cout, int co_ld,
                      int stride, void* stream);
int vqk_conv4x4_wgrad_plan(int n, int h, int wd, int cin, int cin_w, int cout, int stride);
int64_t vqk_conv4x4_wgrad_ws_bytes(int n, int h, int wd, int cin, int cin_w, int cout, int stride);
int vqk_conv4x4_wgrad(int dtype, const void* x, const void* dy, float* dw, int n, int h, int wd, int cin, int cin_w, int cout, int co_ld,
                      int stride, float scale, int accumulate, void* ws, int64_t ws_bytes, void* stream);
/* bias gradient: db[k] (+)= scale * sum_rows dy[row][k], k < cout, dy[rows][co_ld]; per-block fp64 partials in ws (>=
 * vqk_bn_ws_bytes(rows, co_ld) bytes) added in block order by a second launch. */
int vqk_conv4x4_bgrad(int dtype, const void* dy, float* db, int64_t rows, int co_ld, int cout, float scale, int accumulate, void* ws,
                      int64_t ws_bytes, void* stream);
/* BatchNorm over x[rows][c] (rows = N H W of an NHWC tensor, c a whole chunk, c / chunk <= 256), gamma / beta / statistics fp32.
 * forward, training != 0: per-channel mean and biased variance from fp64 sums (per-block partials in ws, added in block order by a
 * one-pass finish: no atomics), mean[c] and rstd[c] = 1 / sqrt(var + eps) saved; the same launch sequence updates running_mean /
 * running_var (optional) with `momentum` and the UNBIASED variance, and adds 1 to *num_batches_tracked (optional, device int64), so a
 * captured graph carries the update.  rows == 1 is VQK_ERR_SHAPE (no variance).  training == 0: running_mean / running_var are used,
 * nothing is saved or updated, ws is not read.  y = act(gamma xhat + beta), lrelu != 0: LeakyReLU(0.2).
 * backward (of the training-mode forward): g = dy through the LeakyReLU mask (recomputed from x: the pre-activation's sign);
 * sum g and sum g xhat per channel in the same ordered two-stage form; dx = gamma rstd (g - mean(g) - xhat mean(g xhat));
 * dgamma / dbeta (each optional: NULL = not wanted) are written, or added to when accumulate != 0.
 * ws: >= vqk_bn_ws_bytes(rows, c) bytes (VQK_ERR_SHAPE as a negative size for an unserved shape), serves forward and backward. */
int64_t vqk_bn_ws_bytes(int64_t rows, int c);
int vqk_bn_forward(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                   float* running_mean, float* running_var, int64_t* num_batches_tracked, int64_t rows, int c, float eps, float momentum,
                   int training, int lrelu, void* ws, int64_t ws_bytes, void* stream);
int vqk_bn_backward(int dtype, const void* x, const void* dy, const float* gamma, const float* beta, const float* mean, const float* rstd,
                    void* dx, float* dgamma, float* dbeta, int accumulate, int64_t rows, int c, int lrelu, void* ws, int64_t ws_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQK_H_ */
