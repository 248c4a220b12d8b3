"""Quantizer operators over the vqk C-ABI (Standard / EMA lookup, Entropy and Gumbel quantizers, EMA statistics): the autograd
Functions behind ``modules/vector_quantizers.py``.  Private part of :mod:`ops` (imported at the end of ``ops.py``, which re-exports
every name): shared infrastructure -- stream / workspace contexts, kernel-event timing, the operand cache, the switches tests flip
through ``ops.X = ...`` -- is reached through ``core``."""
from __future__ import annotations

import weakref

import torch

from . import _native
from . import ops as core

# ------------------------------------------------------------------------------------------------------
# vector quantizer
# ------------------------------------------------------------------------------------------------------
_VQ_WS: dict = {}


def _vq_filter_ws(device, k: int, d: int) -> torch.Tensor:
    core._stream()
    key = core._wkey(device) + (k, d)
    ws = _VQ_WS.get(key)
    if ws is None:
        ws = _VQ_WS[key] = torch.empty(_native.lib().vqk_vq_filter_ws_bytes(k, d), dtype=torch.uint8, device=device)
    return ws


class _VQPrep:
    __slots__ = ('wref', 'ws', 'stamp', 'k', 'd')


_VQ_PREP: dict = {}             # data_ptr of the codebook -> _VQPrep: what vqk_vq_prepare_f32 derived from it
# every table of prepared workspaces refresh_vq_prepared keeps current: (data_ptr -> _VQPrep, prepare(ent, codebook)); the
# cosine quantizer's (_ops_cos.py) registers itself here
_PREP_TABLES: list = []


def _vq_prepare_now(ent, cb) -> None:
    _native.check(_native.lib().vqk_vq_prepare_f32(cb.data_ptr(), ent.k, ent.d, ent.ws.data_ptr(), ent.ws.numel(), core._stream()),
                  'vq_prepare')


_PREP_TABLES.append((_VQ_PREP, _vq_prepare_now))


def prepared_ws(codebook, table: dict, served: bool, ws_bytes, prepare) -> torch.Tensor | None:
    """The cache frame of :func:`vq_prepared` and ``cos_prepared``: the workspace ``prepare(ent, codebook)`` derives from
    ``codebook`` [K, D], ``ws_bytes(k, d)`` bytes, kept in ``table`` under the codebook's data_ptr.  Built when the codebook
    CHANGES, not per step: the entry is stamped like the packed conv operands (in-place version + generation of the owning
    FlatAdamW), refreshed by :func:`repack_owned` right after the AdamW kernel and by :func:`ema_apply` after the EMA update
    (``refresh_vq_prepared`` walks every table of ``_PREP_TABLES``), so a captured step holds no prepare launch.
    None: ``served`` is false."""
    if not served:
        return None
    k, d = codebook.shape
    cb = codebook.detach()
    ent = table.get(cb.data_ptr())
    if ent is not None and (ent.wref() is not codebook or ent.k != k or ent.d != d):
        ent = None
    stamp = core._pack_stamp(codebook)
    if ent is None:
        ent = _VQPrep()
        ent.wref, ent.k, ent.d, ent.stamp = weakref.ref(codebook), k, d, None
        ent.ws = torch.empty(ws_bytes(k, d), dtype=torch.uint8, device=cb.device)
        table[cb.data_ptr()] = ent
    if ent.stamp != stamp:
        prepare(ent, cb)
        ent.stamp = stamp
    return ent.ws


def vq_prepared(codebook) -> torch.Tensor | None:
    """Workspace of the filtered assignment for ``codebook`` (a Parameter / tensor [K, 256] fp32, contiguous): the bf16
    fragment-major copy, |e|^2, the filter margins and max |e|^2 -- everything that depends on the codebook only
    (:func:`prepared_ws`).  None: shape not served."""
    k, d = codebook.shape
    served = core.VQ_FILTER and core.VQ_FUSED and d == 256 and k % 32 == 0 and codebook.dtype == torch.float32 and codebook.is_contiguous()
    return prepared_ws(codebook, _VQ_PREP, served, lambda k, d: _native.lib().vqk_vq_filter_ws_bytes(k, d), _vq_prepare_now)


def hist_sse(k: int, device, depth: int | None = None):
    """zeroed (hist int32 [K], sse fp32 [1]) -- with ``depth`` ([depth, K], [depth]) -- in one buffer: one fill launch"""
    m = depth or 1
    zbuf = torch.zeros(m * k + m, dtype=torch.int32, device=device)
    hist, sse = zbuf[:m * k], zbuf[m * k:].view(torch.float32)
    return (hist.view(depth, k) if depth else hist), sse


def nhwc_rows(z):
    """z [B,D,H,W] -> (z as fp32 NHWC, its memory as rows [N, D] -- a view --, (b, d, h, w))"""
    z = core.nhwc(z.to(torch.float32))
    b, d, h, w = z.shape
    return z, z.permute(0, 2, 3, 1).reshape(b * h * w, d), (b, d, h, w)


def rows_image(q, shape):
    """rows [N, D] -> [B,D,H,W] over the same (NHWC) memory"""
    b, d, h, w = shape
    return q.view(b, h, w, d).permute(0, 3, 1, 2)


def lookup_backward_frame(ctx, z, dq, dloss, beta: float, k: int, want_de: bool, cast_dq: bool = True):
    """What the backward of every nearest-code lookup sets up before its kernel: (dz, de, de_tgt, gs, dqc, cz, ce).
    de: where the codebook gradient is accumulated (atomics / ordered adds) -- straight into the optimizer's arena (de_tgt) when
    ``ctx.cb_param`` has one, else a zeroed [K, D]; None without ``want_de``.  gs: the loss cotangent on the device or None (then
    cz = ce = 0).  dqc: the upstream gradient as NHWC (``cast_dq``: anything but fp32 / bf16 becomes fp32) or None."""
    b, d, h, w = z.shape
    dz = torch.empty_like(z, memory_format=core._CL)
    de = de_tgt = None
    if want_de:
        de_tgt = core.direct_grad(ctx.cb_param) if ctx.cb_param.is_contiguous() else None
        de = de_tgt if de_tgt is not None else torch.zeros((k, d), dtype=torch.float32, device=z.device)
    gs = dloss.to(torch.float32).contiguous() if dloss is not None else None
    dqc = core.nhwc(dq) if dq is not None else None
    if cast_dq and dqc is not None and dqc.dtype not in (torch.float32, torch.bfloat16):
        dqc = dqc.to(torch.float32)
    scale = 2.0 / float(b * h * w * d) if gs is not None else 0.0
    return dz, de, de_tgt, gs, dqc, beta * scale, scale


def refresh_vq_prepared(owner=None, data_ptr: int | None = None) -> int:
    """re-derive the prepared workspaces whose codebook belongs to ``owner`` (a FlatAdamW that just stepped), lives at
    ``data_ptr`` (the EMA update wrote it through the C-ABI: no version bump), or -- both None -- is stale"""
    n = 0
    for table, prepare in _PREP_TABLES:
        for ptr, ent in list(table.items()):
            cbp = ent.wref()
            if cbp is None or cbp.data_ptr() != ptr:
                del table[ptr]
                continue
            if data_ptr is not None:
                hit = ptr == data_ptr
            elif owner is not None:
                hit = getattr(cbp, '_vqk_owner', None) is owner
            else:
                hit = ent.stamp != core._pack_stamp(cbp)
            if hit:
                prepare(ent, cbp.detach())
                ent.stamp = core._pack_stamp(cbp)
                n += 1
    return n


def vq_assign(flat_z: torch.Tensor, codebook: torch.Tensor, assoc: int) -> torch.Tensor:
    """flat_z [N,D] fp32, codebook [K,D] fp32 -> idx [N] int64 (bit-exact vs oracle/vq_oracle.c)."""
    core._require_gpu(flat_z)
    n, d = flat_z.shape
    k = codebook.shape[0]
    lib = _native.lib()
    z2 = torch.empty(n, dtype=torch.float32, device=flat_z.device)
    e2 = torch.empty(k, dtype=torch.float32, device=flat_z.device)
    idx = torch.empty(n, dtype=torch.int64, device=flat_z.device)
    s = core._stream()
    _native.check(lib.vqk_row_sqnorm_f32(flat_z.data_ptr(), n, d, z2.data_ptr(), s), 'row_sqnorm(z)')
    _native.check(lib.vqk_row_sqnorm_f32(codebook.data_ptr(), k, d, e2.data_ptr(), s), 'row_sqnorm(e)')
    if core.VQ_FILTER and d == 256 and k % 32 == 0:
        # bf16 candidate filter + exact fp32 re-rank: the same indices, bit for bit (csrc/vq_filter.hip)
        ws = _vq_filter_ws(flat_z.device, k, d)
        st = lib.vqk_vq_assign_filtered_f32(flat_z.data_ptr(), codebook.data_ptr(), z2.data_ptr(), e2.data_ptr(), n, k, d,
                                            assoc, idx.data_ptr(), ws.data_ptr(), ws.numel(), s)
        if st != _native.ERR_SHAPE:
            _native.check(st, 'vq_assign_filtered')
            return idx
    _native.check(lib.vqk_vq_assign_f32(flat_z.data_ptr(), codebook.data_ptr(), z2.data_ptr(), e2.data_ptr(), n, k, d,
                                        assoc, idx.data_ptr(), s), 'vq_assign')
    return idx


class VQLookupFn(torch.autograd.Function):
    """Nearest-codeword lookup with straight-through gradient and the (q-z)^2 losses.

    Standard (vector_quantizers.py:23-61): loss = mse(q, z.detach()) + beta * mse(q.detach(), z), grads to z and E.
    EMA      (vector_quantizers.py:128-180): loss = beta * mse(q.detach(), z), codebook has no grad.
    ``rotate``: the rotation-trick estimator (Fifty et al., ICLR 2025; csrc/vq_rot.hip) -- the forward is the same call sequence,
    the backward carries dq to z through the rotation and rescaling that maps z onto q instead of copying it; the commitment
    term and the codebook gradient are unchanged.  The mode travels on the autograd node.
    Returns (q [B,D,H,W] in out_dtype, idx [B, H*W] int64, loss 0-dim fp32, hist int32 [K])."""

    @staticmethod
    def forward(ctx, z, codebook, beta: float, codebook_loss: bool, assoc: int, out_dtype, rotate: bool = False):
        core._require_gpu(z)
        z, flat, (b, d, h, w) = nhwc_rows(z)
        n = b * h * w
        # EMA rewrites the codebook in place right after the lookup: backward must see the pre-update rows
        cb = codebook.detach().contiguous() if codebook_loss else codebook.detach().clone()
        k = cb.shape[0]
        qlo = core.empty_nhwc(b, d, h, w, torch.bfloat16, z.device) if out_dtype == torch.bfloat16 else None
        hist, sse = hist_sse(k, z.device)
        sse = sse.view(())
        ws = vq_prepared(codebook) if codebook.is_contiguous() else None
        if ws is not None:
            # ONE kernel: |z|^2, bf16 filter + exact re-rank, gather, sum (q - z)^2, histogram (csrc/vq_filter.hip); the
            # fp32 copy of q is only written when it is the output
            q32 = core.empty_nhwc(b, d, h, w, torch.float32, z.device) if qlo is None else None
            idx = torch.empty(n, dtype=torch.int64, device=z.device)
            _native.check(_native.lib().vqk_vq_forward_f32(flat.data_ptr(), codebook.detach().data_ptr(), ws.data_ptr(), ws.numel(),
                                                           n, k, d, assoc, idx.data_ptr(), core._p(q32), core._p(qlo), sse.data_ptr(),
                                                           hist.data_ptr(), core._stream()), 'vq_forward')
        else:
            idx = vq_assign(flat, cb, assoc)
            q32 = core.empty_nhwc(b, d, h, w, torch.float32, z.device)
            _native.check(_native.lib().vqk_vq_gather_f32(flat.data_ptr(), cb.data_ptr(), idx.data_ptr(), n, k, d,
                                                          q32.data_ptr(), core._p(qlo), sse.data_ptr(), hist.data_ptr(),
                                                          core._stream()), 'vq_gather')
        loss = sse * (((1.0 + beta) if codebook_loss else beta) / float(n * d))       # mse + beta * mse | beta * mse: one launch
        ctx.save_for_backward(z, cb, idx)
        ctx.cfg = (beta, codebook_loss, n, k, d)
        ctx.rotate = bool(rotate)
        ctx.cb_param = codebook
        ctx.mark_non_differentiable(idx, hist)
        q = qlo if qlo is not None else q32
        return q, idx.view(b, h * w), loss, hist

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist):
        z, cb, idx = ctx.saved_tensors
        beta, codebook_loss, n, k, d = ctx.cfg
        dz, de, de_tgt, gs, dqc, cz, ce = lookup_backward_frame(ctx, z, dq, dloss, beta, k, codebook_loss and ctx.needs_input_grad[1],
                                                                cast_dq=False)
        fused = core.VQ_FUSED and d == 256 and not core.DETERMINISTIC       # (deterministic mode: the ordered two-kernel form)
        if ctx.rotate:                                                      # one entry point: it picks the fused / ordered form itself
            fn = _native.lib().vqk_vq_backward_rot_f32
        else:
            fn = _native.lib().vqk_vq_backward_fused_f32 if fused else _native.lib().vqk_vq_backward_f32
        _native.check(fn(z.data_ptr(), cb.data_ptr(), idx.data_ptr(), core._p(dqc),
                         core.dcode(dqc.dtype) if dqc is not None else core.F32, n, k, d, cz, ce, core._p(gs), dz.data_ptr(),
                         core._p(de), core._stream()), 'vq_backward_rot' if ctx.rotate else 'vq_backward')
        return dz, (None if de_tgt is not None else de), None, None, None, None, None



class EntropyVQFn(torch.autograd.Function):
    """Entropy-regularised lookup (vector_quantizers.py:290-356, ent_loss_type='softmax'):
    loss = beta*mse(q.detach(), z) + mse(q, z.detach()) + ratio*(mean_i H(p_i) - H(mean_i p_i)),  p = softmax(-d/T).
    The fp32 distance matrix is a TRANSIENT of each direction (N*K*4 bytes: 0.5 GB at N=16384, K=8192): the forward
    reduces it to lse[N], hrow[N], u[K] and frees it, the backward recomputes it once (same kernel, same bits) and
    overwrites it in place by its cotangent; dz / dE come from two fp32-MFMA GEMMs that reuse the 1x1 conv kernels.
    Returns (q, idx [B,HW], loss, hist)."""

    @staticmethod
    def forward(ctx, z, codebook, beta: float, ratio: float, temperature: float, out_dtype, loss_type: str = 'softmax'):
        core._require_gpu(z)
        if loss_type not in ('softmax', 'argmax'):
            raise ValueError('Entropy loss {} not supported'.format(loss_type))      # vector_quantizers.py:317, at forward
        z = core.nhwc(z.to(torch.float32))
        b, d, h, w = z.shape
        n = b * h * w
        cb = codebook.detach().contiguous()
        k = cb.shape[0]
        if k % 4:
            raise RuntimeError('vqk: entropy quantizer needs num_embeddings % 4 == 0')
        flat = z.permute(0, 2, 3, 1).reshape(n, d)
        lib, st, dev = _native.lib(), core._stream(), z.device
        f32 = dict(dtype=torch.float32, device=dev)
        z2, e2 = torch.empty(n, **f32), torch.empty(k, **f32)
        idx = torch.empty(n, dtype=torch.int64, device=dev)
        dmat = torch.empty((n, k), **f32)
        _native.check(lib.vqk_row_sqnorm_f32(flat.data_ptr(), n, d, z2.data_ptr(), st), 'row_sqnorm(z)')
        _native.check(lib.vqk_row_sqnorm_f32(cb.data_ptr(), k, d, e2.data_ptr(), st), 'row_sqnorm(e)')
        scal = torch.zeros(3, **f32)                           # sse, hsum, avg_term
        lse, hrow = torch.empty(n, **f32), torch.empty(n, **f32)
        fused_rows = loss_type == 'softmax' and d == 256 and core.ENTROPY_FUSED_ROWS
        if fused_rows:                                         # the row statistics ride under the distance MFMAs (csrc/vq.hip)
            _native.check(lib.vqk_vq_distances_stats_f32(flat.data_ptr(), cb.data_ptr(), z2.data_ptr(), e2.data_ptr(), n, k, d, 1,
                                                         idx.data_ptr(), dmat.data_ptr(), temperature, lse.data_ptr(),
                                                         hrow.data_ptr(), scal[1:2].data_ptr(), st), 'vq_distances_stats')
        else:
            _native.check(lib.vqk_vq_distances_f32(flat.data_ptr(), cb.data_ptr(), z2.data_ptr(), e2.data_ptr(), n, k, d, 1,
                                                   idx.data_ptr(), dmat.data_ptr(), st), 'vq_distances')
        q32 = core.empty_nhwc(b, d, h, w, torch.float32, dev)
        qlo = core.empty_nhwc(b, d, h, w, torch.bfloat16, dev) if out_dtype == torch.bfloat16 else None
        hist = torch.zeros(k, dtype=torch.int32, device=dev)
        _native.check(lib.vqk_vq_gather_f32(flat.data_ptr(), cb.data_ptr(), idx.data_ptr(), n, k, d, q32.data_ptr(),
                                            core._p(qlo), scal[0:1].data_ptr(), hist.data_ptr(), st), 'vq_gather')
        psum, u = torch.zeros(k, **f32), torch.empty(k, **f32)
        if fused_rows:
            _native.check(lib.vqk_entropy_forward_presummed_f32(dmat.data_ptr(), n, k, temperature, lse.data_ptr(), psum.data_ptr(),
                                                                u.data_ptr(), scal[2:3].data_ptr(), st), 'entropy_forward_presummed')
            ent = scal[1] / float(n) + scal[2]
        elif loss_type == 'softmax':
            _native.check(lib.vqk_entropy_forward_f32(dmat.data_ptr(), n, k, temperature, lse.data_ptr(), hrow.data_ptr(),
                                                      scal[1:2].data_ptr(), psum.data_ptr(), u.data_ptr(),
                                                      scal[2:3].data_ptr(), st), 'entropy_forward')
            ent = scal[1] / float(n) + scal[2]
        else:                                                  # one-hot targets: sample term from the assigned code only
            s2 = torch.zeros(2, **f32)                         # row-entropy sum (unused by the loss), sample-term sum
            _native.check(lib.vqk_entropy_argmax_forward_f32(dmat.data_ptr(), idx.data_ptr(), hist.data_ptr(), n, k,
                                                             temperature, lse.data_ptr(), hrow.data_ptr(),
                                                             s2[0:1].data_ptr(), s2[1:2].data_ptr(), psum.data_ptr(),
                                                             u.data_ptr(), scal[2:3].data_ptr(), st), 'entropy_argmax_forward')
            ent = s2[1] / float(n) + scal[2]
        mse = scal[0] / float(n * d)
        loss = beta * mse + mse + ent * ratio
        # Nothing of size N x K survives the forward: the backward recomputes the distance matrix ONCE (the same kernel, the same
        # bits) into a transient buffer; what is kept is z, the codebook, idx and the row / column statistics lse[N], hrow[N], u[K]
        # (round 3 saved dmat: 537 MB at N = 16,384, K = 8,192, growing with N x K)
        del dmat
        ctx.save_for_backward(z, cb, idx, lse, hrow, u, z2, e2)
        ctx.cfg = (beta, ratio, temperature, n, k, d, loss_type)
        ctx.split_gemm = (core.ENTROPY_SPLIT_GEMM and out_dtype == torch.bfloat16 and loss_type == 'softmax' and k % 128 == 0
                          and d % 128 == 0 and n % 128 == 0)
        ctx.mark_non_differentiable(idx, hist)
        return (qlo if qlo is not None else q32), idx.view(b, h * w), loss, hist

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist):
        z, cb, idx, lse, hrow, u, z2, e2 = ctx.saved_tensors
        beta, ratio, temperature, n, k, d, loss_type = ctx.cfg
        lib, st = _native.lib(), core._stream()
        flat = z.permute(0, 2, 3, 1).reshape(n, d)
        gs = dloss.to(torch.float32).contiguous() if dloss is not None else None
        dqc = core.nhwc(dq) if dq is not None else None
        scale = 2.0 / float(n * d) if gs is not None else 0.0
        dz = torch.empty_like(z, memory_format=core._CL)
        de = torch.zeros_like(cb)
        fused = core.VQ_FUSED and d == 256 and not core.DETERMINISTIC       # one kernel (csrc/vq_filter.hip); K = 8192: 41 against 235 us
        fn = lib.vqk_vq_backward_fused_f32 if fused else lib.vqk_vq_backward_f32
        _native.check(fn(z.data_ptr(), cb.data_ptr(), idx.data_ptr(), core._p(dqc),
                         core.dcode(dqc.dtype) if dqc is not None else core.F32, n, k, d, beta * scale, scale,
                         core._p(gs), dz.data_ptr(), de.data_ptr(), st), 'vq_backward')
        if gs is None:
            return dz, de, None, None, None, None, None
        # the distance matrix again (transient), then dmat <- dL_ent/dd  (rows sum to zero)
        dmat = torch.empty((n, k), dtype=torch.float32, device=z.device)
        idx2 = torch.empty(n, dtype=torch.int64, device=z.device)
        _native.check(lib.vqk_vq_distances_f32(flat.data_ptr(), cb.data_ptr(), z2.data_ptr(), e2.data_ptr(), n, k, d, 1,
                                               idx2.data_ptr(), dmat.data_ptr(), st), 'vq_distances (backward recompute)')
        if ctx.split_gemm:
            # throughput mode: the cotangent as hi + lo bf16 matrices and the two GEMMs as split products on the bf16 MFMA kernels
            #   dd E  ~ hi [E_hi | E_lo] + lo E_hi,     dd^T Z ~ hi^T [Z_hi | Z_lo] + lo^T Z_hi     (dropped: lo x lo, 2^-16 relative)
            # -- 3x the multiply-adds at > 5x the rate of the fp32 MFMA kernels (0.70 ms per GEMM at N = 16,384, K = 8,192)
            bf = dict(dtype=torch.bfloat16, device=z.device)
            hi, lo = torch.empty((n, k), **bf), torch.empty((n, k), **bf)
            _native.check(lib.vqk_entropy_backward_split_f32(dmat.data_ptr(), lse.data_ptr(), hrow.data_ptr(), u.data_ptr(), n, k,
                                                             temperature, ratio, gs.data_ptr(), hi.data_ptr(), lo.data_ptr(), st),
                          'entropy_backward_split')
            del dmat

            def split(t):
                th = t.to(torch.bfloat16)
                return th, (t - th.float()).to(torch.bfloat16)
            e_hi, e_lo = split(cb)                                                      # [K][D]
            z_hi, z_lo = split(flat)                                                    # [N][D]
            img = lambda t: t.view(1, t.shape[0], 1, t.shape[1]).permute(0, 3, 1, 2)    # [rows][C] memory as a [1, C, rows, 1] nhwc image
            w1 = torch.cat([e_hi.t(), e_lo.t()], 0).contiguous()                        # [2D][K]
            g1 = core.raw_conv_fprop(img(hi), w1, None, None, 1, False, 0, torch.float32, 2 * d, 0).permute(0, 2, 3, 1).reshape(n, 2 * d)
            g1b = core.raw_conv_fprop(img(lo), e_hi.t().contiguous(), None, None, 1, False, 0, torch.float32, d, 0).permute(0, 2, 3, 1).reshape(n, d)
            dz.permute(0, 2, 3, 1).reshape(n, d).add_(g1[:, :d] + g1[:, d:] + g1b, alpha=-2.0)
            zc = torch.cat([z_hi, z_lo], 1).contiguous()                                # [N][2D]
            g2 = core.raw_conv_wgrad(img(zc), img(hi), 1, False).permute(0, 2, 3, 1).reshape(k, 2 * d)
            g2b = core.raw_conv_wgrad(img(z_hi.contiguous()), img(lo), 1, False).permute(0, 2, 3, 1).reshape(k, d)
            de.add_(g2[:, :d] + g2[:, d:] + g2b, alpha=-2.0)
            cs = core.raw_colsum(n, k, hi)
            core.raw_colsum(n, k, lo, out=cs)
            _native.check(lib.vqk_row_scale_add_f32(de.data_ptr(), cb.data_ptr(), cs.data_ptr(), k, d, 2.0, st), 'row_scale_add')
            return dz, de, None, None, None, None, None
        if loss_type == 'softmax':
            _native.check(lib.vqk_entropy_backward_f32(dmat.data_ptr(), lse.data_ptr(), hrow.data_ptr(), u.data_ptr(), n, k,
                                                       temperature, ratio, gs.data_ptr(), st), 'entropy_backward')
        else:
            _native.check(lib.vqk_entropy_argmax_backward_f32(dmat.data_ptr(), idx.data_ptr(), lse.data_ptr(), hrow.data_ptr(),
                                                              u.data_ptr(), n, k, temperature, ratio, gs.data_ptr(), st),
                          'entropy_argmax_backward')
        dd = dmat.view(1, n, 1, k).permute(0, 3, 1, 2)            # [1, K, N, 1] logical, [N][K] memory (NHWC)
        # dz += -2 dd @ E      (1x1 conv: pixels = rows of dd, Cin = K, Cout = D, weight [D][K] = E^T)
        et = cb.t().contiguous()
        g1 = core.raw_conv_fprop(dd, et, None, None, 1, False, 0, torch.float32, d, 0)        # [1, D, N, 1] -> memory [N][D]
        _native.check(lib.vqk_axpby(core.F32, g1.data_ptr(), dz.data_ptr(), dz.data_ptr(), -2.0, 1.0, n * d, st), 'axpby')
        # dE += -2 dd^T @ Z + 2 E * colsum(dd)   (1x1 wgrad: contraction over the N rows)
        zimg = flat.view(1, n, 1, d).permute(0, 3, 1, 2)
        g2 = core.raw_conv_wgrad(zimg, dd, 1, False)                                           # memory [K][D]
        g2 = g2.permute(0, 2, 3, 1).reshape(k, d)
        _native.check(lib.vqk_axpby(core.F32, g2.data_ptr(), de.data_ptr(), de.data_ptr(), -2.0, 1.0, k * d, st), 'axpby')
        cs = core.raw_colsum(n, k, dmat)
        _native.check(lib.vqk_row_scale_add_f32(de.data_ptr(), cb.data_ptr(), cs.data_ptr(), k, d, 2.0, st), 'row_scale_add')
        return dz, de, None, None, None, None, None


class GumbelVQFn(torch.autograd.Function):
    """Gumbel-softmax quantization of logits [B,K,H,W] (vector_quantizers.py:233-243): y = softmax((logits+g)/tau),
    q = y @ E, kl = kl_cost * mean_i sum_n qy log(qy K + 1e-10).  The Exp(1) noise is an INPUT (drawn with torch's
    RNG by the module, or injected for parity).  Both GEMMs (y@E, dq@E^T) and dE = y^T@dq run on the 1x1 conv
    kernels.  Returns (q [B,D,H,W], idx [B,H,W], kl, hist)."""

    @staticmethod
    def forward(ctx, logits, codebook, noise, tau: float, kl_cost: float, hard: bool, out_dtype, sched=None):
        """``sched``: optional device tensor [tau, kl_cost] that overrides the two scalars inside the kernels (graph replay)"""
        core._require_gpu(logits)
        logits = core.nhwc(logits.to(torch.float32))
        noise = core.nhwc(noise.to(torch.float32))
        b, k, h, w = logits.shape
        n = b * h * w
        cb = codebook.detach().contiguous()
        d = cb.shape[1]
        dt = out_dtype
        lib, st, dev = _native.lib(), core._stream(), logits.device
        y = torch.empty(n * k, dtype=dt, device=dev).view(1, n, 1, k).permute(0, 3, 1, 2)
        idx = torch.empty(n, dtype=torch.int64, device=dev)
        klsum = torch.zeros((), dtype=torch.float32, device=dev)
        hist = torch.zeros(k, dtype=torch.int32, device=dev)
        _native.check(lib.vqk_gumbel_forward(core.dcode(dt), logits.data_ptr(), noise.data_ptr(), n, k, tau, int(hard),
                                             y.data_ptr(), idx.data_ptr(), klsum.data_ptr(), hist.data_ptr(), core._p(sched), st),
                      'gumbel_forward')
        et = core.pack_weights(cb.t().contiguous().reshape(-1), dt, d, k, 1, False, 0)                # [D][K]
        q = core.raw_conv_fprop(y, et, None, None, 1, False, 0, dt, d, 0)                              # [1,D,N,1] == [N][D]
        q = q.permute(0, 2, 3, 1).reshape(b, h, w, d).permute(0, 3, 1, 2)                         # [B,D,H,W] nhwc view
        ctx.save_for_backward(logits, noise, cb, y)
        ctx.cfg = (tau, kl_cost, n, k, d, dt, (b, h, w))
        ctx.sched = sched
        ctx.mark_non_differentiable(idx, hist)
        kl = klsum * (kl_cost / float(n)) if sched is None else klsum * sched[1] / float(n)
        return q, idx.view(b, h, w), kl, hist

    @staticmethod
    def backward(ctx, dq, _didx, dkl, _dhist):
        logits, noise, cb, y = ctx.saved_tensors
        tau, kl_cost, n, k, d, dt, (b, h, w) = ctx.cfg
        lib, st = _native.lib(), core._stream()
        dqc = core.nhwc(dq.to(dt)) if dq is not None else torch.zeros((b, d, h, w), dtype=dt, device=logits.device).contiguous(memory_format=core._CL)
        dq_img = dqc.permute(0, 2, 3, 1).reshape(1, n, 1, d).permute(0, 3, 1, 2)                  # [1,D,N,1], memory [N][D]
        e_w = core.pack_weights(cb.reshape(-1), dt, k, d, 1, False, 0)                                 # [K][D]
        dyv = core.raw_conv_fprop(dq_img, e_w, None, None, 1, False, 0, dt, k, 0)                      # [N][K]
        gs = dkl.to(torch.float32).contiguous() if dkl is not None else None
        if gs is None and ctx.sched is not None:
            # no KL cotangent, but y must still be recomputed at the forward's temperature sched[0]: the kernel takes the schedule
            # tensor and a zero cotangent (with a schedule tensor it reads its KL coefficient sched[1] / n itself)
            gs = torch.zeros((), dtype=torch.float32, device=logits.device)
        dlogits = torch.empty_like(logits, memory_format=core._CL)
        _native.check(lib.vqk_gumbel_backward(core.dcode(dt), logits.data_ptr(), noise.data_ptr(), dyv.data_ptr(), n, k, tau,
                                              kl_cost if gs is not None else 0.0, core._p(gs), dlogits.data_ptr(),
                                              core._p(ctx.sched), st),
                      'gumbel_backward')
        de = None
        if ctx.needs_input_grad[1]:
            de = core.raw_conv_wgrad(dq_img, y, 1, False).permute(0, 2, 3, 1).reshape(k, d)            # y^T @ dq
        return dlogits, de, None, None, None, None, None, None


def ema_stats(flat_z, idx, k: int, out=None) -> torch.Tensor:
    """packed [counts(K) | dw(K*D)] of this rank's batch (vector_quantizers.py:159-163); ``out``: a persistent buffer
    (zeroed here) so that a captured graph always writes the same memory"""
    n, d = flat_z.shape
    buf = out if out is not None else torch.empty(k + k * d, dtype=torch.float32, device=flat_z.device)
    buf.zero_()
    fn = _native.lib().vqk_ema_stats_fused_f32 if (core.VQ_FUSED and d == 256) else _native.lib().vqk_ema_stats_f32
    _native.check(fn(flat_z.data_ptr(), idx.data_ptr(), n, k, d, buf.data_ptr(), buf[k:].data_ptr(), core._stream()), 'ema_stats')
    return buf


def ema_apply(buf, ema_count, ema_weight, codebook, decay: float, eps: float, batch: float) -> None:
    """EMA update in place from the (all-reduced) packed statistics (vector_quantizers.py:164-169)"""
    k, d = codebook.shape
    _native.check(_native.lib().vqk_ema_update_f32(ema_count.data_ptr(), ema_weight.data_ptr(), codebook.data_ptr(),
                                                   buf.data_ptr(), buf[k:].data_ptr(), k, d, decay, eps, batch, core._stream()),
                  'ema_update')
    refresh_vq_prepared(data_ptr=codebook.data_ptr())      # written through the C-ABI: no version bump to notice


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations')]
