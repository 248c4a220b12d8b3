"""Residual-quantizer operators over the vqk C-ABI (csrc/rvq.hip): the autograd Function behind ``ResidualVectorQuantizer`` plus the
assignment-only and decode launchers, and the STAGED formulation of the same definition on the single-stage lookup.  Private part of
:mod:`ops` like ``_ops_proj.py`` (imported at the end of ``ops.py``, which re-exports every name); shared infrastructure is reached
through ``core``.

Definition (include/vqk.h, "residual quantizer"): r_0 = z; k_q = the standard quantizer's argmin on r_{q-1}; r_q = r_{q-1} - e[k_q];
zhat = ((e[k_1] + e[k_2]) + ...) + e[k_Q]; loss = (1 + beta) / (N D) sum_q |r_q|^2."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core
from ._ops_vq import hist_sse, lookup_backward_frame, nhwc_rows, rows_image, vq_assign, vq_prepared

RVQ_MAX_DEPTH = 8
_RVQ_WS: dict = {}                  # _wkey() -> the residual stack of the deterministic backward (core.grow_ws)


def _check_depth(depth) -> int:
    depth = int(depth)
    if not 1 <= depth <= RVQ_MAX_DEPTH:
        raise ValueError(f'residual quantizer: depth must be between 1 and {RVQ_MAX_DEPTH}, got {depth}')
    return depth


def rvq_fused_serves(codebook) -> bool:
    """the one-launch forward serves this codebook (D == 256, K % 32 == 0, fp32, contiguous) and is switched on"""
    return bool(core.RVQ_FUSED and codebook.is_contiguous() and vq_prepared(codebook) is not None)


def rvq_staged(flat_z: torch.Tensor, codebook: torch.Tensor, depth: int, want_lo: bool = False):
    """The definition built from the single-stage operators: per stage one lookup (vqk_vq_forward_f32 on the prepared workspace when
    the shape is served, else vq_assign + vqk_vq_gather_f32), then r <- r - q and zhat <- zhat + q as fp32 torch operations.
    The product path of the shapes the fused kernel does not serve, and what the fused kernel must equal bit for bit.
    flat_z [N, D] fp32 -> (idx [N, depth] int64, zhat [N, D] fp32, zhat as bf16 or None, sse [depth] fp32, hist [depth, K] int32)."""
    core._require_gpu(flat_z)
    depth = _check_depth(depth)
    n, d = flat_z.shape
    k = codebook.shape[0]
    cb = core.f32c(codebook)
    dev = flat_z.device
    lib, st = _native.lib(), core._stream()
    ws = vq_prepared(codebook) if codebook.is_contiguous() else None
    hist, sse = hist_sse(k, dev, depth)
    idx = torch.empty((n, depth), dtype=torch.int64, device=dev)
    r = core.f32c(flat_z)
    zhat = None
    for q in range(depth):
        q32 = torch.empty((n, d), dtype=torch.float32, device=dev)
        if ws is not None:
            iq = torch.empty(n, dtype=torch.int64, device=dev)
            _native.check(lib.vqk_vq_forward_f32(r.data_ptr(), cb.data_ptr(), ws.data_ptr(), ws.numel(), n, k, d, 0, iq.data_ptr(),
                                                 q32.data_ptr(), 0, sse[q:].data_ptr(), hist[q].data_ptr(), st), 'vq_forward (rvq stage)')
        else:
            iq = vq_assign(r, cb, 0)
            _native.check(lib.vqk_vq_gather_f32(r.data_ptr(), cb.data_ptr(), iq.data_ptr(), n, k, d, q32.data_ptr(), 0,
                                                sse[q:].data_ptr(), hist[q].data_ptr(), st), 'vq_gather (rvq stage)')
        idx[:, q] = iq
        r = r - q32
        zhat = q32 if zhat is None else zhat + q32
    return idx, zhat, (zhat.to(torch.bfloat16) if want_lo else None), sse, hist


def _rvq_forward(flat_z, codebook, depth: int, want_q32: bool, want_lo: bool, want_stats: bool):
    """(idx [N, depth], zhat fp32 or None, zhat bf16 or None, sse [depth] or None, hist [depth, K] or None): the fused kernel when
    it serves the codebook, the staged formulation otherwise"""
    n, d = flat_z.shape
    k = codebook.shape[0]
    if not rvq_fused_serves(codebook):
        idx, q32, qlo, sse, hist = rvq_staged(flat_z, codebook, depth, want_lo)
        return idx, q32, qlo, sse, hist
    dev = flat_z.device
    ws = vq_prepared(codebook)
    sse = hist = None
    if want_stats:
        hist, sse = hist_sse(k, dev, depth)
    idx = torch.empty((n, depth), dtype=torch.int64, device=dev)
    q32 = torch.empty((n, d), dtype=torch.float32, device=dev) if want_q32 else None
    qlo = torch.empty((n, d), dtype=torch.bfloat16, device=dev) if want_lo else None
    _native.check(_native.lib().vqk_rvq_forward_f32(flat_z.data_ptr(), codebook.detach().data_ptr(), ws.data_ptr(), ws.numel(), n, k, d,
                                                    depth, idx.data_ptr(), core._p(q32), core._p(qlo), core._p(sse), core._p(hist),
                                                    core._stream()), 'rvq_forward')
    return idx, q32, qlo, sse, hist


def rvq_assign(flat_z: torch.Tensor, codebook: torch.Tensor, depth: int) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N, depth] int64: the forward without zhat and the statistics"""
    core._require_gpu(flat_z)
    depth = _check_depth(depth)
    return _rvq_forward(core.f32c(flat_z), codebook, depth, False, False, False)[0]


def rvq_decode(idx: torch.Tensor, codebook: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """idx [..., depth] int64 -> zhat [..., D] in ``out_dtype``: the bits the forward writes for the same tokens"""
    depth = _check_depth(idx.shape[-1])
    core._require_gpu(idx)
    cb = core.f32c(codebook)
    k, d = cb.shape
    flat = idx.reshape(-1, depth).to(torch.int64).contiguous()
    n = flat.shape[0]
    lo = out_dtype == torch.bfloat16
    q = torch.empty((n, d), dtype=torch.bfloat16 if lo else torch.float32, device=idx.device)
    _native.check(_native.lib().vqk_rvq_decode_f32(flat.data_ptr(), cb.data_ptr(), n, k, d, depth, 0 if lo else q.data_ptr(),
                                                   q.data_ptr() if lo else 0, core._stream()), 'rvq_decode')
    return q.view(*idx.shape[:-1], d)


class RVQLookupFn(torch.autograd.Function):
    """Residual lookup with the straight-through gradient and the per-stage codebook + commitment losses.
    Returns (q [B,D,H,W] in out_dtype, idx [B, H*W, depth] int64, loss 0-dim fp32, hist int32 [K] pooled over the stages,
    depth_hist int32 [depth, K], stage_sse fp32 [depth])."""

    @staticmethod
    def forward(ctx, z, codebook, beta: float, depth: int, out_dtype):
        core._require_gpu(z)
        depth = _check_depth(depth)
        z, flat, (b, d, h, w) = nhwc_rows(z)
        n = b * h * w
        cb = codebook.detach().contiguous()
        k = cb.shape[0]
        lo = out_dtype == torch.bfloat16
        idx, q32, qlo, sse, depth_hist = _rvq_forward(flat, codebook, depth, not lo, lo, True)
        q = rows_image(qlo if lo else q32, (b, d, h, w))
        hist = depth_hist.sum(0, dtype=torch.int32)              # pooled usage: what the model accumulates and re-initialises from
        loss = sse.sum() * ((1.0 + beta) / float(n * d))
        ctx.save_for_backward(z, cb, idx)
        ctx.cfg = (beta, depth, n, k, d)
        ctx.cb_param = codebook
        ctx.mark_non_differentiable(idx, hist, depth_hist, sse)
        ctx.set_materialize_grads(False)                       # an unused output's gradient arrives as None (dq = NULL in the kernel), not as zeros
        return q, idx.view(b, h * w, depth), loss, hist, depth_hist, sse

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist, _ddh, _dsse):
        z, cb, idx = ctx.saved_tensors
        beta, depth, n, k, d = ctx.cfg
        dz, de, de_tgt, gs, dqc, cz, ce = lookup_backward_frame(ctx, z, dq, dloss, beta, k, ctx.needs_input_grad[1])
        if d == 256:
            lib = _native.lib()
            ws = core.grow_ws(_RVQ_WS, z.device, lib.vqk_rvq_backward_ws_bytes(n, d, depth)) if (core.DETERMINISTIC and de is not None) else None
            _native.check(lib.vqk_rvq_backward_f32(z.data_ptr(), cb.data_ptr(), idx.data_ptr(), core._p(dqc),
                                                   core.dcode(dqc.dtype) if dqc is not None else core.F32, n, k, d, depth, cz, ce,
                                                   core._p(gs), dz.data_ptr(), core._p(de), core._p(ws),
                                                   ws.numel() if ws is not None else 0, core._stream()), 'rvq_backward')
        else:
            # the shapes the kernels do not serve: the same running subtraction as fp32 torch operations (index_add_ in arrival order)
            flat_dz = dz.permute(0, 2, 3, 1).reshape(n, d)
            r = z.permute(0, 2, 3, 1).reshape(n, d)
            total = None
            for q in range(depth):
                r = r - cb[idx[:, q]]
                total = r if total is None else total + r
                if de is not None and gs is not None:
                    de.index_add_(0, idx[:, q], r * (gs * -ce))
            g = total * (gs * cz) if gs is not None else torch.zeros_like(total)
            flat_dz.copy_(g if dqc is None else g + dqc.permute(0, 2, 3, 1).reshape(n, d).float())
        return dz, (None if de_tgt is not None else de), None, None, None


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations', 'hist_sse', 'lookup_backward_frame', 'nhwc_rows', 'rows_image', 'vq_assign', 'vq_prepared')]
