"""Cosine-quantizer operators over the vqk C-ABI (csrc/vq_cos.hip): the autograd Function behind ``CosineVectorQuantizer`` plus the
assignment-only and decode launchers, and the STAGED formulation of the same definition on the standard quantizer's operators.
Private part of :mod:`ops` like ``_ops_rvq.py`` (imported at the end of ``ops.py``, which re-exports every name); shared
infrastructure is reached through ``core``.

Definition (include/vqk.h, "cosine quantizer"): zn = nrm(z), en = nrm(e) (l2 normalisation, eps = 1e-12); idx = the standard
quantizer's argmin on (zn, en); q = en[idx]; loss = (1 + beta) / (N D) sum |q - zn|^2; the straight-through estimator is taken at zn."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core
from ._ops_vq import _PREP_TABLES, hist_sse, lookup_backward_frame, nhwc_rows, prepared_ws, rows_image, vq_assign

COS_EPS = 1e-12
COS_FUSED_DIMS = (8, 16, 32, 64)
_COS_PREP: dict = {}            # data_ptr of the codebook -> _VQPrep: what vqk_cos_prepare_f32 derived from it
_COS_WS: dict = {}                  # _wkey() -> the per-row terms of the deterministic backward (core.grow_ws)


def _cos_prepare_now(ent, cb) -> None:
    _native.check(_native.lib().vqk_cos_prepare_f32(cb.data_ptr(), ent.k, ent.d, ent.ws.data_ptr(), ent.ws.numel(), core._stream()),
                  'cos_prepare')


_PREP_TABLES.append((_COS_PREP, _cos_prepare_now))       # ops.refresh_vq_prepared keeps these workspaces current too


def cos_prepared(codebook) -> torch.Tensor | None:
    """Workspace of the cosine lookup for ``codebook`` (a Parameter / tensor [K, D] fp32, contiguous, D % 4 == 0): the normalised
    rows en [K, D], |en|^2 [K] and 1 / max(|e|, eps) [K].  Built when the codebook CHANGES, not per step: stamped and refreshed
    exactly like :func:`vq_prepared` (``refresh_vq_prepared`` walks both tables), so a captured step holds no prepare launch and a
    replay after an optimizer step sees the new codebook.  None: shape not served (the caller normalises per call)."""
    served = codebook.shape[1] % 4 == 0 and codebook.dtype == torch.float32 and codebook.is_contiguous() and codebook.is_cuda
    return prepared_ws(codebook, _COS_PREP, served, lambda k, d: _native.lib().vqk_cos_ws_bytes(k, d), _cos_prepare_now)


def _ws_views(ws, k: int, d: int):
    """(en [K, D], |en|^2 [K], inv_e [K]) fp32 views of a prepared workspace"""
    o2 = k * d * 4
    oi = o2 + (k * 4 + 15) // 16 * 16
    return ws[:o2].view(torch.float32).view(k, d), ws[o2:o2 + k * 4].view(torch.float32), ws[oi:oi + k * 4].view(torch.float32)


def _cos_ws(codebook):
    """the prepared workspace of ``codebook``; a tensor that is not cached (non-contiguous, another dtype) is prepared per call"""
    ws = cos_prepared(codebook)
    if ws is not None:
        return ws
    cb = core.f32c(codebook)
    k, d = cb.shape
    ws = torch.empty(_native.lib().vqk_cos_ws_bytes(k, d), dtype=torch.uint8, device=cb.device)
    _native.check(_native.lib().vqk_cos_prepare_f32(cb.data_ptr(), k, d, ws.data_ptr(), ws.numel(), core._stream()), 'cos_prepare')
    return ws


def l2norm_rows(x: torch.Tensor, want_inv: bool = False):
    """x [R, D] fp32 (D % 4 == 0) -> nrm(x) [R, D] (and inv [R]): vqk_l2norm_rows_f32, the bits every cosine kernel normalises with"""
    core._require_gpu(x)
    x = core.f32c(x)
    r, d = x.shape
    xn = torch.empty_like(x)
    inv = torch.empty(r, dtype=torch.float32, device=x.device) if want_inv else None
    _native.check(_native.lib().vqk_l2norm_rows_f32(x.data_ptr(), r, d, xn.data_ptr(), core._p(inv), core._stream()), 'l2norm_rows')
    return (xn, inv) if want_inv else xn


def cos_fused_serves(codebook) -> bool:
    """the one-launch forward serves this codebook (D in {8, 16, 32, 64}, K % 32 == 0, fp32, contiguous) and is switched on"""
    k, d = codebook.shape
    return bool(core.COS_FUSED and d in COS_FUSED_DIMS and k % 32 == 0 and cos_prepared(codebook) is not None)


def cos_staged(flat_z: torch.Tensor, codebook: torch.Tensor, want_lo: bool = False):
    """The definition built from the stand-alone operators: vqk_l2norm_rows_f32 on z, the prepared (= vqk_l2norm_rows_f32) codebook,
    ``ops.vq_assign(zn, en, 0)`` and vqk_vq_gather_f32.  The product path of the shapes the fused kernel does not serve (other D,
    including 256 where vq_assign takes the filter path; K not a multiple of 32), and what the fused kernel must equal bit for bit.
    In deterministic mode the sum |q - zn|^2 is taken by vqk_cos_sse_f32 (the gather's is one float atomic per block).
    flat_z [N, D] fp32 -> (idx [N] int64, q [N, D] fp32, q as bf16 or None, sse [1] fp32, hist [K] int32, zn [N, D], inv_z [N])."""
    core._require_gpu(flat_z)
    n, d = flat_z.shape
    k = codebook.shape[0]
    dev = flat_z.device
    lib, st = _native.lib(), core._stream()
    en = _ws_views(_cos_ws(codebook), k, d)[0]
    zn, inv_z = l2norm_rows(flat_z, want_inv=True)
    idx = vq_assign(zn, en, 0)
    hist, sse = hist_sse(k, dev)
    q32 = torch.empty((n, d), dtype=torch.float32, device=dev)
    qlo = torch.empty((n, d), dtype=torch.bfloat16, device=dev) if want_lo else None
    det = core.DETERMINISTIC
    _native.check(lib.vqk_vq_gather_f32(zn.data_ptr(), en.data_ptr(), idx.data_ptr(), n, k, d, q32.data_ptr(), core._p(qlo),
                                        0 if det else sse.data_ptr(), hist.data_ptr(), st), 'vq_gather (cos staged)')
    if det:
        _native.check(lib.vqk_cos_sse_f32(zn.data_ptr(), q32.data_ptr(), n, d, sse.data_ptr(), st), 'cos_sse')
    return idx, q32, qlo, sse, hist, zn, inv_z


def _cos_forward(flat_z, codebook, want_q32: bool, want_lo: bool, want_stats: bool):
    """(idx [N], q fp32 or None, q bf16 or None, sse [1] or None, hist [K] or None): the fused kernel when it serves the codebook,
    the staged formulation otherwise"""
    n, d = flat_z.shape
    k = codebook.shape[0]
    if not cos_fused_serves(codebook):
        return cos_staged(flat_z, codebook, want_lo)[:5]
    dev = flat_z.device
    ws = cos_prepared(codebook)
    sse = hist = None
    if want_stats:
        hist, sse = hist_sse(k, dev)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    q32 = torch.empty((n, d), dtype=torch.float32, device=dev) if want_q32 else None
    qlo = torch.empty((n, d), dtype=torch.bfloat16, device=dev) if want_lo else None
    _native.check(_native.lib().vqk_cos_forward_f32(flat_z.data_ptr(), ws.data_ptr(), ws.numel(), n, k, d, idx.data_ptr(), core._p(q32),
                                                    core._p(qlo), core._p(sse), core._p(hist), core._stream()), 'cos_forward')
    return idx, q32, qlo, sse, hist


def cos_assign(flat_z: torch.Tensor, codebook: torch.Tensor) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N] int64: the forward without q and the statistics"""
    core._require_gpu(flat_z)
    return _cos_forward(core.f32c(flat_z), codebook, False, False, False)[0]


def cos_decode(idx: torch.Tensor, codebook: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """idx [...] int64 -> q [..., D] in ``out_dtype``: the normalised code rows, the bits the forward writes for the same tokens.
    A token outside [0, K) reads nothing and gives a zero row."""
    core._require_gpu(idx)
    k, d = codebook.shape
    ws = _cos_ws(codebook)
    flat = idx.reshape(-1).to(torch.int64).contiguous()
    n = flat.shape[0]
    lo = out_dtype == torch.bfloat16
    q = torch.empty((n, d), dtype=torch.bfloat16 if lo else torch.float32, device=idx.device)
    _native.check(_native.lib().vqk_cos_decode_f32(flat.data_ptr(), ws.data_ptr(), ws.numel(), n, k, d, 0 if lo else q.data_ptr(),
                                                   q.data_ptr() if lo else 0, core._stream()), 'cos_decode')
    return q.view(*idx.shape, d)


class CosLookupFn(torch.autograd.Function):
    """Cosine lookup with the straight-through gradient at the normalised latent and the codebook + commitment losses.
    Returns (q [B,D,H,W] in out_dtype -- the normalised code --, idx [B, H*W] int64, loss 0-dim fp32, hist int32 [K])."""

    @staticmethod
    def forward(ctx, z, codebook, beta: float, out_dtype):
        core._require_gpu(z)
        z, flat, (b, d, h, w) = nhwc_rows(z)
        n = b * h * w
        k = codebook.shape[0]
        lo = out_dtype == torch.bfloat16
        idx, q32, qlo, sse, hist = _cos_forward(flat, codebook, not lo, lo, True)
        q = rows_image(qlo if lo else q32, (b, d, h, w))
        loss = sse.view(()) * ((1.0 + beta) / float(n * d))
        ctx.save_for_backward(z, idx)
        ctx.cfg = (beta, n, k, d)
        ctx.cb_param = codebook
        ctx.mark_non_differentiable(idx, hist)
        ctx.set_materialize_grads(False)                       # an unused output's gradient arrives as None (dq = NULL in the kernel), not as zeros
        return q, idx.view(b, h * w), loss, hist

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist):
        z, idx = ctx.saved_tensors
        beta, n, k, d = ctx.cfg
        cbp = ctx.cb_param
        dz, de, de_tgt, gs, dqc, cz, ce = lookup_backward_frame(ctx, z, dq, dloss, beta, k, ctx.needs_input_grad[1])
        # the codebook is unchanged between forward and backward (the optimizer steps afterwards): the prepared workspace is the forward's
        ws = _cos_ws(cbp)
        if d in COS_FUSED_DIMS:
            lib = _native.lib()
            ws2 = core.grow_ws(_COS_WS, z.device, lib.vqk_cos_backward_ws_bytes(n, d)) if (core.DETERMINISTIC and de is not None) else None
            _native.check(lib.vqk_cos_backward_f32(z.data_ptr(), ws.data_ptr(), idx.data_ptr(), core._p(dqc),
                                                   core.dcode(dqc.dtype) if dqc is not None else core.F32, n, k, d, cz, ce, core._p(gs),
                                                   dz.data_ptr(), core._p(de), core._p(ws2), ws2.numel() if ws2 is not None else 0,
                                                   core._stream()), 'cos_backward')
        else:
            # the shapes the kernel does not serve: the same closed forms as fp32 torch operations (index_add_ in arrival order)
            en, _, inv_e = _ws_views(ws, k, d)
            zn, inv_z = l2norm_rows(z.permute(0, 2, 3, 1).reshape(n, d), want_inv=True)
            q = en[idx]
            g = (zn - q) * (gs * cz) if gs is not None else torch.zeros_like(zn)
            if dqc is not None:
                g = g + dqc.permute(0, 2, 3, 1).reshape(n, d).float()
            dz.permute(0, 2, 3, 1).reshape(n, d).copy_((g - zn * (zn * g).sum(1, keepdim=True)) * inv_z[:, None])
            if de is not None and gs is not None:
                s = torch.zeros((k, d), dtype=torch.float32, device=z.device).index_add_(0, idx, zn)
                de.add_((en * (en * s).sum(1, keepdim=True) - s) * (inv_e * (gs * ce))[:, None])
        return dz, (None if de_tgt is not None else de), None, None


def cos_lookup_staged(z, codebook, beta: float, out_dtype=torch.float32):
    """The staged forward with the closed-form backward written in torch operations: the yardstick tools/cos_bench.py times the
    fused kernels against.  Same returns as CosLookupFn."""
    return _CosStagedFn.apply(z, codebook, beta, out_dtype)


class _CosStagedFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, z, codebook, beta: float, out_dtype):
        core._require_gpu(z)
        z, flat, (b, d, h, w) = nhwc_rows(z)
        n = b * h * w
        k = codebook.shape[0]
        lo = out_dtype == torch.bfloat16
        idx, q32, qlo, sse, hist, zn, inv_z = cos_staged(flat, codebook, lo)
        q = rows_image(qlo if lo else q32, (b, d, h, w))
        loss = sse.view(()) * ((1.0 + beta) / float(n * d))
        ctx.save_for_backward(zn, inv_z, idx, q32)
        ctx.cfg = (beta, n, k, d, b, h, w)
        ctx.cb_param = codebook
        ctx.mark_non_differentiable(idx, hist)
        ctx.set_materialize_grads(False)
        return q, idx.view(b, h * w), loss, hist

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist):
        zn, inv_z, idx, q = ctx.saved_tensors
        beta, n, k, d, b, h, w = ctx.cfg
        en, _, inv_e = _ws_views(_cos_ws(ctx.cb_param), k, d)
        gs = dloss.to(torch.float32) if dloss is not None else None
        scale = 2.0 / float(n * d)
        g = (zn - q) * (gs * (beta * scale)) if gs is not None else torch.zeros_like(zn)
        if dq is not None:
            g = g + core.nhwc(dq).permute(0, 2, 3, 1).reshape(n, d).float()
        dz = ((g - zn * (zn * g).sum(1, keepdim=True)) * inv_z[:, None]).view(b, h, w, d).permute(0, 3, 1, 2)
        de = None
        if ctx.needs_input_grad[1]:
            de = torch.zeros((k, d), dtype=torch.float32, device=zn.device)
            if gs is not None:
                s = torch.zeros_like(de).index_add_(0, idx, zn)
                de = (en * (en * s).sum(1, keepdim=True) - s) * (inv_e * (gs * scale))[:, None]
        return dz, de, None, None


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations', 'hist_sse', 'lookup_backward_frame', 'nhwc_rows', 'prepared_ws', 'rows_image', 'vq_assign')]
