"""Grouped-quantizer operators over the vqk C-ABI (csrc/gvq.hip): the autograd Function behind ``GroupedVectorQuantizer`` plus the
assignment-only and decode launchers, and the STAGED formulation of the same definition on the standard quantizer's operators.
Private part of :mod:`ops` like ``_ops_cos.py`` (imported at the end of ``ops.py``, which re-exports every name); shared
infrastructure is reached through ``core``.

Definition (include/vqk.h, "grouped quantizer"): the D = G d channels of a latent row are cut into G contiguous groups, group g is
looked up in its own codebook -- rows g K .. (g + 1) K - 1 of ``codebook`` [G K, d] -- with the standard quantizer's argmin (assoc 0);
q = the concatenation of the G code rows; loss = (1 + beta) / (N D) sum |q - z|^2; tokens [N, G]; hist [G K]."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core
from ._ops_vq import hist_sse, lookup_backward_frame, nhwc_rows, rows_image, vq_assign

GVQ_MAX_GROUPS = 16
GVQ_FUSED_DIMS = (8, 16, 32, 64)
_GVQ_WS: dict = {}                  # _wkey() -> the per-row terms and ids of the deterministic backward (core.grow_ws)


def _check_groups(codebook, groups: int) -> tuple:
    """(K, d) of ``codebook`` [G K, d] for ``groups`` = G"""
    groups = int(groups)
    if not 1 <= groups <= GVQ_MAX_GROUPS:
        raise ValueError(f'grouped quantizer: groups must be between 1 and {GVQ_MAX_GROUPS}, got {groups}')
    if codebook.dim() != 2 or codebook.shape[0] % groups != 0:
        raise ValueError(f'grouped quantizer: the codebook must be [groups * K, d], got {tuple(codebook.shape)} for groups = {groups}')
    return codebook.shape[0] // groups, codebook.shape[1]


def gvq_fused_serves(codebook, groups: int) -> bool:
    """the one-launch forward and the flat-row backward serve this codebook (d in {8, 16, 32, 64}, K % 32 == 0, fp32, contiguous) and
    are switched on.  Every served shape measured faster than the staged formulation (profiles/gvq_bench.txt), so none is routed away."""
    k, d = _check_groups(codebook, groups)
    return bool(core.GVQ_FUSED and d in GVQ_FUSED_DIMS and k % 32 == 0 and codebook.dtype == torch.float32 and codebook.is_contiguous()
                and codebook.is_cuda)


def gvq_staged(flat_z: torch.Tensor, codebook: torch.Tensor, groups: int, want_lo: bool = False):
    """The definition built from the stand-alone operators, per group on contiguous copies of the slices: ``ops.vq_assign(z_g, e_g, 0)``
    (vqk_row_sqnorm_f32 twice + vqk_vq_assign_f32) and vqk_vq_gather_f32, 4 launches and a slice copy each way per group.  The product
    path of the shapes the fused kernels do not serve (other d, K not a multiple of 32), and what the fused forward must equal bit
    for bit in idx, q and hist (its sum of squares arrives in another order).
    flat_z [N, G d] fp32 -> (idx [N, G] int64, q [N, G d] fp32, q as bf16 or None, sse [1] fp32, hist [G K] int32)."""
    core._require_gpu(flat_z)
    k, d = _check_groups(codebook, groups)
    n = flat_z.shape[0]
    if flat_z.shape[1] != groups * d:
        raise ValueError(f'grouped quantizer: latents must be [N, {groups * d}], got {tuple(flat_z.shape)}')
    dev = flat_z.device
    lib, st = _native.lib(), core._stream()
    cb = core.f32c(codebook)
    hist, sse = hist_sse(groups * k, dev)
    idx = torch.empty((n, groups), dtype=torch.int64, device=dev)
    q32 = torch.empty((n, groups * d), dtype=torch.float32, device=dev)
    qlo = torch.empty((n, groups * d), dtype=torch.bfloat16, device=dev) if want_lo else None
    for g in range(groups):
        zg = flat_z[:, g * d:(g + 1) * d].contiguous()
        eg = cb[g * k:(g + 1) * k]
        ig = vq_assign(zg, eg, 0)
        qg = torch.empty((n, d), dtype=torch.float32, device=dev)
        qlg = torch.empty((n, d), dtype=torch.bfloat16, device=dev) if want_lo else None
        _native.check(lib.vqk_vq_gather_f32(zg.data_ptr(), eg.data_ptr(), ig.data_ptr(), n, k, d, qg.data_ptr(), core._p(qlg),
                                            sse.data_ptr(), hist[g * k:].data_ptr(), st), 'vq_gather (gvq staged)')
        idx[:, g] = ig
        q32[:, g * d:(g + 1) * d] = qg
        if want_lo:
            qlo[:, g * d:(g + 1) * d] = qlg
    return idx, q32, qlo, sse, hist


def _gvq_forward(flat_z, codebook, groups: int, want_q32: bool, want_lo: bool, want_stats: bool):
    """(idx [N, G], q fp32 or None, q bf16 or None, sse [1] or None, hist [G K] or None): the fused kernel when it serves the
    codebook, the staged formulation otherwise"""
    if not gvq_fused_serves(codebook, groups):
        return gvq_staged(flat_z, codebook, groups, want_lo)
    k, d = _check_groups(codebook, groups)
    n = flat_z.shape[0]
    if flat_z.shape[1] != groups * d:
        raise ValueError(f'grouped quantizer: latents must be [N, {groups * d}], got {tuple(flat_z.shape)}')
    dev = flat_z.device
    lib, st = _native.lib(), core._stream()
    cb = codebook.detach()
    sse = hist = None
    if want_stats:
        hist, sse = hist_sse(groups * k, dev)
    # |e|^2 of the CURRENT codebook on every call: one small launch, nothing cached that a captured step could see go stale
    e2 = torch.empty(groups * k, dtype=torch.float32, device=dev)
    _native.check(lib.vqk_row_sqnorm_f32(cb.data_ptr(), groups * k, d, e2.data_ptr(), st), 'row_sqnorm(e)')
    idx = torch.empty((n, groups), dtype=torch.int64, device=dev)
    q32 = torch.empty((n, groups * d), dtype=torch.float32, device=dev) if want_q32 else None
    qlo = torch.empty((n, groups * d), dtype=torch.bfloat16, device=dev) if want_lo else None
    _native.check(lib.vqk_gvq_forward_f32(flat_z.data_ptr(), cb.data_ptr(), e2.data_ptr(), n, k, d, groups, idx.data_ptr(), core._p(q32),
                                          core._p(qlo), core._p(sse), core._p(hist), st), 'gvq_forward')
    return idx, q32, qlo, sse, hist


def gvq_assign(flat_z: torch.Tensor, codebook: torch.Tensor, groups: int) -> torch.Tensor:
    """flat_z [N, G d] fp32 -> idx [N, G] int64: the forward without q and the statistics"""
    core._require_gpu(flat_z)
    return _gvq_forward(core.f32c(flat_z), codebook, groups, False, False, False)[0]


def gvq_decode(idx: torch.Tensor, codebook: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """idx [..., G] int64 -> q [..., G d] in ``out_dtype``: the concatenated code rows, the bits the forward writes for the same
    tokens.  A token outside [0, K) gives a zero slice; the other groups' slices of the row are untouched by it."""
    core._require_gpu(idx)
    groups = idx.shape[-1]
    k, d = _check_groups(codebook, groups)
    if d % 4:
        raise ValueError(f'grouped quantizer: the group width must be a multiple of 4, got {d}')
    cb = core.f32c(codebook)
    flat = idx.reshape(-1, groups).to(torch.int64).contiguous()
    n = flat.shape[0]
    lo = out_dtype == torch.bfloat16
    q = torch.empty((n, groups * d), dtype=torch.bfloat16 if lo else torch.float32, device=idx.device)
    _native.check(_native.lib().vqk_gvq_decode_f32(flat.data_ptr(), cb.data_ptr(), n, k, d, groups, 0 if lo else q.data_ptr(),
                                                   q.data_ptr() if lo else 0, core._stream()), 'gvq_decode')
    return q.view(*idx.shape[:-1], groups * d)


class GVQLookupFn(torch.autograd.Function):
    """Per-group nearest-code lookup with the straight-through gradient and the codebook + commitment losses.
    Returns (q [B,D,H,W] in out_dtype, idx [B, H*W, G] int64, loss 0-dim fp32, hist int32 [G K])."""

    @staticmethod
    def forward(ctx, z, codebook, beta: float, groups: int, out_dtype):
        core._require_gpu(z)
        groups = int(groups)
        k, dg = _check_groups(codebook, groups)
        z, flat, (b, d, h, w) = nhwc_rows(z)
        n = b * h * w
        lo = out_dtype == torch.bfloat16
        fused = gvq_fused_serves(codebook, groups)
        idx, q32, qlo, sse, hist = _gvq_forward(flat, codebook, groups, not lo, lo, True)
        q = rows_image(qlo if lo else q32, (b, d, h, w))
        loss = sse.view(()) * ((1.0 + beta) / float(n * d))
        ctx.save_for_backward(z, core.f32c(codebook), idx)
        ctx.cfg = (beta, n, k, dg, groups, fused)
        ctx.cb_param = codebook
        ctx.mark_non_differentiable(idx, hist)
        ctx.set_materialize_grads(False)                       # an unused output's gradient arrives as None (dq = NULL in the kernel), not as zeros
        return q, idx.view(b, h * w, groups), loss, hist

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist):
        z, cb, idx = ctx.saved_tensors
        beta, n, k, dg, groups, fused = ctx.cfg
        # the frame sizes a fresh codebook gradient as [K, D]: the same G K d floats, viewed as the parameter's [G K, d] below
        dz, de, de_tgt, gs, dqc, cz, ce = lookup_backward_frame(ctx, z, dq, dloss, beta, k, ctx.needs_input_grad[1])
        if de is not None and de_tgt is None:
            de = de.view(groups * k, dg)
        if fused:
            lib = _native.lib()
            det = core.DETERMINISTIC and de is not None
            ws = core.grow_ws(_GVQ_WS, z.device, lib.vqk_gvq_backward_ws_bytes(n, dg, groups)) if det else None
            _native.check(lib.vqk_gvq_backward_f32(z.data_ptr(), cb.data_ptr(), idx.data_ptr(), core._p(dqc),
                                                   core.dcode(dqc.dtype) if dqc is not None else core.F32, n, k, dg, groups, cz, ce,
                                                   core._p(gs), dz.data_ptr(), core._p(de), core._p(ws),
                                                   ws.numel() if ws is not None else 0, core._stream()), 'gvq_backward')
        else:
            # the shapes the kernels do not serve (and the staged yardstick): the same closed forms as fp32 torch operations on the
            # flat view [N G, d] with global code ids (index_add_ in arrival order)
            gidx = (idx + torch.arange(groups, device=idx.device) * k).reshape(-1)
            zf = z.permute(0, 2, 3, 1).reshape(n * groups, dg)
            diff = zf - cb[gidx]
            g = diff * (gs * cz) if gs is not None else torch.zeros_like(zf)
            if dqc is not None:
                g = g + dqc.permute(0, 2, 3, 1).reshape(n * groups, dg).float()
            dz.permute(0, 2, 3, 1).reshape(n * groups, dg).copy_(g)
            if de is not None and gs is not None:
                s = torch.zeros((groups * k, dg), dtype=torch.float32, device=z.device).index_add_(0, gidx, diff)
                de.sub_(s * (gs * ce))
        return dz, (None if de_tgt is not None else de), None, None, None


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations', 'hist_sse', 'lookup_backward_frame', 'nhwc_rows', 'rows_image', 'vq_assign')]
