"""SimVQ operators over the vqk C-ABI (csrc/simvq.hip): the autograd Function behind ``SimVectorQuantizer`` plus the projection
launcher and the STAGED formulation of the same definition on existing pieces.  Private part of :mod:`ops` like ``_ops_gvq.py``
(imported at the end of ``ops.py``, which re-exports every name); shared infrastructure is reached through ``core``.

Definition (include/vqk.h, "SimVQ quantizer"): the code table ``codebook`` C [K, D] is frozen, ``proj_weight`` W [D, D] and
``proj_bias`` b [D] (nn.Linear orientation) are learned, the effective codebook is E = C W^T + b; the lookup against E is the
standard quantizer's (assoc 0); loss = (1 + beta) / (N D) sum |q - z|^2; straight-through; dW = g^T C[idx], db = colsum(g) with
g = s 2 / (N D) (q - z); C receives no gradient."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core
from ._ops_vq import hist_sse, lookup_backward_frame, nhwc_rows, rows_image, vq_assign

SIMVQ_FUSED_DIMS = (64, 128, 256)
SIMVQ_ONE_KERNEL_MAX_K = 16384      # D == 256: prepare + one-kernel lookup up to this K, the staged launches beyond (the keep decision)
_SIMVQ_PREP_WS: dict = {}           # _wkey() -> the filter workspace vqk_vq_prepare_f32 derives from E on EVERY forward (core.grow_ws)
_SIMVQ_BWD_WS: dict = {}            # _wkey() -> the per-block D x D + D partials of the backward (core.grow_ws)


def _check_simvq(codebook, proj_weight, proj_bias) -> tuple:
    if codebook.dim() != 2:
        raise ValueError(f'simvq: the code table must be [K, D], got {tuple(codebook.shape)}')
    k, d = codebook.shape
    if tuple(proj_weight.shape) != (d, d):
        raise ValueError(f'simvq: the projection weight must be [{d}, {d}], got {tuple(proj_weight.shape)}')
    if proj_bias is not None and tuple(proj_bias.shape) != (d,):
        raise ValueError(f'simvq: the projection bias must be [{d}], got {tuple(proj_bias.shape)}')
    return k, d


def simvq_fused_serves(codebook) -> bool:
    """the per-call prepare + one-kernel lookup (D == 256) and the two-launch HIP backward serve this code table (D in {64, 128, 256},
    K % 32 == 0, K < 2^26, fp32, contiguous) and are switched on; every other shape goes through :func:`simvq_staged` and the torch
    backward.  The backward met the keep criterion at every measured shape class, the forward where its launches differ from the
    staged ones (profiles/simvq_bench.txt)."""
    k, d = codebook.shape
    return bool(core.SIMVQ_FUSED and d in SIMVQ_FUSED_DIMS and k % 32 == 0 and k < (1 << 26) and codebook.dtype == torch.float32
                and codebook.is_contiguous() and codebook.is_cuda)


def simvq_project_serves(codebook) -> bool:
    """E comes from the HIP projection (vqk_simvq_project_f32) and not from torch.addmm: the shapes :func:`simvq_fused_serves` serves,
    with ``ops.SIMVQ_PROJECT`` on.  OFF by default: measured at N = 8192 the kernel is level with torch.addmm at (K, D) = (8192, 256)
    and 4 to 23 us behind it at (65536, 256), (65536, 128) and (262144, 64) -- no shape class met the keep criterion, so every class
    is routed to the staged projection (profiles/simvq_bench.txt)."""
    return bool(core.SIMVQ_PROJECT and simvq_fused_serves(codebook))


def simvq_project(codebook, proj_weight, proj_bias) -> torch.Tensor:
    """E [K, D] fp32 = C W^T + b by vqk_simvq_project_f32 into a fresh tensor (served shapes only: anything else raises)"""
    core._require_gpu(codebook)
    k, d = _check_simvq(codebook, proj_weight, proj_bias)
    cb, w = core.f32c(codebook), core.f32c(proj_weight)
    b = core.f32c(proj_bias) if proj_bias is not None else None
    e = torch.empty((k, d), dtype=torch.float32, device=cb.device)
    _native.check(_native.lib().vqk_simvq_project_f32(cb.data_ptr(), w.data_ptr(), core._p(b), k, d, e.data_ptr(), core._stream()),
                  'simvq_project')
    return e


def simvq_effective(codebook, proj_weight, proj_bias) -> torch.Tensor:
    """the effective codebook E [K, D] fp32 of the CURRENT parameters (detached, a fresh tensor): the HIP projection where
    :func:`simvq_project_serves` routes to it, torch.addmm otherwise -- the call the forward makes, so the rows are the forward's bits"""
    _check_simvq(codebook, proj_weight, proj_bias)
    core._require_gpu(codebook)
    if simvq_project_serves(codebook):
        return simvq_project(codebook, proj_weight, proj_bias)
    cb, w = core.f32c(codebook), core.f32c(proj_weight)
    return torch.addmm(core.f32c(proj_bias), cb, w.t()) if proj_bias is not None else cb @ w.t()


def _gather(flat_z, e, idx, want_q32: bool, want_lo: bool, want_stats: bool):
    """vqk_vq_gather_f32 on (z, E, idx): (q fp32 or None, q bf16 or None, sse [1] or None, hist [K] or None).  The gather kernel keeps
    its histogram in LDS up to 16384 codes; beyond, the tokens are counted by vqk_simvq_hist_i32."""
    n, d = flat_z.shape
    k = e.shape[0]
    dev = flat_z.device
    lib, st = _native.lib(), core._stream()
    sse = hist = None
    if want_stats:
        hist, sse = hist_sse(k, dev)
    q32 = torch.empty((n, d), dtype=torch.float32, device=dev)         # (the gather kernel always writes its fp32 q)
    qlo = torch.empty((n, d), dtype=torch.bfloat16, device=dev) if want_lo else None
    in_gather = hist is not None and k <= 16384
    _native.check(lib.vqk_vq_gather_f32(flat_z.data_ptr(), e.data_ptr(), idx.data_ptr(), n, k, d, core._p(q32), core._p(qlo), core._p(sse),
                                        core._p(hist) if in_gather else 0, st), 'vq_gather (simvq)')
    if hist is not None and not in_gather:
        _native.check(lib.vqk_simvq_hist_i32(idx.data_ptr(), n, k, hist.data_ptr(), st), 'simvq_hist')
    return q32, qlo, sse, hist


def _simvq_lookup(flat_z, e, want_q32: bool, want_lo: bool, want_stats: bool):
    """the standard lookup (assoc 0) of rows flat_z [N, D] against a FRESH E [K, D]: (idx [N], q fp32 or None, q bf16 or None, sse [1]
    or None, hist [K] or None).  D == 256: vqk_vq_prepare_f32 into a workspace this operator owns -- on every call, inside a captured
    step too, with no entry in the prepared-workspace tables: E is written by a kernel without a version bump, a cached preparation
    could be ranked against after E moved -- then the one-kernel vqk_vq_forward_f32.  D 64 / 128, and D == 256 beyond
    SIMVQ_ONE_KERNEL_MAX_K codes (measured there: no gap to the staged launches outside the run-to-run spread): ops.vq_assign, which
    derives everything it ranks with from E on every call as well, + vqk_vq_gather_f32."""
    n, d = flat_z.shape
    k = e.shape[0]
    dev = flat_z.device
    lib = _native.lib()
    if d == 256 and k % 32 == 0 and k <= SIMVQ_ONE_KERNEL_MAX_K:
        ws = core.grow_ws(_SIMVQ_PREP_WS, dev, lib.vqk_vq_filter_ws_bytes(k, d))
        st = core._stream()
        _native.check(lib.vqk_vq_prepare_f32(e.data_ptr(), k, d, ws.data_ptr(), ws.numel(), st), 'vq_prepare (simvq)')
        sse = hist = None
        if want_stats:
            hist, sse = hist_sse(k, dev)
        idx = torch.empty(n, dtype=torch.int64, device=dev)
        q32 = torch.empty((n, d), dtype=torch.float32, device=dev) if want_q32 else None
        qlo = torch.empty((n, d), dtype=torch.bfloat16, device=dev) if want_lo else None
        _native.check(lib.vqk_vq_forward_f32(flat_z.data_ptr(), e.data_ptr(), ws.data_ptr(), ws.numel(), n, k, d, 0, idx.data_ptr(),
                                             core._p(q32), core._p(qlo), core._p(sse), core._p(hist), st), 'vq_forward (simvq)')
        return idx, q32, qlo, sse, hist
    idx = vq_assign(flat_z, e, 0)
    if not (want_q32 or want_lo or want_stats):
        return idx, None, None, None, None
    return (idx,) + _gather(flat_z, e, idx, want_q32, want_lo, want_stats)


def simvq_staged(flat_z: torch.Tensor, codebook, proj_weight, proj_bias, want_lo: bool = False):
    """The definition on existing pieces: E by ``torch.addmm``, then ``ops.vq_assign(z, E, 0)`` and vqk_vq_gather_f32 on it.  The
    product path of the shapes the HIP projection does not serve (other D, K not a multiple of 32) and the yardstick of
    tools/simvq_bench.py.  flat_z [N, D] fp32 -> (E [K, D], idx [N] int64, q [N, D] fp32, q as bf16 or None, sse [1], hist [K] int32)."""
    core._require_gpu(flat_z)
    k, d = _check_simvq(codebook, proj_weight, proj_bias)
    if flat_z.dim() != 2 or flat_z.shape[1] != d:
        raise ValueError(f'simvq: latents must be [N, {d}], got {tuple(flat_z.shape)}')
    cb, w = core.f32c(codebook), core.f32c(proj_weight)
    e = torch.addmm(core.f32c(proj_bias), cb, w.t()) if proj_bias is not None else cb @ w.t()
    idx = vq_assign(flat_z, e, 0)
    q32, qlo, sse, hist = _gather(flat_z, e, idx, True, want_lo, True)
    return e, idx, q32, qlo, sse, hist


def simvq_assign(flat_z: torch.Tensor, codebook, proj_weight, proj_bias) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N] int64: project and rank, without q and the statistics"""
    core._require_gpu(flat_z)
    e = simvq_effective(codebook, proj_weight, proj_bias)
    flat_z = core.f32c(flat_z)
    if simvq_fused_serves(codebook):
        return _simvq_lookup(flat_z, e, False, False, False)[0]
    return vq_assign(flat_z, e, 0)


def simvq_backward_staged(flat_z, e, cb, idx, dq_rows, cz_s, ce_s):
    """the closed-form backward as fp32 torch operations: (dz rows [N, D], dW [D, D], db [D]) with cz_s = s cz and ce_s = s ce as 0-dim
    tensors or floats; the codebook-sized scatter target and the D x K x D product are what the HIP pair avoids"""
    k, d = e.shape
    diff = flat_z - e[idx]
    dz = diff * cz_s
    if dq_rows is not None:
        dz = dz + dq_rows.float()
    de = torch.zeros((k, d), dtype=torch.float32, device=e.device).index_add_(0, idx, diff)
    de = de * (-ce_s)
    return dz, de.t() @ cb, de.sum(0)


class SimVQLookupFn(torch.autograd.Function):
    """Nearest-code lookup against the effective codebook E = C W^T + b with the straight-through gradient and the codebook +
    commitment losses.  Returns (q [B,D,H,W] in out_dtype, idx [B, H*W] int64, loss 0-dim fp32, hist int32 [K])."""

    @staticmethod
    def forward(ctx, z, codebook, proj_weight, proj_bias, beta: float, out_dtype):
        core._require_gpu(z)
        k, d = _check_simvq(codebook, proj_weight, proj_bias)
        z, flat, (b, dz_, h, w) = nhwc_rows(z)
        if dz_ != d:
            raise ValueError(f'simvq: latents must have {d} channels, got {dz_}')
        n = b * h * w
        lo = out_dtype == torch.bfloat16
        fused = simvq_fused_serves(codebook)
        cb = core.f32c(codebook)
        if fused:
            e = simvq_effective(cb, proj_weight, proj_bias)        # a fresh E on every call, saved below
            idx, q32, qlo, sse, hist = _simvq_lookup(flat, e, not lo, lo, True)
        else:
            e, idx, q32, qlo, sse, hist = simvq_staged(flat, cb, proj_weight, proj_bias, lo)
        q = rows_image(qlo if lo else q32, (b, d, h, w))
        loss = sse.view(()) * ((1.0 + beta) / float(n * d))
        ctx.save_for_backward(z, e, cb, idx)
        ctx.cfg = (beta, n, k, d, fused)
        ctx.w_param, ctx.b_param = proj_weight, proj_bias
        ctx.mark_non_differentiable(idx, hist)
        ctx.set_materialize_grads(False)                       # an unused output's gradient arrives as None (dq = NULL in the kernel), not as zeros
        return q, idx.view(b, h * w), loss, hist

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist):
        z, e, cb, idx = ctx.saved_tensors
        beta, n, k, d, fused = ctx.cfg
        dz, _, _, gs, dqc, cz, ce = lookup_backward_frame(ctx, z, dq, dloss, beta, k, False)
        want_w = ctx.needs_input_grad[2]
        want_b = ctx.b_param is not None and ctx.needs_input_grad[3]
        # dW / db are accumulated (old + sum) straight into the optimizer's arena where it offers a view
        dw_tgt = core.direct_grad(ctx.w_param) if (want_w and ctx.w_param.is_contiguous()) else None
        db_tgt = core.direct_grad(ctx.b_param) if (want_b and ctx.b_param.is_contiguous()) else None
        dw = dw_tgt if dw_tgt is not None else torch.zeros((d, d), dtype=torch.float32, device=z.device)
        db = db_tgt if db_tgt is not None else (torch.zeros(d, dtype=torch.float32, device=z.device) if want_b else None)
        if fused:
            lib = _native.lib()
            ws = core.grow_ws(_SIMVQ_BWD_WS, z.device, lib.vqk_simvq_backward_ws_bytes(n, d))
            _native.check(lib.vqk_simvq_backward_f32(z.data_ptr(), e.data_ptr(), cb.data_ptr(), idx.data_ptr(), core._p(dqc),
                                                     core.dcode(dqc.dtype) if dqc is not None else core.F32, n, k, d, cz, ce,
                                                     core._p(gs), dz.data_ptr(), dw.data_ptr(), core._p(db), ws.data_ptr(), ws.numel(),
                                                     core._stream()), 'simvq_backward')
        else:
            zf = z.permute(0, 2, 3, 1).reshape(n, d)
            dqr = dqc.permute(0, 2, 3, 1).reshape(n, d) if dqc is not None else None
            if gs is not None:
                dzr, dws, dbs = simvq_backward_staged(zf, e, cb, idx, dqr, gs * cz, gs * ce)
                dw.add_(dws)
                if db is not None:
                    db.add_(dbs)
            else:
                dzr = dqr.float() if dqr is not None else torch.zeros_like(zf)
            dz.permute(0, 2, 3, 1).reshape(n, d).copy_(dzr)
        return (dz, None, (dw if want_w and dw_tgt is None else None), (db if want_b and db_tgt is None else None), None, None)


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations', 'hist_sse', 'lookup_backward_frame', 'nhwc_rows', 'rows_image', 'vq_assign')]
