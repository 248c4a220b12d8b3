"""Finite-scalar-quantizer operators over the vqk C-ABI (csrc/fsq.hip): the autograd Function behind ``FSQuantizer`` plus the
assignment-only and decode launchers.  Private part of :mod:`ops` like ``_ops_vq.py`` (imported at the end of ``ops.py``, which
re-exports every name); shared infrastructure is reached through ``core``."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _native
from . import ops as core

_FSQ_WS: dict = {}


def _levels_arg(levels):
    """the levels as the host int array the launchers pass by value, and K = prod(levels)"""
    levels = [int(v) for v in levels]
    if not 1 <= len(levels) <= 8:
        raise ValueError('fsq: between 1 and 8 levels')
    return (ctypes.c_int32 * 8)(*levels), len(levels), math.prod(levels)


def _fsq_ws(device, nbytes: int) -> torch.Tensor:
    """slab workspace of vqk_fsq_backward, one per (device, stream, host thread): plain stores + ordered sums, no atomics"""
    core._stream()
    key = core._wkey(device)
    ws = _FSQ_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _FSQ_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _weights(w_in, w_out, d: int):
    """the [d, D] / [D, d] memory of the two 1x1 projections (Conv2d weights [O, I, 1, 1], or plain matrices)"""
    dm = w_in.numel() // d
    if w_in.numel() != d * dm or w_out.numel() != d * dm or w_in.shape[0] != d or w_out.shape[0] != dm:
        raise RuntimeError(f'vqk: fsq projections {tuple(w_in.shape)} / {tuple(w_out.shape)} do not match {d} levels')
    return dm


def _f32c(t):
    t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


def fsq_assign(flat_z: torch.Tensor, w_in: torch.Tensor, b_in: torch.Tensor, levels) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N] int64: the forward kernel without q and u"""
    core._require_gpu(flat_z)
    lv, d, _ = _levels_arg(levels)
    n, dm = flat_z.shape
    flat_z = _f32c(flat_z)
    idx = torch.empty(n, dtype=torch.int64, device=flat_z.device)
    _native.check(_native.lib().vqk_fsq_forward(flat_z.data_ptr(), _f32c(w_in).data_ptr(), _f32c(b_in).data_ptr(), 0, 0, n, dm, d, lv,
                                                idx.data_ptr(), 0, 0, 0, 0, core._stream()), 'fsq_forward (assign)')
    return idx


def fsq_decode(idx: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, levels, out_dtype=torch.float32) -> torch.Tensor:
    """idx [...] int64 -> q [..., D] in ``out_dtype``: the bits the forward writes for the same index"""
    core._require_gpu(idx)
    lv, d, _ = _levels_arg(levels)
    dm = w_out.numel() // d
    flat = idx.reshape(-1).to(torch.int64).contiguous()
    q = torch.empty((flat.numel(), dm), dtype=out_dtype, device=idx.device)
    lo = out_dtype == torch.bfloat16
    _native.check(_native.lib().vqk_fsq_decode(flat.data_ptr(), _f32c(w_out).data_ptr(), _f32c(b_out).data_ptr(), flat.numel(), dm, d, lv,
                                               0 if lo else q.data_ptr(), q.data_ptr() if lo else 0, core._stream()), 'fsq_decode')
    return q.view(*idx.shape, dm)


class FSQFn(torch.autograd.Function):
    """Finite scalar quantization with the straight-through gradient: project to len(levels) channels, tanh-bound, round,
    project back.  One forward kernel; the backward is one kernel + the ordered slab sum (bitwise reproducible in every mode).
    Returns (q [B,D,H,W] in out_dtype, idx [B, H*W] int64, loss 0-dim fp32 zero, hist int32 [K])."""

    @staticmethod
    def forward(ctx, z, w_in, b_in, w_out, b_out, levels, out_dtype):
        core._require_gpu(z)
        z = core.nhwc(z.to(torch.float32))
        b, dm, h, w = z.shape
        n = b * h * w
        lv, d, k = _levels_arg(levels)
        if _weights(w_in, w_out, d) != dm:
            raise RuntimeError(f'vqk: fsq projections are for {w_in.numel() // d} channels, the latent map has {dm}')
        wi, bi, wo, bo = _f32c(w_in), _f32c(b_in), _f32c(w_out), _f32c(b_out)
        flat = z.permute(0, 2, 3, 1).reshape(n, dm)          # a view: NHWC memory is already [N][D]
        lo = out_dtype == torch.bfloat16
        q = core.empty_nhwc(b, dm, h, w, torch.bfloat16 if lo else torch.float32, z.device)
        zbuf = torch.zeros(k + 1, dtype=torch.int32, device=z.device)            # histogram | the zero loss: one fill launch
        hist, loss = zbuf[:k], zbuf[k:].view(torch.float32).view(())
        idx = torch.empty(n, dtype=torch.int64, device=z.device)
        u = torch.empty((n, d), dtype=torch.float32, device=z.device)
        _native.check(_native.lib().vqk_fsq_forward(flat.data_ptr(), wi.data_ptr(), bi.data_ptr(), wo.data_ptr(), bo.data_ptr(), n, dm,
                                                    d, lv, idx.data_ptr(), u.data_ptr(), 0 if lo else q.data_ptr(),
                                                    q.data_ptr() if lo else 0, hist.data_ptr(), core._stream()), 'fsq_forward')
        ctx.save_for_backward(z, u, wi, wo)
        ctx.cfg = (tuple(int(v) for v in levels), n, dm, d)
        ctx.params = (w_in, b_in, w_out, b_out)
        ctx.mark_non_differentiable(idx, loss, hist)
        return q, idx.view(b, h * w), loss, hist

    @staticmethod
    def backward(ctx, dq, _didx, _dloss, _dhist):
        z, u, wi, wo = ctx.saved_tensors
        levels, n, dm, d = ctx.cfg
        lv = _levels_arg(levels)[0]
        dqc = core.nhwc(dq) if dq is not None else torch.zeros_like(z, memory_format=core._CL)
        if dqc.dtype not in (torch.float32, torch.bfloat16):
            dqc = dqc.to(torch.float32)
        dz = torch.empty_like(z, memory_format=core._CL)
        # the parameter gradients go straight into the optimizer's arena when every one of the four has a place there
        tgt = [core.direct_grad(p) if p.is_contiguous() else None for p in ctx.params]
        direct = all(t is not None for t in tgt)
        if not direct:
            tgt = [torch.empty_like(p, dtype=torch.float32, memory_format=torch.contiguous_format) for p in ctx.params]
        lib = _native.lib()
        nbytes = lib.vqk_fsq_backward_ws_bytes(n, dm, d)
        ws = _fsq_ws(z.device, nbytes)
        _native.check(lib.vqk_fsq_backward(z.data_ptr(), u.data_ptr(), dqc.data_ptr(), core.dcode(dqc.dtype), wi.data_ptr(), wo.data_ptr(),
                                           n, dm, d, lv, dz.data_ptr(), tgt[0].data_ptr(), tgt[1].data_ptr(), tgt[2].data_ptr(),
                                           tgt[3].data_ptr(), int(direct), ws.data_ptr(), ws.numel(), core._stream()), 'fsq_backward')
        if direct:
            return dz, None, None, None, None, None, None
        grads = [t.view(p.shape) if ctx.needs_input_grad[i + 1] else None for i, (t, p) in enumerate(zip(tgt, ctx.params))]
        return (dz, *grads, None, None)


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations', 'ctypes', 'math')]
