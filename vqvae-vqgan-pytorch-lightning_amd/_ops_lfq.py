"""Lookup-free-quantizer operators over the vqk C-ABI (csrc/lfq.hip): the autograd Function behind ``LFQuantizer`` plus the
assignment-only and decode launchers.  Private part of :mod:`ops` like ``_ops_fsq.py`` (imported at the end of ``ops.py``, which
re-exports every name); shared infrastructure is reached through ``core``."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core
from ._ops_fsq import _f32c

LFQ_MAX_BITS = 18
LFQ_MAX_GROUP_BITS = 10
_LFQ_WS: dict = {}


def _lfq_ws(device, nbytes: int) -> torch.Tensor:
    """slab workspace of vqk_lfq_forward / vqk_lfq_backward, one per (device, stream, host thread): plain stores + ordered sums"""
    core._stream()
    key = core._wkey(device)
    ws = _LFQ_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _LFQ_WS[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    return ws


def _lfq_bits(bits: int) -> int:
    bits = int(bits)
    if not 1 <= bits <= LFQ_MAX_BITS:
        raise ValueError(f'lfq: bits must be between 1 and {LFQ_MAX_BITS}, got {bits}')
    return bits


def _lfq_dm(w_in, w_out, d: int) -> int:
    """D of the [d, D] / [D, d] memory of the two 1x1 projections (Conv2d weights [O, I, 1, 1], or plain matrices)"""
    dm = w_in.numel() // d
    if w_in.numel() != d * dm or w_out.numel() != d * dm or w_in.shape[0] != d or w_out.shape[0] != dm:
        raise RuntimeError(f'vqk: lfq projections {tuple(w_in.shape)} / {tuple(w_out.shape)} do not match {d} bits')
    return dm


def lfq_assign(flat_z: torch.Tensor, w_in: torch.Tensor, b_in: torch.Tensor, bits: int) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N] int64: the forward kernel without q, u, loss and workspace"""
    core._require_gpu(flat_z)
    d = _lfq_bits(bits)
    n, dm = flat_z.shape
    flat_z = _f32c(flat_z)
    idx = torch.empty(n, dtype=torch.int64, device=flat_z.device)
    _native.check(_native.lib().vqk_lfq_forward(flat_z.data_ptr(), _f32c(w_in).data_ptr(), _f32c(b_in).data_ptr(), 0, 0, n, dm, d, 1, 1.0,
                                                0.0, 0.0, 0.0, idx.data_ptr(), 0, 0, 0, 0, 0, 0, 0, 0, core._stream()), 'lfq_forward (assign)')
    return idx


def lfq_decode(idx: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, bits: int, out_dtype=torch.float32) -> torch.Tensor:
    """idx [...] int64 -> q [..., D] in ``out_dtype``: the bits the forward writes for the same index"""
    core._require_gpu(idx)
    d = _lfq_bits(bits)
    dm = w_out.numel() // d
    flat = idx.reshape(-1).to(torch.int64).contiguous()
    q = torch.empty((flat.numel(), dm), dtype=out_dtype, device=idx.device)
    lo = out_dtype == torch.bfloat16
    _native.check(_native.lib().vqk_lfq_decode(flat.data_ptr(), _f32c(w_out).data_ptr(), _f32c(b_out).data_ptr(), flat.numel(), dm, d,
                                               0 if lo else q.data_ptr(), q.data_ptr() if lo else 0, core._stream()), 'lfq_decode')
    return q.view(*idx.shape, dm)


class LFQFn(torch.autograd.Function):
    """Lookup-free quantization (MAGVIT-v2): project to ``bits`` channels, take the sign, project back; straight-through gradient at
    the projected latent plus the true gradient of loss = beta commit + ratio (H_sample - gamma H_batch).  Forward: one kernel + the
    ordered finish; backward: one kernel + the ordered slab sum (bitwise reproducible in every mode).  ``cfg`` = (bits, group_bits,
    beta, ratio, gamma, tau).  Returns (q [B,D,H,W] in out_dtype, idx [B, H*W] int64, loss 0-dim fp32 differentiable, hist int32 [K],
    parts fp32 [3] = commit, H_sample, H_batch)."""

    @staticmethod
    def forward(ctx, z, w_in, b_in, w_out, b_out, cfg, out_dtype):
        core._require_gpu(z)
        d, g, beta, ratio, gamma, tau = int(cfg[0]), int(cfg[1]), float(cfg[2]), float(cfg[3]), float(cfg[4]), float(cfg[5])
        d = _lfq_bits(d)
        if not 1 <= g <= LFQ_MAX_GROUP_BITS:
            raise ValueError(f'lfq: ent_group_bits must be between 1 and {LFQ_MAX_GROUP_BITS}, got {g}')
        z = core.nhwc(z.to(torch.float32))
        b, dm, h, w = z.shape
        n = b * h * w
        k = 1 << d
        if _lfq_dm(w_in, w_out, d) != dm:
            raise RuntimeError(f'vqk: lfq projections are for {w_in.numel() // d} channels, the latent map has {dm}')
        wi, bi, wo, bo = _f32c(w_in), _f32c(b_in), _f32c(w_out), _f32c(b_out)
        flat = z.permute(0, 2, 3, 1).reshape(n, dm)          # a view: NHWC memory is already [N][D]
        lo = out_dtype == torch.bfloat16
        q = core.empty_nhwc(b, dm, h, w, torch.bfloat16 if lo else torch.float32, z.device)
        hist = torch.zeros(k, dtype=torch.int32, device=z.device)
        idx = torch.empty(n, dtype=torch.int64, device=z.device)
        u = torch.empty((n, d), dtype=torch.float32, device=z.device)
        out = torch.empty(4, dtype=torch.float32, device=z.device)
        ltab = torch.empty(((d + g - 1) // g) << g, dtype=torch.float32, device=z.device)
        lib = _native.lib()
        nbytes = lib.vqk_lfq_ws_bytes(n, dm, d, g)
        if nbytes < 0:
            _native.check(int(nbytes), 'lfq_ws_bytes')
        ws = _lfq_ws(z.device, nbytes)
        _native.check(lib.vqk_lfq_forward(flat.data_ptr(), wi.data_ptr(), bi.data_ptr(), wo.data_ptr(), bo.data_ptr(), n, dm, d, g, tau,
                                          beta, ratio, gamma, idx.data_ptr(), u.data_ptr(), 0 if lo else q.data_ptr(),
                                          q.data_ptr() if lo else 0, hist.data_ptr(), out.data_ptr(), ltab.data_ptr(), ws.data_ptr(),
                                          ws.numel(), core._stream()), 'lfq_forward')
        ctx.save_for_backward(z, u, wi, wo, ltab)
        ctx.cfg = (n, dm, d, g, beta, ratio, gamma, tau)
        ctx.params = (w_in, b_in, w_out, b_out)
        loss, parts = out[0], out[1:]
        ctx.mark_non_differentiable(idx, hist, parts)
        return q, idx.view(b, h * w), loss, hist, parts

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist, _dparts):
        z, u, wi, wo, ltab = ctx.saved_tensors
        n, dm, d, g, beta, ratio, gamma, tau = ctx.cfg
        dqc = core.nhwc(dq) if dq is not None else torch.zeros_like(z, memory_format=core._CL)
        if dqc.dtype not in (torch.float32, torch.bfloat16):
            dqc = dqc.to(torch.float32)
        # the loss cotangent stays on the device (a captured graph follows it); an unused loss contributes nothing
        gs = dloss.to(torch.float32).contiguous() if dloss is not None else torch.zeros((), dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z, memory_format=core._CL)
        # the parameter gradients go straight into the optimizer's arena when every one of the four has a place there
        tgt = [core.direct_grad(p) if p.is_contiguous() else None for p in ctx.params]
        direct = all(t is not None for t in tgt)
        if not direct:
            tgt = [torch.empty_like(p, dtype=torch.float32, memory_format=torch.contiguous_format) for p in ctx.params]
        lib = _native.lib()
        ws = _lfq_ws(z.device, lib.vqk_lfq_ws_bytes(n, dm, d, g))
        _native.check(lib.vqk_lfq_backward(z.data_ptr(), u.data_ptr(), dqc.data_ptr(), core.dcode(dqc.dtype), wi.data_ptr(), wo.data_ptr(),
                                           ltab.data_ptr(), gs.data_ptr(), n, dm, d, g, tau, beta, ratio, gamma, dz.data_ptr(),
                                           tgt[0].data_ptr(), tgt[1].data_ptr(), tgt[2].data_ptr(), tgt[3].data_ptr(), int(direct),
                                           ws.data_ptr(), ws.numel(), core._stream()), 'lfq_backward')
        if direct:
            return dz, None, None, None, None, None, None
        grads = [t.view(p.shape) if ctx.needs_input_grad[i + 1] else None for i, (t, p) in enumerate(zip(tgt, ctx.params))]
        return (dz, *grads, None, None)


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations', '_f32c')]
