"""Operators of the projection quantizers over the vqk C-ABI -- finite scalar (csrc/fsq.hip), lookup-free (csrc/lfq.hip) and binary
spherical (csrc/bsq.hip), one kernel core (csrc/proj_quant.h, csrc/sign_quant.h) and one host frame: the autograd Functions behind ``FSQuantizer`` /
``LFQuantizer`` / ``BSQuantizer`` plus the assignment-only and decode launchers.  Private part of :mod:`ops` like ``_ops_vq.py`` (imported at the end of ``ops.py``, which re-exports every name);
shared infrastructure is reached through ``core``."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _native
from . import ops as core

LFQ_MAX_BITS = 18
LFQ_MAX_GROUP_BITS = 10
_FSQ_WS: dict = {}                  # _wkey() -> slab workspace of vqk_fsq_backward: plain stores + ordered sums, no atomics
_LFQ_WS: dict = {}                  # _wkey() -> slab workspace of vqk_lfq_forward / vqk_lfq_backward
BSQ_MAX_BITS = 18
BSQ_MAX_GROUP_BITS = 10
_BSQ_WS: dict = {}                  # _wkey() -> slab workspace of vqk_bsq_forward / vqk_bsq_backward


def _levels_arg(levels):
    """the levels as the host int array the launchers pass by value, and K = prod(levels)"""
    levels = [int(v) for v in levels]
    if not 1 <= len(levels) <= 8:
        raise ValueError('fsq: between 1 and 8 levels')
    return (ctypes.c_int32 * 8)(*levels), len(levels), math.prod(levels)


# the sign quantizers (csrc/sign_quant.h), by kind: (max bits, max group bits, workspace dict, has the per-row buffer r = 1 / |v|)
_SIGN = {'lfq': (LFQ_MAX_BITS, LFQ_MAX_GROUP_BITS, _LFQ_WS, False), 'bsq': (BSQ_MAX_BITS, BSQ_MAX_GROUP_BITS, _BSQ_WS, True)}


def _sign_bits(kind: str, bits: int) -> int:
    bits = int(bits)
    if not 1 <= bits <= _SIGN[kind][0]:
        raise ValueError(f'{kind}: bits must be between 1 and {_SIGN[kind][0]}, got {bits}')
    return bits


# ---- the frame the quantizers share; ``kind`` / ``unit`` ('fsq', 'levels' | 'lfq', 'bits' | 'bsq', 'bits') only word the messages ----

def _proj_dm(kind: str, unit: str, w_in, w_out, d: int) -> int:
    """D of the [d, D] / [D, d] memory of the two 1x1 projections (Conv2d weights [O, I, 1, 1], or plain matrices)"""
    dm = w_in.numel() // d
    if w_in.numel() != d * dm or w_out.numel() != d * dm or w_in.shape[0] != d or w_out.shape[0] != dm:
        raise RuntimeError(f'vqk: {kind} projections {tuple(w_in.shape)} / {tuple(w_out.shape)} do not match {d} {unit}')
    return dm


def _q_ptrs(q: torch.Tensor):
    """the (fp32 q, bf16 q) pointer pair of the C-ABI: the kernels write the one that is set"""
    return (0, q.data_ptr()) if q.dtype == torch.bfloat16 else (q.data_ptr(), 0)


def _assign_args(flat_z, w_in, b_in):
    """flat_z [N, D], the input projection -> (z, W_in, b_in as fp32 memory, idx [N] int64 to fill)"""
    flat_z = core.f32c(flat_z)
    return flat_z, core.f32c(w_in), core.f32c(b_in), torch.empty(flat_z.shape[0], dtype=torch.int64, device=flat_z.device)


def _decode(idx, w_out, b_out, d: int, out_dtype, launch, what: str) -> torch.Tensor:
    """idx [...] int64 -> q [..., D] in ``out_dtype``; ``launch((idx, W_out, b_out, n, D), q, q_lo)`` is the quantizer's C-ABI call"""
    dm = w_out.numel() // d
    flat = idx.reshape(-1).to(torch.int64).contiguous()
    q = torch.empty((flat.numel(), dm), dtype=out_dtype, device=idx.device)
    wo, bo = core.f32c(w_out), core.f32c(b_out)
    _native.check(launch((flat.data_ptr(), wo.data_ptr(), bo.data_ptr(), flat.numel(), dm), *_q_ptrs(q)), what)
    return q.view(*idx.shape, dm)


def _forward_buffers(kind: str, unit: str, z, params, d: int, out_dtype):
    """-> z (NHWC fp32), flat [N, D] (a view: NHWC memory is already [N][D]), the four projection tensors as fp32 memory, and the
    buffers every forward fills: q [B,D,H,W] in ``out_dtype``, idx [N] int64, u [N, d] fp32"""
    z = core.nhwc(z.to(torch.float32))
    b, dm, h, w = z.shape
    n = b * h * w
    w_in, w_out = params[0], params[2]
    if _proj_dm(kind, unit, w_in, w_out, d) != dm:
        raise RuntimeError(f'vqk: {kind} projections are for {w_in.numel() // d} channels, the latent map has {dm}')
    mem = tuple(core.f32c(p) for p in params)
    flat = z.permute(0, 2, 3, 1).reshape(n, dm)
    q = core.empty_nhwc(b, dm, h, w, torch.bfloat16 if out_dtype == torch.bfloat16 else torch.float32, z.device)
    idx = torch.empty(n, dtype=torch.int64, device=z.device)
    u = torch.empty((n, d), dtype=torch.float32, device=z.device)
    return z, flat, mem, q, idx, u


def _cotangent(dq, z):
    """dq as the kernels read it: NHWC, fp32 or bf16 (zeros when q went unused)"""
    dqc = core.nhwc(dq) if dq is not None else torch.zeros_like(z, memory_format=core._CL)
    return dqc if dqc.dtype in (torch.float32, torch.bfloat16) else dqc.to(torch.float32)


def _grad_targets(params):
    """where the backward adds / stores the four parameter gradients: straight in the optimizer's arena when every one of the four has
    a place there (direct: the kernel ACCUMULATES), fresh fp32 buffers otherwise"""
    tgt = [core.direct_grad(p) if p.is_contiguous() else None for p in params]
    direct = all(t is not None for t in tgt)
    if not direct:
        tgt = [torch.empty_like(p, dtype=torch.float32, memory_format=torch.contiguous_format) for p in params]
    return tgt, direct


def _grads(ctx, dz, tgt, direct: bool):
    """what ``backward`` returns for (z, w_in, b_in, w_out, b_out, cfg, out_dtype)"""
    if direct:
        return dz, None, None, None, None, None, None
    grads = [t.view(p.shape) if ctx.needs_input_grad[i + 1] else None for i, (t, p) in enumerate(zip(tgt, ctx.params))]
    return (dz, *grads, None, None)


# ---- finite scalar quantizer ----

def fsq_assign(flat_z: torch.Tensor, w_in: torch.Tensor, b_in: torch.Tensor, levels) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N] int64: the forward kernel without q and u"""
    core._require_gpu(flat_z)
    lv, d, _ = _levels_arg(levels)
    z, wi, bi, idx = _assign_args(flat_z, w_in, b_in)
    _native.check(_native.lib().vqk_fsq_forward(z.data_ptr(), wi.data_ptr(), bi.data_ptr(), 0, 0, z.shape[0], z.shape[1], d, lv,
                                                idx.data_ptr(), 0, 0, 0, 0, core._stream()), 'fsq_forward (assign)')
    return idx


def fsq_decode(idx: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, levels, out_dtype=torch.float32) -> torch.Tensor:
    """idx [...] int64 -> q [..., D] in ``out_dtype``: the bits the forward writes for the same index"""
    core._require_gpu(idx)
    lv, d, _ = _levels_arg(levels)
    return _decode(idx, w_out, b_out, d, out_dtype,
                   lambda head, q, q_lo: _native.lib().vqk_fsq_decode(*head, d, lv, q, q_lo, core._stream()), 'fsq_decode')


class FSQFn(torch.autograd.Function):
    """Finite scalar quantization with the straight-through gradient: project to len(levels) channels, tanh-bound, round,
    project back.  One forward kernel; the backward is one kernel + the ordered slab sum (bitwise reproducible in every mode).
    Returns (q [B,D,H,W] in out_dtype, idx [B, H*W] int64, loss 0-dim fp32 zero, hist int32 [K])."""

    @staticmethod
    def forward(ctx, z, w_in, b_in, w_out, b_out, levels, out_dtype):
        core._require_gpu(z)
        lv, d, k = _levels_arg(levels)
        ctx.params = (w_in, b_in, w_out, b_out)
        z, flat, (wi, bi, wo, bo), q, idx, u = _forward_buffers('fsq', 'levels', z, ctx.params, d, out_dtype)
        n, dm = flat.shape
        zbuf = torch.zeros(k + 1, dtype=torch.int32, device=z.device)            # histogram | the zero loss: one fill launch
        hist, loss = zbuf[:k], zbuf[k:].view(torch.float32).view(())
        _native.check(_native.lib().vqk_fsq_forward(flat.data_ptr(), wi.data_ptr(), bi.data_ptr(), wo.data_ptr(), bo.data_ptr(), n, dm,
                                                    d, lv, idx.data_ptr(), u.data_ptr(), *_q_ptrs(q), hist.data_ptr(), core._stream()),
                      'fsq_forward')
        ctx.save_for_backward(z, u, wi, wo)
        ctx.cfg = (tuple(int(v) for v in levels), n, dm, d)
        ctx.mark_non_differentiable(idx, loss, hist)
        return q, idx.view(z.shape[0], z.shape[2] * z.shape[3]), loss, hist

    @staticmethod
    def backward(ctx, dq, _didx, _dloss, _dhist):
        z, u, wi, wo = ctx.saved_tensors
        levels, n, dm, d = ctx.cfg
        lv = _levels_arg(levels)[0]
        dqc = _cotangent(dq, z)
        dz = torch.empty_like(z, memory_format=core._CL)
        tgt, direct = _grad_targets(ctx.params)
        lib = _native.lib()
        ws = core.grow_ws(_FSQ_WS, z.device, lib.vqk_fsq_backward_ws_bytes(n, dm, d))
        _native.check(lib.vqk_fsq_backward(z.data_ptr(), u.data_ptr(), dqc.data_ptr(), core.dcode(dqc.dtype), wi.data_ptr(), wo.data_ptr(),
                                           n, dm, d, lv, dz.data_ptr(), *(t.data_ptr() for t in tgt), int(direct), ws.data_ptr(),
                                           ws.numel(), core._stream()), 'fsq_backward')
        return _grads(ctx, dz, tgt, direct)


# ---- the sign quantizers, lookup-free (lfq) and binary spherical (bsq): one frame; ``kind`` names the C functions vqk_<kind>_* ----

def _sign_fn(kind: str, name: str):
    return getattr(_native.lib(), f'vqk_{kind}_{name}')


def _sign_assign(kind: str, flat_z, w_in, b_in, bits: int) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N] int64: the forward kernel without q, u, r, loss and workspace"""
    core._require_gpu(flat_z)
    d = _sign_bits(kind, bits)
    z, wi, bi, idx = _assign_args(flat_z, w_in, b_in)
    no_r = (0,) if _SIGN[kind][3] else ()
    _native.check(_sign_fn(kind, 'forward')(z.data_ptr(), wi.data_ptr(), bi.data_ptr(), 0, 0, z.shape[0], z.shape[1], d, 1, 1.0, 0.0, 0.0,
                                            0.0, idx.data_ptr(), 0, *no_r, 0, 0, 0, 0, 0, 0, 0, core._stream()), f'{kind}_forward (assign)')
    return idx


def _sign_decode(kind: str, idx, w_out, b_out, bits: int, out_dtype) -> torch.Tensor:
    """idx [...] int64 -> q [..., D] in ``out_dtype``: the bits the forward writes for the same index"""
    core._require_gpu(idx)
    d = _sign_bits(kind, bits)
    fn = _sign_fn(kind, 'decode')
    return _decode(idx, w_out, b_out, d, out_dtype, lambda head, q, q_lo: fn(*head, d, q, q_lo, core._stream()), f'{kind}_decode')


def _sign_forward(kind: str, ctx, z, w_in, b_in, w_out, b_out, cfg, out_dtype):
    core._require_gpu(z)
    _, max_group, ws_of, has_r = _SIGN[kind]
    d, g, beta, ratio, gamma, tau = int(cfg[0]), int(cfg[1]), float(cfg[2]), float(cfg[3]), float(cfg[4]), float(cfg[5])
    d = _sign_bits(kind, d)
    if not 1 <= g <= max_group:
        raise ValueError(f'{kind}: ent_group_bits must be between 1 and {max_group}, got {g}')
    ctx.params = (w_in, b_in, w_out, b_out)
    z, flat, (wi, bi, wo, bo), q, idx, u = _forward_buffers(kind, 'bits', z, ctx.params, d, out_dtype)
    n, dm = flat.shape
    r = (torch.empty(n, dtype=torch.float32, device=z.device),) if has_r else ()
    hist = torch.zeros(1 << d, dtype=torch.int32, device=z.device)
    out = torch.empty(4, dtype=torch.float32, device=z.device)
    ltab = torch.empty(((d + g - 1) // g) << g, dtype=torch.float32, device=z.device)
    nbytes = _sign_fn(kind, 'ws_bytes')(n, dm, d, g)
    if nbytes < 0:
        _native.check(int(nbytes), f'{kind}_ws_bytes')
    ws = core.grow_ws(ws_of, z.device, max(nbytes, 16))
    _native.check(_sign_fn(kind, 'forward')(flat.data_ptr(), wi.data_ptr(), bi.data_ptr(), wo.data_ptr(), bo.data_ptr(), n, dm, d, g, tau,
                                            beta, ratio, gamma, idx.data_ptr(), u.data_ptr(), *(t.data_ptr() for t in r), *_q_ptrs(q),
                                            hist.data_ptr(), out.data_ptr(), ltab.data_ptr(), ws.data_ptr(), ws.numel(), core._stream()),
                  f'{kind}_forward')
    ctx.save_for_backward(z, u, *r, wi, wo, ltab)
    ctx.cfg = (n, dm, d, g, beta, ratio, gamma, tau)
    loss, parts = out[0], out[1:]
    ctx.mark_non_differentiable(idx, hist, parts)
    return q, idx.view(z.shape[0], z.shape[2] * z.shape[3]), loss, hist, parts


def _sign_backward(kind: str, ctx, dq, dloss):
    z, u, *r, wi, wo, ltab = ctx.saved_tensors
    n, dm, d, g, beta, ratio, gamma, tau = ctx.cfg
    dqc = _cotangent(dq, z)
    # the loss cotangent stays on the device (a captured graph follows it); an unused loss contributes nothing
    gs = dloss.to(torch.float32).contiguous() if dloss is not None else torch.zeros((), dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z, memory_format=core._CL)
    tgt, direct = _grad_targets(ctx.params)
    ws = core.grow_ws(_SIGN[kind][2], z.device, max(_sign_fn(kind, 'ws_bytes')(n, dm, d, g), 16))
    _native.check(_sign_fn(kind, 'backward')(z.data_ptr(), u.data_ptr(), *(t.data_ptr() for t in r), dqc.data_ptr(), core.dcode(dqc.dtype),
                                             wi.data_ptr(), wo.data_ptr(), ltab.data_ptr(), gs.data_ptr(), n, dm, d, g, tau, beta, ratio,
                                             gamma, dz.data_ptr(), *(t.data_ptr() for t in tgt), int(direct), ws.data_ptr(), ws.numel(),
                                             core._stream()), f'{kind}_backward')
    return _grads(ctx, dz, tgt, direct)


def lfq_assign(flat_z: torch.Tensor, w_in: torch.Tensor, b_in: torch.Tensor, bits: int) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N] int64: the forward kernel without q, u, loss and workspace"""
    return _sign_assign('lfq', flat_z, w_in, b_in, bits)


def lfq_decode(idx: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, bits: int, out_dtype=torch.float32) -> torch.Tensor:
    """idx [...] int64 -> q [..., D] in ``out_dtype``: the bits the forward writes for the same index"""
    return _sign_decode('lfq', idx, w_out, b_out, bits, out_dtype)


class LFQFn(torch.autograd.Function):
    """Lookup-free quantization (MAGVIT-v2): project to ``bits`` channels, take the sign, project back; straight-through gradient at
    the projected latent plus the true gradient of loss = beta commit + ratio (H_sample - gamma H_batch).  Forward: one kernel + the
    ordered finish; backward: one kernel + the ordered slab sum (bitwise reproducible in every mode).  ``cfg`` = (bits, group_bits,
    beta, ratio, gamma, tau).  Returns (q [B,D,H,W] in out_dtype, idx [B, H*W] int64, loss 0-dim fp32 differentiable, hist int32 [K],
    parts fp32 [3] = commit, H_sample, H_batch)."""

    @staticmethod
    def forward(ctx, z, w_in, b_in, w_out, b_out, cfg, out_dtype):
        return _sign_forward('lfq', ctx, z, w_in, b_in, w_out, b_out, cfg, out_dtype)

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist, _dparts):
        return _sign_backward('lfq', ctx, dq, dloss)


def bsq_assign(flat_z: torch.Tensor, w_in: torch.Tensor, b_in: torch.Tensor, bits: int) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N] int64: the forward kernel without q, u, r, loss and workspace"""
    return _sign_assign('bsq', flat_z, w_in, b_in, bits)


def bsq_decode(idx: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, bits: int, out_dtype=torch.float32) -> torch.Tensor:
    """idx [...] int64 -> q [..., D] in ``out_dtype``: the bits the forward writes for the same index"""
    return _sign_decode('bsq', idx, w_out, b_out, bits, out_dtype)


class BSQFn(torch.autograd.Function):
    """Binary spherical quantization (BSQ-ViT): project to ``bits`` channels, normalise to the unit sphere, take the sign (the corner
    +-1 / sqrt(bits)), project back; straight-through gradient at the normalised latent u, carried through the normalisation, plus the
    true gradient of loss = beta commit + ratio (H_sample - gamma H_batch).  Forward: one kernel + the ordered finish; backward: one
    kernel + the ordered slab sum (bitwise reproducible in every mode).  ``cfg`` = (bits, group_bits, beta, ratio, gamma, tau).  Returns
    (q [B,D,H,W] in out_dtype, idx [B, H*W] int64, loss 0-dim fp32 differentiable, hist int32 [K], parts fp32 [3] = commit, H_sample,
    H_batch)."""

    @staticmethod
    def forward(ctx, z, w_in, b_in, w_out, b_out, cfg, out_dtype):
        return _sign_forward('bsq', ctx, z, w_in, b_in, w_out, b_out, cfg, out_dtype)

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist, _dparts):
        return _sign_backward('bsq', ctx, dq, dloss)


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations', 'ctypes', 'math')]
