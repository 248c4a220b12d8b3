"""Self-attention operators over the vqk C-ABI (csrc/attn.hip): the autograd Function behind ``AttnBlock`` plus the staged torch
formulation that serves the head dims the kernels do not.  Private part of :mod:`ops` like ``_ops_cos.py`` (imported at the end of
``ops.py``, which re-exports every name); shared infrastructure is reached through ``core``."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core

ATTN_FUSED_DIMS = (64, 128, 256, 512)


def attn_fused_serves(dtype, heads: int, d: int) -> bool:
    """the fused kernels serve this problem (fp32 or bf16 storage, head dim in ATTN_FUSED_DIMS; any N, any number of heads)"""
    return dtype in (torch.float32, torch.bfloat16) and int(heads) >= 1 and int(d) in ATTN_FUSED_DIMS


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[B, N, C] with unit channel stride, one row stride for the whole tensor (a multiple of 16 bytes) and a 16-byte aligned start:
    what the kernels read in place -- a channel slice of a [B, N, 3C] tensor passes as it is, anything else is copied"""
    b, n, c = t.shape
    es = t.element_size()
    ld = t.stride(1)
    ok = (t.stride(2) == 1 and ld >= c and (ld * es) % 16 == 0 and (b == 1 or t.stride(0) == n * ld) and t.data_ptr() % 16 == 0)
    if n == 1 and t.stride(2) == 1 and not ok:          # a single row: its stride is free
        ok = t.data_ptr() % 16 == 0 and (b == 1 or (t.stride(0) >= c and (t.stride(0) * es) % 16 == 0))
    return t if ok else t.contiguous()


def _ld(t: torch.Tensor) -> int:
    b, n, _ = t.shape
    if n == 1:
        return t.stride(0) if b > 1 else t.shape[2]
    return t.stride(1)


class AttentionFn(torch.autograd.Function):
    """o = softmax(scale q k^T) v per (batch, head) on [B, N, heads * d] rows (fp32 or bf16).  Forward: one kernel (online softmax,
    lse saved); backward: delta + the key-owning dK / dV pass + the query-owning dQ pass, no atomics: the same bits on every run in
    every mode.  No host synchronisation, nothing but ``torch.empty`` between the launches: captures into a graph."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale):
        core._require_gpu(q)
        b, n, c = q.shape
        d = c // heads
        q, k, v = _rows(q), _rows(k), _rows(v)
        o = torch.empty((b, n, c), dtype=q.dtype, device=q.device)
        lse = torch.empty((b, heads, n), dtype=torch.float32, device=q.device)
        _native.check(_native.lib().vqk_attn_fwd(core.dcode(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                                                 b, n, heads, d, _ld(q), _ld(k), _ld(v), c, scale, core._stream()), 'attn_fwd')
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.cfg = (heads, d, scale)
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    def backward(ctx, do, _dlse):
        q, k, v, o, lse = ctx.saved_tensors
        heads, d, scale = ctx.cfg
        b, n, c = q.shape
        do = _rows(do if do.dtype == q.dtype else do.to(q.dtype))
        dq, dk, dv = (torch.empty((b, n, c), dtype=q.dtype, device=q.device) for _ in range(3))
        delta = torch.empty((b, heads, n), dtype=torch.float32, device=q.device)
        _native.check(_native.lib().vqk_attn_bwd(core.dcode(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                                                 do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), b, n, heads,
                                                 d, _ld(q), _ld(k), _ld(v), c, _ld(do), c, c, c, scale, core._stream()), 'attn_bwd')
        return dq, dk, dv, None, None


def _check(q, k, v, heads):
    core._require_gpu(q)
    core._require_gpu(k)
    core._require_gpu(v)
    if q.dim() not in (3, 4) or q.shape != k.shape or q.shape != v.shape:
        raise RuntimeError(f'vqk: attention wants q, k, v of one [B, N, C] or [B, C, H, W] shape, got {tuple(q.shape)}, {tuple(k.shape)}, '
                           f'{tuple(v.shape)}')
    if not (q.dtype == k.dtype == v.dtype) or q.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f'vqk: attention wants q, k, v of one dtype (fp32 or bf16), got {q.dtype}, {k.dtype}, {v.dtype}')
    c = q.shape[1] if q.dim() == 4 else q.shape[2]
    heads = int(heads)
    if heads < 1 or c % heads:
        raise ValueError(f'attention: heads ({heads}) must divide the channel count ({c})')
    return heads, c // heads


def _to_rows(t):
    """NHWC storage of a [B, C, H, W] tensor IS its [B, H*W, C] row matrix: a view, no layout pass"""
    if t.dim() == 3:
        return t
    b, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(b, h * w, c)


def _from_rows(o, like):
    if like.dim() == 3:
        return o
    b, c, h, w = like.shape
    return o.view(b, h, w, c).permute(0, 3, 1, 2)


def _staged_rows(q, k, v, heads: int, scale: float):
    b, n, c = q.shape
    d = c // heads
    qh, kh, vh = (t.reshape(b, n, heads, d).permute(0, 2, 1, 3).to(torch.float32) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale          # fp32 logits and statistics in every storage type
    p = torch.softmax(s, dim=-1)
    if q.dtype != torch.float32:
        # P enters the second product rounded to the storage type, as in the kernels; the rounding carries no gradient of its own
        # (a plain cast would round dP on the way back as well)
        p = p + (p.to(q.dtype).to(torch.float32) - p).detach()
    o = torch.matmul(p, vh).to(q.dtype)
    return o.permute(0, 2, 1, 3).reshape(b, n, c)


def attention_staged(q, k, v, heads: int = 1, scale=None):
    """the mathematics of :func:`attention` from torch matmul / softmax with fp32 logits and statistics (the B x heads x N x N matrix
    is materialised): serves every head dim, the A/B partner of the fused kernels"""
    heads, d = _check(q, k, v, heads)
    scale = float(d) ** -0.5 if scale is None else float(scale)
    return _from_rows(_staged_rows(_to_rows(q), _to_rows(k), _to_rows(v), heads, scale), q)


def attention(q, k, v, heads: int = 1, scale=None):
    """softmax(scale q k^T) v per (batch, head); q, k, v [B, N, C] rows or [B, C, H, W] maps in NHWC storage, C = heads * d, fp32 or
    bf16; scale defaults to d ** -0.5.  Fused HIP kernels for d in ATTN_FUSED_DIMS (``ops.ATTN_FUSED``), the staged form otherwise."""
    heads, d = _check(q, k, v, heads)
    scale = float(d) ** -0.5 if scale is None else float(scale)
    if not (core.ATTN_FUSED and attn_fused_serves(q.dtype, heads, d)):
        return attention_staged(q, k, v, heads, scale)
    o, _ = AttentionFn.apply(_to_rows(q), _to_rows(k), _to_rows(v), heads, scale)
    return _from_rows(o, q)


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations')]
