"""Spatially conditioned GroupNorm (MoVQ's spatially conditional normalisation, diffusers' ``SpatialNorm``) over the vqk C-ABI
(csrc/spnorm.hip): the autograd Function behind ``modules.autoencoder.SpatialNorm`` plus the staged torch formulation of the same
function, which serves what the kernels do not (and CPU tensors).  Private part of :mod:`ops` like ``_ops_attn.py`` (imported at
the end of ``ops.py``, which re-exports every name); shared infrastructure is reached through ``core``."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core

SPNORM_RATIOS = (1, 2, 4, 8, 16, 32)
SPNORM_MAX_CHANNELS = 512


def _sp_ratio(f, m) -> int:
    """H / h of a feature map f [N, C, H, W] over the tables' [N, C, h, w]; 0 when the shapes do not nest by one integer ratio"""
    (n, c, hh, ww), (n2, c2, h, w) = f.shape, m.shape
    if n != n2 or c != c2 or h < 1 or w < 1 or hh % h or ww % w or hh // h != ww // w:
        return 0
    return hh // h


def spnorm_fused_serves(f, m, groups: int = 32) -> bool:
    """the fused kernels serve this problem: GPU tensors, fp32 or bf16 feature map, 32 groups, C a multiple of 32 up to 512, a
    power-of-two ratio up to 32"""
    n, c = f.shape[0], f.shape[1]
    return (f.is_cuda and f.dtype in (torch.float32, torch.bfloat16) and int(groups) == 32 and c % 32 == 0
            and c <= SPNORM_MAX_CHANNELS and _sp_ratio(f, m) in SPNORM_RATIOS and 1 <= n <= 65535 and m.shape[2] * m.shape[3] < (1 << 24)
            and f.shape[2] * f.shape[3] < (1 << 31))


def _sp_check(f, m, a, gamma, beta, groups: int) -> int:
    if f.dim() != 4 or m.dim() != 4 or m.shape != a.shape:
        raise RuntimeError(f'vqk: spatial_norm wants f [N, C, H, W] and M, A of one [N, C, h, w] shape, got {tuple(f.shape)}, '
                           f'{tuple(m.shape)}, {tuple(a.shape)}')
    r = _sp_ratio(f, m)
    if r < 1:
        raise RuntimeError(f'vqk: spatial_norm: the map {tuple(f.shape)} is no integer multiple of the tables {tuple(m.shape)}')
    c = f.shape[1]
    if int(groups) < 1 or c % int(groups):
        raise ValueError(f'spatial_norm: {groups} groups do not divide the {c} channels')
    if gamma.numel() != c or beta.numel() != c:
        raise RuntimeError(f'vqk: spatial_norm: gamma / beta must hold {c} values, got {gamma.numel()} / {beta.numel()}')
    return r


def spatial_norm_staged(f, m, a, gamma, beta, groups: int = 32, eps: float = 1e-6, silu: bool = False):
    """the mathematics of :func:`spatial_norm` from torch operations in fp32 (the tables are upsampled to the map): serves every
    shape and CPU tensors, the A/B partner of the fused kernels.  Result in f's dtype."""
    r = _sp_check(f, m, a, gamma, beta, groups)
    n, c = f.shape[0], f.shape[1]
    x = f.to(torch.float32)
    xg = x.reshape(n, int(groups), -1)
    mean = xg.mean(dim=2, keepdim=True)
    var = xg.var(dim=2, keepdim=True)                           # unbiased: this project's GroupNorm
    xh = ((xg - mean) * torch.rsqrt(var + eps)).reshape(x.shape)
    u = xh * gamma.to(torch.float32).reshape(1, c, 1, 1) + beta.to(torch.float32).reshape(1, c, 1, 1)
    m, a = m.to(torch.float32), a.to(torch.float32)
    if r > 1:
        m = torch.nn.functional.interpolate(m, scale_factor=r, mode='nearest')
        a = torch.nn.functional.interpolate(a, scale_factor=r, mode='nearest')
    p = u * m + a
    if silu:
        p = torch.nn.functional.silu(p)
    return p.to(f.dtype).contiguous(memory_format=torch.channels_last)


def _sp_ws(dtype, n, h, w, r, c, device) -> torch.Tensor:
    nbytes = _native.lib().vqk_spnorm_ws_bytes(core.dcode(dtype), n, h, w, r, c)
    if nbytes < 0:
        _native.check(int(nbytes), 'spnorm_ws_bytes')
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)     # torch's allocator: legal under graph capture


def raw_spnorm_forward(f, m, a, gamma, beta, eps: float, silu: bool):
    """(out, stats) of the fused forward; f NHWC fp32 / bf16, m / a NHWC fp32, gamma / beta flat fp32"""
    n, c, hh, ww = f.shape
    h, w = m.shape[2], m.shape[3]
    r = hh // h
    out = torch.empty_like(f, memory_format=torch.channels_last)
    stats = torch.empty(n * 32 * 2, dtype=torch.float32, device=f.device)
    ws = _sp_ws(f.dtype, n, h, w, r, c, f.device)
    nb = f.numel() * f.element_size()
    st = core._timed('spatial_norm_fwd (HBM)', 0.0,
                     lambda: _native.lib().vqk_spnorm_forward(core.dcode(f.dtype), f.data_ptr(), m.data_ptr(), a.data_ptr(), gamma.data_ptr(),
                                                              beta.data_ptr(), out.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                                              n, h, w, r, c, 32, eps, int(silu), core._stream()),
                     3 * nb + 2 * m.numel() * 4, launches=3)
    _native.check(st, 'spnorm_forward')
    return out, stats


def raw_spnorm_backward(f, stats, m, a, gamma, beta, dy, silu: bool, dgamma=None, dbeta=None):
    """(df, dM, dA, dgamma, dbeta); ``dgamma`` / ``dbeta``: fp32 [C] targets the sums are ADDED onto (fresh zeros when None)"""
    n, c, hh, ww = f.shape
    h, w = m.shape[2], m.shape[3]
    r = hh // h
    df = torch.empty_like(f, memory_format=torch.channels_last)
    dm = torch.empty_like(m, memory_format=torch.channels_last)
    da = torch.empty_like(m, memory_format=torch.channels_last)
    dgamma = dgamma if dgamma is not None else torch.zeros(c, dtype=torch.float32, device=f.device)
    dbeta = dbeta if dbeta is not None else torch.zeros(c, dtype=torch.float32, device=f.device)
    ws = _sp_ws(f.dtype, n, h, w, r, c, f.device)
    nb = f.numel() * f.element_size()
    st = core._timed('spatial_norm_bwd (HBM)', 0.0,
                     lambda: _native.lib().vqk_spnorm_backward(core.dcode(f.dtype), f.data_ptr(), stats.data_ptr(), m.data_ptr(), a.data_ptr(),
                                                               gamma.data_ptr(), beta.data_ptr(), dy.data_ptr(), df.data_ptr(), dm.data_ptr(),
                                                               da.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel(),
                                                               n, h, w, r, c, 32, int(silu), core._stream()),
                     5 * nb + 6 * m.numel() * 4, launches=4)
    _native.check(st, 'spnorm_backward')
    return df, dm, da, dgamma, dbeta


class SpatialNormFn(torch.autograd.Function):
    """out = [silu]((GroupNorm_32(f) * gamma + beta) * M_up + A_up) on the fused kernels.  Forward: statistics (per-block partials,
    added in block order) + one apply pass; backward: two sweeps over (f, dy) with the pre-activation recomputed.  No atomics: the
    same bits on every run in every mode.  No host synchronisation, nothing but ``torch.empty`` / ``torch.zeros`` between the
    launches: captures into a graph."""

    @staticmethod
    def forward(ctx, f, m, a, gamma, beta, eps, silu):
        core._require_gpu(f)
        f = core.nhwc(f)
        m = core.nhwc(m.detach())
        a = core.nhwc(a.detach())
        g = core.f32c(gamma).reshape(-1)
        b = core.f32c(beta).reshape(-1)
        out, stats = raw_spnorm_forward(f, m, a, g, b, float(eps), bool(silu))
        ctx.save_for_backward(f, stats, m, a, g, b)
        ctx.params = (gamma, beta)
        ctx.cfg = (bool(silu), gamma.shape, beta.shape)
        return out

    @staticmethod
    def backward(ctx, dy):
        f, stats, m, a, g, b = ctx.saved_tensors
        silu, gshape, bshape = ctx.cfg
        dy = core.nhwc(dy if dy.dtype == f.dtype else dy.to(f.dtype))
        tg, tb = core.direct_grad(ctx.params[0]), core.direct_grad(ctx.params[1])
        direct = tg is not None and tb is not None
        df, dm, da, dgamma, dbeta = raw_spnorm_backward(f, stats, m, a, g, b, dy, silu, tg.view(-1) if direct else None,
                                                        tb.view(-1) if direct else None)
        if direct:
            return df, dm, da, None, None, None, None
        return df, dm, da, dgamma.view(gshape), dbeta.view(bshape), None, None


def spatial_norm(f, M, A, gamma, beta, groups: int = 32, eps: float = 1e-6, silu: bool = False):
    """act((GroupNorm(f) * gamma + beta) * M[:, :, i // r, j // r] + A[:, :, i // r, j // r]), act = identity or SiLU: f [N, C, H, W]
    (NHWC storage, fp32 or bf16), M / A [N, C, h, w] fp32 modulation tables at the latent resolution (H = r h, W = r w), gamma / beta
    the GroupNorm affine (C values, any shape).  This project's GroupNorm: per (sample, group) mean and unbiased variance.  Fused HIP
    kernels inside their served domain (``spnorm_fused_serves``) when ``ops.SPNORM_FUSED`` is on, the staged form otherwise."""
    _sp_check(f, M, A, gamma, beta, groups)
    if not (core.SPNORM_FUSED and spnorm_fused_serves(f, M, groups)):
        return spatial_norm_staged(f, M, A, gamma, beta, groups, eps, silu)
    # (the kernels read fp32 tables: a cast, if any, is autograd's to differentiate)
    return SpatialNormFn.apply(f, M.to(torch.float32), A.to(torch.float32), gamma, beta, eps, silu)


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations')]
