"""Index-backpropagation (IBQ) operators over the vqk C-ABI (csrc/ibq.hip): the autograd Function behind ``IBQuantizer``, the
argmax-only call and the STAGED formulation of the same definition with N x K tensors in memory.  Private part of :mod:`ops` like
``_ops_simvq.py`` (imported at the end of ``ops.py``, which re-exports every name); shared infrastructure is reached through ``core``.

Definition (include/vqk.h, "IBQ quantizer"): S = (z E^T) / T, P = softmax(S), idx = argmax S (the smallest index wins a tie),
q = E[idx]; loss = (2 + beta) / (N D) sum |q - z|^2, the value of mean((Ind E - z)^2) + mean((sg[q] - z)^2) + beta mean((q - sg[z])^2)
with Ind = hard - sg[P] + P.  There is no straight-through copy onto z: with G = g + s c2 (q - z), c2 = 2 / (N D),
dS = P (G E^T - rowsum(G ebar)), dz = -2 s c2 (q - z) + dS E / T and dE = scatter_idx(G + s beta c2 (q - z)) + dS^T z / T -- every
code receives gradient on every step."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core
from ._ops_vq import hist_sse, lookup_backward_frame, nhwc_rows, rows_image

IBQ_FUSED_DIMS = (64, 128, 256)
# the backward of shapes with N K at or below this runs the staged torch operations on the fused forward's lse / ebar: measured at
# N = 8192, K = 1024 (N K = 2^23, 32 MiB per N x K tensor) the code-owning pass has 16 workgroups to fill the device with and the three
# launches take 2.83 ms against 0.35 ms staged (profiles/ibq_bench.txt).  Beyond it the fused launches stay for memory.
IBQ_STAGED_BWD_MAX_NK = 1 << 23
_IBQ_FWD_WS: dict = {}              # _wkey() -> the forward's per-block sse slots (core.grow_ws)
_IBQ_BWD_WS: dict = {}              # _wkey() -> G, H and delta of the backward's row pass (core.grow_ws)


def _check_ibq(codebook, temperature: float) -> tuple:
    if codebook.dim() != 2:
        raise ValueError(f'ibq: the codebook must be [K, D], got {tuple(codebook.shape)}')
    t = float(temperature)
    if not (t > 0.0 and t < float('inf')):
        raise ValueError(f'ibq: the temperature must be a positive finite number, got {temperature!r}')
    return codebook.shape[0], codebook.shape[1], 1.0 / t


def ibq_fused_serves(codebook) -> bool:
    """the fused HIP forward and the three-launch backward serve this codebook (D in {64, 128, 256}, any K >= 1 below 2^31, fp32,
    contiguous, on the GPU) and are switched on; every other shape goes through :func:`ibq_staged` and the torch backward.  Of the
    served shapes the small ones (N K <= IBQ_STAGED_BWD_MAX_NK) take the torch backward as well, on the fused forward's statistics."""
    k, d = codebook.shape
    return bool(core.IBQ_FUSED and d in IBQ_FUSED_DIMS and 1 <= k < (1 << 31) and codebook.dtype == torch.float32
                and codebook.is_contiguous() and codebook.is_cuda)


def _ibq_forward(flat_z, e, inv_t: float, soft: bool, want_q32: bool, want_lo: bool, want_stats: bool):
    """vqk_ibq_forward_f32 on rows flat_z [N, D] and e [K, D]: (idx [N] int64, q fp32 or None, q bf16 or None, sse [1] or None,
    hist [K] or None, lse [N] or None, ebar [N, D] or None); ``soft`` False is the argmax-only mode"""
    n, d = flat_z.shape
    k = e.shape[0]
    dev = flat_z.device
    lib = _native.lib()
    sse = hist = ws = lse = ebar = None
    if want_stats:
        hist, sse = hist_sse(k, dev)
        ws = core.grow_ws(_IBQ_FWD_WS, dev, lib.vqk_ibq_forward_ws_bytes(n))
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    if soft:
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        ebar = torch.empty((n, d), dtype=torch.float32, device=dev)
    q32 = torch.empty((n, d), dtype=torch.float32, device=dev) if want_q32 else None
    qlo = torch.empty((n, d), dtype=torch.bfloat16, device=dev) if want_lo else None
    _native.check(lib.vqk_ibq_forward_f32(flat_z.data_ptr(), e.data_ptr(), n, k, d, inv_t, idx.data_ptr(), core._p(lse), core._p(ebar),
                                          core._p(q32), core._p(qlo), core._p(sse), core._p(hist), core._p(ws),
                                          ws.numel() * ws.element_size() if ws is not None else 0, core._stream()), 'ibq_forward')
    return idx, q32, qlo, sse, hist, lse, ebar


def ibq_staged(flat_z: torch.Tensor, codebook: torch.Tensor, temperature: float = 1.0, want_lo: bool = False):
    """The definition as fp32 torch operations with the N x K logits and probabilities in memory: the route of the shapes the fused
    kernels do not serve and the yardstick of tools/ibq_bench.py.  flat_z [N, D] fp32 -> (idx [N] int64, q [N, D] fp32, q as bf16 or
    None, sse [1], hist [K] int32, lse [N], ebar [N, D])."""
    core._require_gpu(flat_z)
    k, d, inv_t = _check_ibq(codebook, temperature)
    if flat_z.dim() != 2 or flat_z.shape[1] != d:
        raise ValueError(f'ibq: latents must be [N, {d}], got {tuple(flat_z.shape)}')
    e = core.f32c(codebook)
    s = (flat_z @ e.t()) * inv_t
    idx = s.argmax(dim=1)
    lse = torch.logsumexp(s, dim=1)
    ebar = torch.exp(s - lse[:, None]) @ e
    q32 = e[idx]
    sse = (q32 - flat_z).square().sum().view(1)
    hist = torch.bincount(idx, minlength=k).to(torch.int32)
    return idx, q32, (q32.to(torch.bfloat16) if want_lo else None), sse, hist, lse, ebar


def ibq_assign(flat_z: torch.Tensor, codebook: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """flat_z [N, D] fp32 -> idx [N] int64: the argmax-only call (no exponentials, no second product; the training forward's tokens
    bit for bit on the shapes the fused kernels serve)"""
    core._require_gpu(flat_z)
    k, d, inv_t = _check_ibq(codebook, temperature)
    if flat_z.dim() != 2 or flat_z.shape[1] != d:
        raise ValueError(f'ibq: latents must be [N, {d}], got {tuple(flat_z.shape)}')
    flat_z, e = core.f32c(flat_z), core.f32c(codebook.detach())
    if ibq_fused_serves(e):
        return _ibq_forward(flat_z, e, inv_t, False, False, False, False)[0]
    return ((flat_z @ e.t()) * inv_t).argmax(dim=1)


def ibq_backward_staged(flat_z, e, idx, lse, ebar, dq_rows, inv_t: float, cz_s, ce_s, want_de: bool = True):
    """the closed-form backward as fp32 torch operations with N x K tensors in memory: (dz rows [N, D], dE [K, D] or None) with
    cz_s = s beta c2 and ce_s = s c2 as 0-dim tensors or floats; a token outside [0, K) has no hard terms"""
    k, d = e.shape
    ok = (idx >= 0) & (idx < k)
    diff = torch.where(ok[:, None], e[idx.clamp(0, k - 1)] - flat_z, torch.zeros_like(flat_z))
    g = diff * ce_s
    if dq_rows is not None:
        g = g + dq_rows.float()
    p = torch.exp((flat_z @ e.t()) * inv_t - lse[:, None])
    ds = p * (g @ e.t() - (g * ebar).sum(1, keepdim=True))
    dz = diff * (-2.0 * ce_s) + (ds @ e) * inv_t
    de = None
    if want_de:
        # the hard term as a product with the 0 / 1 selection matrix (one more N x K tensor): no float atomics, unlike index_add_
        sel = (idx[:, None] == torch.arange(k, device=e.device)[None, :]).to(torch.float32)
        de = sel.t() @ (g + diff * cz_s) + (ds.t() @ flat_z) * inv_t
    return dz, de


def ibq_backward_rows(z_rows, e, idx, lse, ebar, dq_rows, inv_t: float, cz: float, ce: float, gs, dz_rows, de) -> None:
    """vqk_ibq_backward_f32 on row views: dz_rows [N, D] is written, de [K, D] (or None) accumulated as old + sum"""
    n, d = z_rows.shape
    lib = _native.lib()
    ws = core.grow_ws(_IBQ_BWD_WS, z_rows.device, lib.vqk_ibq_backward_ws_bytes(n, d))
    _native.check(lib.vqk_ibq_backward_f32(z_rows.data_ptr(), e.data_ptr(), idx.data_ptr(), lse.data_ptr(), ebar.data_ptr(),
                                           core._p(dq_rows), core.dcode(dq_rows.dtype) if dq_rows is not None else core.F32, n,
                                           e.shape[0], d, inv_t, cz, ce, core._p(gs), dz_rows.data_ptr(), core._p(de), ws.data_ptr(),
                                           ws.numel() * ws.element_size(), core._stream()), 'ibq_backward')


class IBQLookupFn(torch.autograd.Function):
    """Index-backpropagation lookup: the token is the argmax of softmax(z E^T / T), the output the gathered code, and the gradient
    reaches z and EVERY code through the softmax.  Returns (q [B,D,H,W] in out_dtype, idx [B, H*W] int64, loss 0-dim fp32,
    hist int32 [K]).  Without a gradient to compute (torch.no_grad(), frozen inputs) the forward runs the argmax-only kernel mode."""

    @staticmethod
    def forward(ctx, z, codebook, beta: float, temperature: float, out_dtype):
        core._require_gpu(z)
        k, d, inv_t = _check_ibq(codebook, temperature)
        z, flat, (b, dz_, h, w) = nhwc_rows(z)
        if dz_ != d:
            raise ValueError(f'ibq: latents must have {d} channels, got {dz_}')
        n = b * h * w
        lo = out_dtype == torch.bfloat16
        e = core.f32c(codebook.detach())
        fused = ibq_fused_serves(e)
        soft = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        if fused:
            idx, q32, qlo, sse, hist, lse, ebar = _ibq_forward(flat, e, inv_t, soft, not lo, lo, True)
        else:
            idx, q32, qlo, sse, hist, lse, ebar = ibq_staged(flat, e, temperature, lo)
        q = rows_image(qlo if lo else q32, (b, d, h, w))
        loss = sse.view(()) * ((2.0 + beta) / float(n * d))
        if soft:
            ctx.save_for_backward(z, e, idx, lse, ebar)
        ctx.cfg = (beta, inv_t, n, k, d, fused)
        ctx.cb_param = codebook
        ctx.mark_non_differentiable(idx, hist)
        ctx.set_materialize_grads(False)                       # an unused output's gradient arrives as None (dq = NULL in the kernel), not as zeros
        return q, idx.view(b, h * w), loss, hist

    @staticmethod
    def backward(ctx, dq, _didx, dloss, _dhist):
        z, e, idx, lse, ebar = ctx.saved_tensors
        beta, inv_t, n, k, d, fused = ctx.cfg
        want_de = bool(ctx.needs_input_grad[1])
        if dq is None and dloss is None:                       # g absent and s absent: the result is zero
            return torch.zeros_like(z, memory_format=core._CL), None, None, None, None
        dz, de, de_tgt, gs, dqc, cz, ce = lookup_backward_frame(ctx, z, dq, dloss, beta, k, want_de)
        dz_rows = dz.permute(0, 2, 3, 1).reshape(n, d)         # views of the NHWC memory
        z_rows = z.permute(0, 2, 3, 1).reshape(n, d)
        dq_rows = dqc.permute(0, 2, 3, 1).reshape(n, d) if dqc is not None else None
        if fused and n * k > IBQ_STAGED_BWD_MAX_NK:
            ibq_backward_rows(z_rows, e, idx, lse, ebar, dq_rows, inv_t, cz, ce, gs, dz_rows, de)
        else:
            s = gs if gs is not None else 0.0
            dzr, des = ibq_backward_staged(z_rows, e, idx, lse, ebar, dq_rows, inv_t, s * cz, s * ce, want_de)
            dz_rows.copy_(dzr)
            if want_de:
                de.add_(des)
        return dz, (de if want_de and de_tgt is None else None), None, None, None


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations', 'hist_sse', 'lookup_backward_frame', 'nhwc_rows', 'rows_image')]
