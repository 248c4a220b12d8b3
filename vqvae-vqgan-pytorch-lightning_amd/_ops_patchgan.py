"""PatchGAN discriminator operators over the vqk C-ABI (csrc/patchgan.hip): the 4x4 conv (+ bias + LeakyReLU) and BatchNorm
(+ LeakyReLU) autograd Functions behind ``modules/loss/patchgan.py``.  Private part of :mod:`ops` like ``_ops_attn.py`` (imported at
the end of ``ops.py``, which re-exports every name); shared infrastructure is reached through ``core``.

The kernels read the fp32 master weights in place (the bf16 mode rounds them as it stages them), so there is no packed operand to
refresh after an optimizer step.  First-order only: the backward passes are not differentiable again."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core

BN_MOMENTUM = 0.1
BN_EPS = 1e-5
_PG_WS: dict = {}            # core._wkey() -> byte workspace of this family's kernels (wgrad partials, BatchNorm partial sums)


def _pg_first_order_only(name: str):
    if torch.is_grad_enabled():
        raise RuntimeError(f'vqk: {name} is first-order only: its backward cannot be differentiated again (create_graph=True / R1 '
                           f'is not built for the PatchGAN discriminator)')


def conv4x4_out(size: int, stride: int) -> int:
    return (size + 2 - 4) // stride + 1


def _pg_weight_mem(weight) -> torch.Tensor:
    """the [O][4][4][I] fp32 memory of a logical [O, I, 4, 4] parameter: the parameter itself when it is channels_last"""
    w = weight.detach().permute(0, 2, 3, 1)
    return w if (w.is_contiguous() and w.dtype == torch.float32) else w.to(torch.float32).contiguous()


def _pg_grad_target(param, shape_mem=None):
    """the arena view of ``param`` as the kernels address it (None: the gradient is returned through autograd)"""
    tgt = core.direct_grad(param)
    if tgt is None or tgt.dtype != torch.float32:
        return None
    if shape_mem is not None:
        tgt = tgt.permute(0, 2, 3, 1)
    return tgt if tgt.is_contiguous() else None


def conv4x4_wgrad_plan(n, h, w, cin, cin_w, cout, stride) -> int:
    """number of pixel partials of the weight gradient of this layer (a function of the shape only)"""
    return int(_native.lib().vqk_conv4x4_wgrad_plan(n, h, w, cin, cin_w, cout, stride))


def raw_conv4x4_fprop(x, wmem, bias, stride: int, lrelu: bool):
    n, cin, h, w = x.shape
    o, i = wmem.shape[0], wmem.shape[3]
    e = core.epc(x.dtype)
    co_ld = -(-o // e) * e
    ho, wo = conv4x4_out(h, stride), conv4x4_out(w, stride)
    if ho < 1 or wo < 1:
        raise ValueError(f'conv4x4: a {h}x{w} map is too small for stride {stride}')
    y = core.empty_nhwc(n, co_ld, ho, wo, x.dtype, x.device)
    st = core._timed('pg_conv_kernel (fprop)', 2.0 * n * ho * wo * o * i * 16,
                     lambda: _native.lib().vqk_conv4x4_fprop(core.dcode(x.dtype), x.data_ptr(), wmem.data_ptr(), core._p(bias), y.data_ptr(),
                                                             n, h, w, cin, i, o, co_ld, stride, int(lrelu), core._stream()))
    _native.check(st, 'conv4x4_fprop')
    return y


def raw_conv4x4_dgrad(t, wmem, h: int, w: int, cin: int, stride: int):
    n, co_ld = t.shape[0], t.shape[1]
    o, i = wmem.shape[0], wmem.shape[3]
    dx = core.empty_nhwc(n, cin, h, w, t.dtype, t.device)
    st = core._timed('pg_conv_kernel (dgrad)', 2.0 * n * t.shape[2] * t.shape[3] * o * i * 16,
                     lambda: _native.lib().vqk_conv4x4_dgrad(core.dcode(t.dtype), t.data_ptr(), wmem.data_ptr(), dx.data_ptr(), n, h, w, cin, i,
                                                             o, co_ld, stride, core._stream()))
    _native.check(st, 'conv4x4_dgrad')
    return dx


def raw_conv4x4_wgrad(x, t, dw_mem, o: int, i: int, stride: int, scale: float = 1.0, accumulate: bool = True):
    """dw_mem[O][4][4][I] (+)= scale * wgrad(x, t)"""
    n, cin, h, w = x.shape
    lib = _native.lib()
    nbytes = int(lib.vqk_conv4x4_wgrad_ws_bytes(n, h, w, cin, i, o, stride))
    if nbytes < 0:
        _native.check(nbytes, 'conv4x4_wgrad_ws_bytes')
    ws = core.grow_ws(_PG_WS, x.device, nbytes)
    st = core._timed('pg_wgrad_kernel', 2.0 * n * t.shape[2] * t.shape[3] * o * i * 16,
                     lambda: lib.vqk_conv4x4_wgrad(core.dcode(x.dtype), x.data_ptr(), t.data_ptr(), dw_mem.data_ptr(), n, h, w, cin, i, o,
                                                   t.shape[1], stride, float(scale), int(accumulate), ws.data_ptr(), ws.numel(),
                                                   core._stream()), launches=2)
    _native.check(st, 'conv4x4_wgrad')


def raw_conv4x4_bgrad(t, db, o: int, scale: float = 1.0, accumulate: bool = True):
    n, co_ld, ho, wo = t.shape
    rows = n * ho * wo
    lib = _native.lib()
    ws = core.grow_ws(_PG_WS, t.device, int(lib.vqk_bn_ws_bytes(rows, co_ld)))
    _native.check(lib.vqk_conv4x4_bgrad(core.dcode(t.dtype), t.data_ptr(), db.data_ptr(), rows, co_ld, o, float(scale), int(accumulate),
                                        ws.data_ptr(), ws.numel(), core._stream()), 'conv4x4_bgrad')


class Conv4x4Fn(torch.autograd.Function):
    """y = act(conv(x, W, kernel 4, padding 1, stride) + bias), act = LeakyReLU(0.2) or none; x NHWC with whole 16-byte channel
    chunks, W the logical [O, I, 4, 4] fp32 parameter (I <= x's channels: the padded image), y carries O rounded up to a chunk
    (zeros behind O).  Backward: t = dy through the LeakyReLU mask (from y's sign), dx = dgrad(t), dW += wgrad(x, t), db += colsum(t)
    -- straight into the optimizer's arena when ``ops.direct_grad`` gives a view, skipped under ``ops.no_param_grads()``."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride: int, lrelu: bool):
        core._require_gpu(x)
        core._require_gpu(weight)
        x = core.nhwc(x)
        if weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4):
            raise RuntimeError(f'vqk: conv4x4 wants an [O, I, 4, 4] weight, got {tuple(weight.shape)}')
        o, i = weight.shape[0], weight.shape[1]
        if x.shape[1] < i or x.shape[1] % core.epc(x.dtype) or x.shape[1] - i >= core.epc(x.dtype):
            raise RuntimeError(f'vqk: conv4x4 input has {x.shape[1]} channels, weight expects {i}')
        b32 = core.f32c(bias) if bias is not None else None
        y = raw_conv4x4_fprop(x, _pg_weight_mem(weight), b32, stride, lrelu)
        ctx.save_for_backward(x, y if lrelu else None)
        ctx.refs = (weight, bias)
        ctx.cfg = (int(stride), bool(lrelu), o, i)
        return y

    @staticmethod
    def backward(ctx, dy):
        _pg_first_order_only('Conv4x4Fn')
        x, y = ctx.saved_tensors
        weight, bias = ctx.refs
        stride, lrelu, o, i = ctx.cfg
        lib = _native.lib()
        t = core.nhwc(dy if dy.dtype == x.dtype else dy.to(x.dtype))
        if lrelu:
            tm = torch.empty_like(t)
            _native.check(lib.vqk_act_backward(core.dcode(t.dtype), t.data_ptr(), y.data_ptr(), tm.data_ptr(), t.numel(),
                                               core.ACT_CODE['lrelu'], 1.0, core._stream()), 'act_backward')
            t = tm
        n, cin, h, w = x.shape
        param_grads = core._grad_modes()[1]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = raw_conv4x4_dgrad(t, _pg_weight_mem(weight), h, w, cin, stride)
        if ctx.needs_input_grad[1] and param_grads:
            tgt = _pg_grad_target(weight, True)
            if tgt is not None:
                raw_conv4x4_wgrad(x, t, tgt, o, i, stride, 1.0, True)
            else:
                dwm = torch.empty((o, 4, 4, i), dtype=torch.float32, device=x.device)
                raw_conv4x4_wgrad(x, t, dwm, o, i, stride, 1.0, False)
                dw = dwm.permute(0, 3, 1, 2)
        if bias is not None and ctx.needs_input_grad[2] and param_grads:
            tgt = _pg_grad_target(bias)
            if tgt is not None:
                raw_conv4x4_bgrad(t, tgt, o, 1.0, True)
            else:
                db = torch.empty(o, dtype=torch.float32, device=x.device)
                raw_conv4x4_bgrad(t, db, o, 1.0, False)
        return dx, dw, db, None, None


def conv4x4(x, weight, bias=None, stride: int = 2, lrelu: bool = False):
    return Conv4x4Fn.apply(x, weight, bias, int(stride), bool(lrelu))


class BatchNormLReLUFn(torch.autograd.Function):
    """y = act(gamma (x - mean) / sqrt(var + eps) + beta) per channel over N H W, act = LeakyReLU(0.2) or none.  training: batch
    statistics (biased variance); running_mean / running_var (momentum 0.1, unbiased variance) and num_batches_tracked are updated on
    the device by the same launch sequence, so a captured graph carries the update.  eval: the running statistics.  Backward (training
    mode only): the mask is recomputed from the saved input, dgamma / dbeta go into the arena or are returned."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, num_batches_tracked, training: bool, lrelu: bool, eps: float,
                momentum: float):
        core._require_gpu(x)
        x = core.nhwc(x)
        n, c, h, w = x.shape
        rows = n * h * w
        if training and rows == 1:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {tuple(x.shape)}')
        if gamma.numel() != c:
            raise RuntimeError(f'vqk: batch norm over {c} channels with {gamma.numel()} weights')
        lib = _native.lib()
        y = torch.empty_like(x)
        g32, b32 = core.f32c(gamma), core.f32c(beta)
        mean = rstd = None
        nbytes = int(lib.vqk_bn_ws_bytes(rows, c))
        if nbytes < 0:
            _native.check(nbytes, 'bn_ws_bytes')
        ws = core.grow_ws(_PG_WS, x.device, nbytes)
        if training:
            mean = torch.empty(c, dtype=torch.float32, device=x.device)
            rstd = torch.empty(c, dtype=torch.float32, device=x.device)
        _native.check(lib.vqk_bn_forward(core.dcode(x.dtype), x.data_ptr(), g32.data_ptr(), b32.data_ptr(), y.data_ptr(), core._p(mean),
                                         core._p(rstd), core._p(running_mean), core._p(running_var), core._p(num_batches_tracked), rows, c,
                                         float(eps), float(momentum), int(training), int(lrelu), ws.data_ptr(), ws.numel(),
                                         core._stream()), 'bn_forward')
        ctx.save_for_backward(x, mean, rstd)
        ctx.refs = (gamma, beta)
        ctx.cfg = (bool(training), bool(lrelu))
        return y

    @staticmethod
    def backward(ctx, dy):
        _pg_first_order_only('BatchNormLReLUFn')
        x, mean, rstd = ctx.saved_tensors
        gamma, beta = ctx.refs
        training, lrelu = ctx.cfg
        if not training:
            raise RuntimeError('vqk: the eval-mode BatchNorm has no backward (validation runs without gradients)')
        lib = _native.lib()
        n, c, h, w = x.shape
        rows = n * h * w
        dyn = core.nhwc(dy if dy.dtype == x.dtype else dy.to(x.dtype))
        dx = torch.empty_like(x)
        param_grads = core._grad_modes()[1]
        want_g = ctx.needs_input_grad[1] and param_grads
        want_b = ctx.needs_input_grad[2] and param_grads
        tg = _pg_grad_target(gamma) if want_g else None
        tb = _pg_grad_target(beta) if want_b else None
        direct = (not want_g or tg is not None) and (not want_b or tb is not None)
        dg = db = None
        if not direct:
            tg = dg = torch.empty(c, dtype=torch.float32, device=x.device) if want_g else None
            tb = db = torch.empty(c, dtype=torch.float32, device=x.device) if want_b else None
        g32, b32 = core.f32c(gamma), core.f32c(beta)
        ws = core.grow_ws(_PG_WS, x.device, int(lib.vqk_bn_ws_bytes(rows, c)))
        _native.check(lib.vqk_bn_backward(core.dcode(x.dtype), x.data_ptr(), dyn.data_ptr(), g32.data_ptr(), b32.data_ptr(), mean.data_ptr(),
                                          rstd.data_ptr(), dx.data_ptr(), core._p(tg), core._p(tb), int(direct), rows, c, int(lrelu),
                                          ws.data_ptr(), ws.numel(), core._stream()), 'bn_backward')
        return dx, dg, db, None, None, None, None, None, None, None


def batch_norm_lrelu(x, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, training: bool = True,
                     lrelu: bool = True, eps: float = BN_EPS, momentum: float = BN_MOMENTUM):
    return BatchNormLReLUFn.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked, bool(training), bool(lrelu), float(eps),
                                  float(momentum))


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations')]
