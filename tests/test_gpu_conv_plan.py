"""Every forward kernel form of tests/conv_plan_rows.py launched once at its row's shape, against the forced im2col kernel
(vqk_conv_set_variant(0), plain weights) on the same operands, with the comparisons and tolerances of tests/test_gpu_conv_edges.py:

  bf16 output      _check_bf16 with two roundings: the form and the im2col kernel each round the exact sum to bf16 once
  pooled epilogue  conv + residual, as that file's pooled test: against the 2x2 average of the im2col kernel's FP32 output with
                   two roundings (the drain parks the conv sums as bf16, then rounds the pooled value)
  fp32 output      5e-6 of max |ref| (fp32 summation noise), 2e-6 for the 36-product sums of the fp32 thin kernels
  split products   3e-5 of max |ref|

The event label of each launch must be the name the plan gives.  Rows that only differ from another row by the fused GroupNorm
sums (their form is the matrix/auxiliary-wave kernel: tests/test_gpu_conv_gnstats.py) or by the general-conv flag launch nothing
here."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from tests import conv_plan_rows as T
from tests.test_gpu_conv_edges import _check, _check_bf16

pytestmark = pytest.mark.gpu

ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
native = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd._native')
DEV, CL = 'cuda:0', torch.channels_last
DT = {T.F32: torch.float32, T.BF16: torch.bfloat16}
LAUNCHED = [r for r in T.ROWS if r.form >= 0 and not r.flags & (T.GNSTATS | T.GENERAL)]


def test_every_form_is_launched():
    assert {r.form for r in LAUNCHED} == set(range(14))


def _run(r, x, wmem, res, variant, layout, tuning, scratch, odt=None):
    lib = native.lib()
    dt, odt = DT[r.dtype], odt or DT[r.out_dtype]
    wq = ops.pack_weights(wmem, dt, r.cout, r.cin, r.ksize, False, layout)
    ops._stream()                                                # the thread's workspace context, before its scratch is taken away
    for slot, val in tuning.items():
        assert lib.vqk_set_tuning(slot.encode(), val) == 0
    lib.vqk_conv_set_variant(variant)
    if not scratch:
        lib.vqk_set_scratch(0, 0)
    ops.KERNEL_EVENTS = []
    try:
        if r.flags & T.POOL and layout:
            y = ops.raw_conv_fprop_pooled(x, wq, None, res, r.ksize, bool(r.ups), r.cout, 0.25)
        else:
            y = ops.raw_conv_fprop(x, wq, None, res, r.ksize, bool(r.ups), r.act, odt, r.cout, layout)
        torch.cuda.synchronize()
    finally:
        names, ops.KERNEL_EVENTS = [e[0] for e in ops.KERNEL_EVENTS], None
        lib.vqk_conv_set_variant(-1)
        if tuning:
            lib.vqk_reset_tuning()
            native.apply_env_tuning(lib)
        ops.rearm_workspaces()
    return y, names


@pytest.mark.parametrize('r', LAUNCHED, ids=[r.name for r in LAUNCHED])
def test_form_against_im2col(r):
    dt = DT[r.dtype]
    g = torch.Generator(device=DEV).manual_seed(r.cin + 3 * r.cout + r.h + 5 * r.w + r.ksize)
    s = 1 << r.ups
    x = torch.randn(r.n, r.cin, r.h, r.w, device=DEV, generator=g).to(dt).contiguous(memory_format=CL)
    wmem = (torch.randn(r.cout, r.ksize, r.ksize, r.cin, device=DEV, generator=g) / (r.ksize * r.cin ** 0.5)).reshape(-1)
    if dt == torch.bfloat16:
        wmem = wmem.to(dt).float()
    res = None
    if r.flags & T.RESIDUAL:
        res = torch.randn(r.n, r.cout, r.h * s, r.w * s, device=DEV, generator=g).to(DT[r.out_dtype]).contiguous(memory_format=CL)
    y, names = _run(r, x, wmem, res, r.variant, r.wlayout, r.tuning, r.scratch)
    if r.flags & T.POOL:
        want, _ = _run(r, x, wmem, res.float() if res is not None else None, 0, 0, {}, True, torch.float32)
    else:
        want, _ = _run(r, x, wmem, res, 0, 0, {}, True)
    assert names == [native.lib().vqk_conv_fprop_form_name(r.form, r.dtype).decode()], names
    want = want.double()
    if r.flags & T.POOL:
        want = F.avg_pool2d(want, 2)
    assert y.shape == want.shape
    if r.out_dtype == T.BF16:
        _check_bf16(y, want, r.name, roundings=2)
    else:
        _check('bf16x3' if r.wlayout == 5 else 'fp32', y, want, r.name, short=min(r.cin, r.cout) <= 4)
