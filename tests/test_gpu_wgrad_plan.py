"""Every launchable row of tests/wgrad_plan_rows.py through its entry point, under the row's variant, tuning, block cap and
deterministic workspace: the launcher serves what the plan says it serves, the recorded event carries the kernel name and the
number of launches that the TABLE gives (the event itself comes from the plan, so this half only catches a launcher that refuses or
a plan that left the table), and dw agrees with a float64 reference -- the state rows (one launch per phase, block cap, the A/B
slots, pair operands) reach launch paths that no other test runs.  Tolerances: those tests/test_gpu_conv_edges.py applies to the
same kernels at larger shapes (bf16: fp32 sums of exact bf16 products; split products 3e-5, fp32 1e-5 of max |ref|).
The strided row launches nothing here: ops._wgrad_event describes the plain stride-1 problem of its arguments (the host's routing
never sends a strided conv through it), so its label would be that problem's, not the row's."""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_plan_rows as T
from tests.test_gpu_conv_edges import _check

pytestmark = pytest.mark.gpu

ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
native = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd._native')
DEV, CL = 'cuda:0', torch.channels_last
DT = {T.F32: torch.float32, T.BF16: torch.bfloat16}
LAUNCHED = [r for r in T.ROWS if r.form >= 0 and r.stride == 1]


def test_every_form_is_launched():
    assert {r.form for r in LAUNCHED} == set(range(16))


def _operands(r):
    """x, dy as the entry point of r.op takes them (include/vqk.h), dw zeroed"""
    g = torch.Generator(device=DEV).manual_seed(r.cin + 3 * r.cout + r.h + 5 * r.w + r.ksize + r.op)
    dt = torch.bfloat16 if r.op == T.FOLD else DT[r.dtype]
    pair = 2 if r.op == T.FOLD else 1                            # (hi | lo) pair tensors
    hx, wx = (2 * r.h, 2 * r.w) if r.op == T.POOLED_DY_PHASE else (r.h, r.w)
    if r.op == T.POOLED_DY or (r.op == T.X3_OP and r.ups == 2):
        hy, wy = r.h // 2, r.w // 2
    elif r.op == T.UPS_PHASE:
        hy, wy = 2 * r.h, 2 * r.w
    elif r.op == T.POOLED_DY_PHASE:
        hy, wy = r.h, r.w
    else:
        hy, wy = r.h_out, r.w_out
    x = torch.randn(r.n, pair * r.cin, hx, wx, device=DEV, generator=g).to(dt).contiguous(memory_format=CL)
    dy = torch.randn(r.n, pair * r.cout, hy, wy, device=DEV, generator=g).to(dt).contiguous(memory_format=CL)
    return x, dy, torch.zeros(r.cout, r.ksize, r.ksize, r.cin, device=DEV)


def _reference(r, x, dy):
    """float64 dw of the row's problem from the operands of :func:`_operands` (scale 1)"""
    up = lambda t: F.interpolate(t, scale_factor=2.0, mode='nearest')      # noqa: E731
    xd, dyd = x.double(), dy.double()
    if r.op == T.UPS_PHASE or (r.op in (T.PLAIN, T.FOLD, T.X3_OP) and r.ups == 1):
        xd = up(xd)
    if r.op in (T.POOLED_DY, T.POOLED_DY_PHASE) or (r.op == T.X3_OP and r.ups == 2):
        dyd = up(dyd)                                            # every pooled pixel stands for its 2x2 block

    def wg(a, b):
        wd = torch.zeros(r.cout, r.cin, r.ksize, r.ksize, device=DEV, dtype=torch.float64, requires_grad=True)
        (F.conv2d(a, wd, None, stride=r.stride, padding=r.pad) * b).sum().backward()
        return wd.grad
    if r.op != T.FOLD:
        return wg(xd, dyd)
    (xh, xl), (dh, dl) = xd.split(r.cin, 1), dyd.split(r.cout, 1)            # (hi | lo): dy_hi x_hi + dy_hi x_lo + dy_lo x_hi
    return wg(xh + xl, dh) + wg(xh, dl)


def _entry(lib, r, x, dy, dw):
    """(name for the error message, the call) of the row's entry point"""
    dims = (r.n, r.h, r.w, r.cin, r.cout)
    zeros = ops.zero_page(x.device).data_ptr()
    if r.op == T.PLAIN:
        return 'conv2d_wgrad', lambda: lib.vqk_conv2d_wgrad(r.dtype, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), *dims, r.ksize, r.ups,
                                                            zeros, ops._stream())
    if r.op == T.FOLD:
        return 'conv2d_wgrad_x3', lambda: lib.vqk_conv2d_wgrad_x3(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), *dims, r.ups, 1.0, zeros,
                                                                  ops._stream())
    if r.op == T.X3_OP:
        return 'conv2d_wgrad_x3_f32', lambda: lib.vqk_conv2d_wgrad_x3_f32(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), *dims, r.ups, 1.0,
                                                                          ops._stream())
    name = {T.POOLED_DY: 'conv2d_wgrad_pooled_dy', T.UPS_PHASE: 'conv2d_wgrad_ups_phase', T.POOLED_DY_PHASE: 'conv2d_wgrad_pooled_dy_phase'}[r.op]
    fn = getattr(lib, 'vqk_' + name)
    return name, lambda: fn(r.dtype, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), *dims, 1.0, zeros, ops._stream())


@pytest.mark.parametrize('r', LAUNCHED, ids=[r.name for r in LAUNCHED])
def test_event_is_the_plan(r):
    lib = native.lib()
    x, dy, dw = _operands(r)
    what, call = _entry(lib, r, x, dy, dw)
    ops._stream()                                                # the thread's workspace context, before its deterministic state is replaced
    ws = torch.empty(max(r.det or 0, 16) // 4, device=DEV) if r.det is not None else None
    for slot, val in r.tuning.items():
        assert lib.vqk_set_tuning(slot.encode(), val) == 0
    lib.vqk_conv_set_variant(r.variant)
    lib.vqk_conv_set_block_caps(0, r.cap)
    if ws is not None:
        assert lib.vqk_set_deterministic(1, ws.data_ptr(), r.det) == 0
    details = (ctypes.c_int * 5)()
    ops.KERNEL_EVENTS = []
    try:
        form = lib.vqk_conv_wgrad_plan(r.op, r.dtype, r.n, r.h, r.w, r.cin, r.cout, r.ksize, r.stride, r.pad, r.ups, r.h_out, r.w_out,
                                       details)
        xe = torch.empty(r.n, r.cin, 1, 1, dtype=DT[r.dtype], device='meta')      # (the event reads n, cin and the dtype off it)
        served = ops._run_wgrad(what, call, r.op, xe, r.cout, r.h, r.w, r.ksize, r.ups, 1.0, '')
        torch.cuda.synchronize()
    finally:
        events, ops.KERNEL_EVENTS = ops.KERNEL_EVENTS, None
        lib.vqk_conv_set_block_caps(0, 0)
        lib.vqk_conv_set_variant(-1)
        if r.tuning:
            lib.vqk_reset_tuning()
            native.apply_env_tuning(lib)
        ops.rearm_workspaces()
    assert served and form == r.form and details[3] == r.launches
    assert [(e[0], e[5]) for e in events] == [(T.NAMES[r.form], r.launches)], events
    _check('bf16x3' if r.op == T.X3_OP else 'bf16' if x.dtype == torch.bfloat16 else 'fp32', dw.permute(0, 3, 1, 2), _reference(r, x, dy),
           r.name, wgrad=True)
