"""Both sides of the conv launchers' shape guards against float64 torch.

The launch plans (csrc/conv.hip::plan_fprop, csrc/conv_wgrad.hip::plan_wgrad) and, for the weight gradients, the routing
between entry points in ops.py pick a kernel from the map shape: w % 32, w % 16, h % 8, the 64 KiB LDS bound of the edge-conv kernels,
the 32-bit buffer offsets of the matrix/auxiliary-wave kernel.  Every case below sits just inside or just outside one of those
guards, runs the product's autograd node (``ops.conv2d``: y, dx, dW) and compares with F.conv2d / its autograd in float64 on
the same inputs (bf16 mode: on the bf16-rounded inputs).  Where the library chooses internally, the case also runs the general
implicit-GEMM kernel (vqk_conv_set_variant(0)) through the raw launchers, requires it to match float64 too, and requires the
specialised kernel to differ from it in at least one bit where a specialised kernel is expected to serve.

Tolerances are the existing ones of each kernel family:
  fp32 edge convs    2e-6 of max |ref| (fprop / data gradient), 1e-5 (weight gradient)      tests/test_gpu_thin_f32.py
  fp32 general       5e-6 of max |ref| (fp32 summation noise at K = 9 * 128)                  tests/test_gpu_conv_x3.py
  bf16x3             3e-5 of max |ref|                                                        tests/test_gpu_conv_x3.py
  bf16               one bf16 rounding per element of y / dx; dW 2e-5 (norm) and 1e-4 (max)   tests/test_gpu_mx_vs_torch.py
"""
import importlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
native = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd._native')
DEV, F32, BF, CL = 'cuda:0', torch.float32, torch.bfloat16, torch.channels_last
BF_EPS = 2.0 ** -8


def _relmax(a, ref):
    return float((a.double() - ref).abs().max()) / float(ref.abs().max())


def _check_bf16(got, want, what, roundings=1):
    """tests/test_gpu_mx_vs_torch.py::_check: one bf16 rounding per element, relative to the element plus the typical magnitude"""
    got, want = got.double(), want.double()
    tol = roundings * BF_EPS * (want.abs() + want.abs().mean())
    worst = float(((got - want).abs() / tol).max())
    rel = float((got - want).norm() / want.norm())
    assert rel < 3e-3 * roundings, (what, rel)
    assert worst < 1.0, (what, worst)


def _check_dw_bf16(got, want, what):
    """fp32 accumulation of exact bf16 products (tests/test_gpu_mx_vs_torch.py)"""
    assert float((got.double() - want).norm() / want.norm()) < 2e-5, what
    assert _relmax(got, want) < 1e-4, what


def _check(mode, got, want, what, wgrad=False, short=False):
    """``short``: an fp32 sum of 36 products (the 4-channel side contracted); otherwise 9 * C of them"""
    if mode == 'bf16':
        return _check_dw_bf16(got, want, what) if wgrad else _check_bf16(got, want, what)
    if mode == 'bf16x3':
        tol = 3e-5
    elif wgrad:
        tol = 1e-5
    else:
        tol = 2e-6 if short else 5e-6
    e = _relmax(got, want)
    assert e < tol, (what, e, tol)


def _data(mode, n, cin, cout, h, w, ups, seed, bias=False):
    """inputs on the device, rounded to bf16 in bf16 mode so that the float64 reference sees the kernel's operands"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    k = 3
    s = 2 if ups else 1
    x = torch.randn(n, cin, h, w, device=DEV, generator=g)
    wt = torch.randn(cout, cin, k, k, device=DEV, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, device=DEV, generator=g) if bias else None
    dy = torch.randn(n, cout, h * s, w * s, device=DEV, generator=g)
    if mode == 'bf16':
        x, wt, dy = x.to(BF).float(), wt.to(BF).float(), dy.to(BF).float()
    return x, wt, b, dy


def _ref64(x, wt, b, dy, ups):
    xd = x.double().requires_grad_(True)
    wd = wt.double().requires_grad_(True)
    xu = F.interpolate(xd, scale_factor=2, mode='nearest') if ups else xd
    y = F.conv2d(xu, wd, b.double() if b is not None else None, padding=wt.shape[2] // 2)
    y.backward(dy.double())
    return y.detach(), xd.grad, wd.grad


def _pad_c(t, c):
    return t if t.shape[1] == c else F.pad(t, (0, 0, 0, 0, 0, c - t.shape[1]))


def _product(mode, x, wt, b, dy, ups, events=True):
    """ops.conv2d autograd (forward on this thread, backward on the autograd engine's device thread)"""
    dt = BF if mode == 'bf16' else F32
    ops.set_conv_products('bf16x3' if mode == 'bf16x3' else 'fp32')
    e = ops.epc(dt)
    cin, cout = x.shape[1], wt.shape[0]
    xd = _pad_c(x, -(-cin // e) * e).to(dt).contiguous(memory_format=CL).requires_grad_(True)
    wd = wt.clone().contiguous(memory_format=CL).requires_grad_(True)
    bd = b.clone().requires_grad_(True) if b is not None else None
    if events:
        ops.KERNEL_EVENTS = []
    try:
        y = ops.conv2d(xd, wd, bd, ups=ups)
        y[:, :cout].backward(dy.to(dt).contiguous(memory_format=CL))
        torch.cuda.synchronize()
    finally:
        ev, ops.KERNEL_EVENTS = ops.KERNEL_EVENTS, None
        ops.set_conv_products('fp32')
    names = [r[0] for r in ev] if events else []
    return y.detach()[:, :cout], xd.grad[:, :cin], wd.grad, names


def _general(mode, x, wt, dy, ups):
    """the general implicit-GEMM kernels (vqk_conv_set_variant(0) is per host thread: raw launchers on this thread)"""
    dt = BF if mode == 'bf16' else F32
    e = ops.epc(dt)
    cin, cout = x.shape[1], wt.shape[0]
    ci, co = -(-cin // e) * e, -(-cout // e) * e
    xp = _pad_c(x, ci).to(dt).contiguous(memory_format=CL)
    dyp = _pad_c(dy, co).to(dt).contiguous(memory_format=CL)
    wmem = torch.zeros(co, 3, 3, ci, device=DEV)
    wmem[:cout, :, :, :cin] = wt.permute(0, 2, 3, 1)
    wmem = wmem.reshape(-1)
    native.lib().vqk_conv_set_variant(0)
    try:
        n, _, h, w = xp.shape
        assert ops.weight_layout(dt, n, h, w, ci, co, 3, ups, x3=False) == 0
        y = ops.raw_conv_fprop(xp, ops.pack_weights(wmem, dt, co, ci, 3, False, 0), None, None, 3, ups, 0, dt, co, 0)
        dx = ops.raw_conv_fprop(dyp, ops.pack_weights(wmem, dt, co, ci, 3, True, 0), None, None, 3, False, 0, dt, ci, 0)
        if ups:
            dx = ops.raw_pool(dx, 1.0)
        dw = ops.raw_conv_wgrad(xp, dyp, 3, ups)
        torch.cuda.synchronize()
    finally:
        native.lib().vqk_conv_set_variant(-1)
    return y[:, :cout], dx[:, :cin], dw[:cout, :cin]


def _run(mode, n, cin, cout, h, w, ups=False, bias=False, general=True, seed=0):
    x, wt, b, dy = _data(mode, n, cin, cout, h, w, ups, seed or (cin + 3 * cout + h + 5 * w + ups), bias)
    ry, rdx, rdw = _ref64(x, wt, b, dy, ups)
    y, dx, dw, names = _product(mode, x, wt, b, dy, ups)
    short_y, short_dx = cin <= 4, cout <= 4
    _check(mode, y, ry, 'y', short=short_y)
    _check(mode, dx, rdx, 'dx', short=short_dx)
    _check(mode, dw, rdw, 'dW', wgrad=True)
    gen = None
    if general:
        gy, gdx, gdw = _general(mode, x, wt, dy, ups)
        if b is not None:
            gy = gy + b.to(gy.dtype).view(1, -1, 1, 1)
        _check(mode, gy, ry, 'y (general)', short=short_y and b is None)
        _check(mode, gdx, rdx, 'dx (general)', short=short_dx)
        _check(mode, gdw, rdw, 'dW (general)', wgrad=True)
        gen = (gy, gdx, gdw)
    return (y, dx, dw), gen, names


def _differs(a, b):
    return not torch.equal(a.float(), b.float())


# ---------------------------------------------------------------------------------------------- fp32 edge convs (conv_thin_f32.hip)
# (n, wide channels, h, w, thin wgrad serves): LDS bound (R + 2) * (w + 2) * 16 <= 64 KiB per R; h % 8 in {0, 4, 2, odd} -> R = 8 / 4 /
# 2 / 1; 1 x 1376 fits no R (general kernel).  Thin-input fprop: 10 * (w + 2) * 16 <= 64 KiB; thin-output fprop: h % 8, w % 32.
THIN = [(2, 128, 8, 400, True), (2, 128, 8, 408, True), (1, 64, 512, 512, True), (2, 128, 12, 512, True), (2, 256, 10, 512, True),
        (1, 128, 9, 1024, True), (2, 128, 1, 1376, False), (2, 128, 24, 48, True), (1, 128, 1024, 408, True)]


@pytest.mark.parametrize('n,c,h,w,served', THIN)
def test_fp32_edge_convs(n, c, h, w, served):
    """conv_in (3 -> C on the 4-channel image: thin-x weight gradient, mode 0) and conv_out (C -> 3, + bias: thin-dy weight
    gradient, mode 1) at both sides of every guard of the exact-fp32 edge kernels"""
    for cin, cout, bias in ((3, c, False), (c, 3, True)):
        prod, gen, _ = _run('fp32', n, cin, cout, h, w, bias=bias)
        if served:
            assert _differs(prod[2], gen[2]), ('thin weight-gradient kernel did not serve', cin, cout, h, w)


# ---------------------------------------------------------------------------------------------- bf16 3x3: fprop / dgrad / wgrad
# halo_twlog: w % 32 & h % 8 -> 32-wide tiles; w % 16 & h % 16 -> 16-wide; else (or cin not a multiple of 64) the general kernel.  Fewer than 256 tiles without a
# whole 128-cout tile: the half-tile stream path.  Weight gradient: 16-wide patches (w % 16) on the matrix/auxiliary-wave kernel
# (cin, cout % 64), the halo kernels otherwise (8-wide patches when w % 16 != 0), the general kernel when h % 8 != 0.
# (n, cin, cout, h, w, forward kernel, data-gradient kernel, weight-gradient kernel); 'stream' below 256 tiles is the half-tile path
BF16 = [(2, 128, 128, 8, 32, 'mx', 'mx', 'mx'), (2, 128, 128, 16, 16, 'mx', 'mx', 'mx'), (2, 128, 128, 24, 16, 'gen', 'gen', 'mx'),
        (1, 128, 64, 8, 32, 'stream', 'mx', 'mx'), (1, 64, 64, 16, 16, 'stream', 'stream', 'mx'),
        (2, 128, 128, 8, 24, 'gen', 'gen', 'halo'), (2, 96, 64, 16, 48, 'gen', 'stream', 'halo'),
        (2, 128, 128, 12, 32, 'gen', 'gen', 'gen'), (1, 128, 128, 136, 200, 'gen', 'gen', 'halo'),
        (1, 128, 128, 200, 136, 'gen', 'gen', 'halo'), (1, 128, 128, 96, 256, 'mx', 'mx', 'mx'), (1, 128, 128, 256, 96, 'mx', 'mx', 'mx'),
        (1, 128, 128, 512, 512, 'mx', 'mx', 'mx')]
_FNAME = {'mx': 'conv3x3_mx_kernel<bf16>', 'stream': 'conv3x3_stream_kernel<bf16>', 'gen': 'conv_fprop_kernel<bf16>'}
_WNAME = {'mx': 'conv3x3_wgrad_mx_kernel<bf16>', 'halo': 'conv3x3_wgrad_halo_kernel<bf16>', 'gen': 'conv_wgrad_kernel<bf16>'}


@pytest.mark.parametrize('n,cin,cout,h,w,fk,dk,wk', BF16)
def test_bf16_conv3x3(n, cin, cout, h, w, fk, dk, wk):
    prod, gen, names = _run('bf16', n, cin, cout, h, w)
    assert names[0] == _FNAME[fk] and names[1] == _FNAME[dk], names  # forward, data gradient (ops' mirror of the launcher)
    assert [k for k in names if 'wgrad' in k] == [_WNAME[wk]], names  # weight gradient (the library's launch plan)
    # two fp32 sums rounded to bf16 agree on almost every element: only a large map tells the kernels apart
    if (fk, dk) != ('gen', 'gen') and prod[0].numel() >= 1 << 21:
        assert _differs(prod[0], gen[0]) or _differs(prod[1], gen[1]), 'specialised fprop kernel did not serve'
    if wk != 'gen' and n * h * w >= 4096:                          # (one block over a few hundred pixels sums in the general order)
        assert _differs(prod[2], gen[2]), 'specialised weight-gradient kernel did not serve'


def test_bf16_wgrad_p16_kernel():
    """the 16-wide-patch halo weight-gradient kernel (taken when the matrix/auxiliary-wave form is switched off)"""
    x, wt, _, dy = _data('bf16', 2, 128, 128, 16, 48, False, 77)
    _, _, rdw = _ref64(x, wt, None, dy, False)
    xd, dyd = x.to(BF).contiguous(memory_format=CL), dy.to(BF).contiguous(memory_format=CL)
    native.lib().vqk_set_tuning(b'WGMX', 0)
    ops.KERNEL_EVENTS = []
    try:
        dw = ops.raw_conv_wgrad(xd, dyd, 3, False)
        torch.cuda.synchronize()
    finally:
        native.lib().vqk_set_tuning(b'WGMX', 1)
        names, ops.KERNEL_EVENTS = [e[0] for e in ops.KERNEL_EVENTS], None
    assert names == ['conv3x3_wgrad_p16_kernel<bf16>'], names
    _check_dw_bf16(dw, rdw, 'p16')
    _, _, gdw = _general('bf16', x, wt, dy, False)
    assert _differs(dw, gdw)


# ---------------------------------------------------------------------------------------------- bf16x3 (conv_x3.hip)
# x3_serves: h % 8, w % 16, cin / cout % 32 (else the exact-fp32 kernels); weight gradient from the fp32 tensors (h, w % 8) or
# through the split pair tensors (w % 16); the upsample conv's weight gradient in phase form when the INPUT is h, w % 8.
X3 = [(2, 128, 128, 8, 16, False), (2, 128, 128, 8, 24, False), (2, 128, 128, 48, 16, False), (1, 128, 128, 136, 200, False),
      (1, 128, 128, 512, 512, False), (1, 128, 128, 68, 100, True), (1, 128, 128, 64, 96, True)]


@pytest.mark.parametrize('n,cin,cout,h,w,ups', X3)
def test_bf16x3_conv3x3(n, cin, cout, h, w, ups):
    _, _, names = _run('bf16x3', n, cin, cout, h, w, ups=ups, general=False)
    s = 2 if ups else 1
    if ops.x3_serves(F32, None, h * s, w * s, cin, cout, 3):
        assert any(k.startswith('conv3x3_x3_kernel') for k in names), names
    else:
        assert not any('x3' in k for k in names[:1]), names


# ---------------------------------------------------------------------------------------------- bf16 edge convs (conv_edge.hip)
# thin-input fprop: w % 32; thin-output fprop: h % 8, w % 32; K = 72 weight gradient: (h * w) % 128, w % 128 or 128 % w
EDGE = [(2, 8, 32), (2, 8, 64), (1, 16, 200), (1, 512, 512), (2, 64, 8)]


@pytest.mark.parametrize('n,h,w', EDGE)
def test_bf16_edge_convs(n, h, w):
    for cin, cout, bias in ((3, 128, False), (128, 3, True)):
        x, wt, b, dy = _data('bf16', n, cin, cout, h, w, False, h + w + cin, bias)
        ry, rdx, rdw = _ref64(x, wt, b, dy, False)
        y, dx, dw, names = _product('bf16', x, wt, b, dy, False)
        _check_bf16(y, ry, 'y', roundings=2 if bias else 1)          # bias: one more rounding (csrc/conv_mx.hip header)
        _check_bf16(dx, rdx, 'dx')
        _check_dw_bf16(dw, rdw, 'dW')
        xp = _pad_c(x, -(-cin // 8) * 8).to(BF).contiguous(memory_format=CL)
        dyp = _pad_c(dy, -(-cout // 8) * 8).to(BF).contiguous(memory_format=CL)
        served = ops.edge_wgrad_served(xp, dyp, 3, False)
        assert served == ((h * w) % 128 == 0 and (w % 128 == 0 or 128 % w == 0))
        assert ('conv3x3_wgrad_thin_kernel<bf16>' in names) == served, names


# ---------------------------------------------------------------------------------------------- 1x1 shortcut, pooled epilogue, upsample
@pytest.mark.parametrize('h,w', [(512, 512), (136, 200)])
def test_bf16_1x1_shortcut(h, w):
    x, wt, _, dy = _data('bf16', 1, 128, 256, h, w, False, 5)
    wt = wt[:, :, 1:2, 1:2].contiguous()
    xd = x.double().requires_grad_(True)
    wd = wt.double().requires_grad_(True)
    F.conv2d(xd, wd).backward(dy.double())
    ry = F.conv2d(x.double(), wt.double())
    xg = x.to(BF).contiguous(memory_format=CL).requires_grad_(True)
    wg = wt.clone().contiguous(memory_format=CL).requires_grad_(True)
    ops.KERNEL_EVENTS = []
    try:
        y = ops.conv2d(xg, wg)
        y.backward(dy.to(BF).contiguous(memory_format=CL))
        torch.cuda.synchronize()
    finally:
        names, ops.KERNEL_EVENTS = [r[0] for r in ops.KERNEL_EVENTS], None
    _check_bf16(y.detach(), ry, 'y')
    _check_bf16(xg.grad, xd.grad, 'dx')
    _check_dw_bf16(wg.grad, wd.grad, 'dW')
    # the NTAP = 1 form of the matrix/auxiliary-wave kernel works on the 8 x 32 pixel tiles: off that grid, the general kernel
    kname = 'conv1x1_mx_kernel<bf16> (HBM)' if (h % 8, w % 32) == (0, 0) else 'conv_fprop_kernel<bf16>'
    assert names.count(kname) == 2, names


@pytest.mark.parametrize('h,w', [(512, 512), (136, 200)])
def test_bf16_pooled_epilogue(h, w):
    """pool_scale * sum-pool2x2(conv(x) + bias + residual) at half resolution (the ResBlock + Downsample pair)"""
    x, wt, b, _ = _data('bf16', 1, 128, 128, h, w, False, 6, bias=True)
    g = torch.Generator(device=DEV).manual_seed(7)
    res = torch.randn(1, 128, h, w, device=DEV, generator=g).to(BF).float()
    want = F.avg_pool2d(F.conv2d(x.double(), wt.double(), b.double(), padding=1) + res.double(), 2)
    layout = ops.weight_layout(BF, 1, h, w, 128, 128, 3, False)
    if not ops.can_pool_epilogue(BF, 128, layout):
        assert (h % 8, w % 32) != (0, 0)                           # off the tile grid: the plain conv + a pooling pass
        return
    wq = ops.pack_weights(wt.permute(0, 2, 3, 1).reshape(-1).contiguous(), BF, 128, 128, 3, False, layout)
    y = ops.raw_conv_fprop_pooled(x.to(BF).contiguous(memory_format=CL), wq, b, res.to(BF).contiguous(memory_format=CL), 3, False,
                                  128, 0.25)
    torch.cuda.synchronize()
    _check_bf16(y, want, 'pooled', roundings=2)


@pytest.mark.parametrize('mode', ['bf16', 'fp32', 'bf16x3'])
@pytest.mark.parametrize('h,w', [(256, 256), (68, 100)])
def test_upsample_conv(mode, h, w):
    """nearest x2 + 3x3 with bias (the Decoder's Upsample): phase forms where they serve (bf16: pre-summed bf16 weights, four phases
    through bf16 -- the norm bounds of tests/test_gpu_mx_vs_torch.py::test_phase_form_upsample_fwd_and_dgrad_vs_torch)"""
    x, wt, b, dy = _data(mode, 1, 128, 128, h, w, True, 8, bias=True)
    ry, rdx, rdw = _ref64(x, wt, b, dy, True)
    y, dx, dw, names = _product(mode, x, wt, b, dy, True)
    if mode == 'bf16':
        assert float((y.double() - ry).norm() / ry.norm()) < 4e-3
        assert float((dx.double() - rdx).norm() / rdx.norm()) < 6e-3
        _check_dw_bf16(dw, rdw, 'dW')
    else:
        _check(mode, y, ry, 'y')
        _check(mode, dx, rdx, 'dx')
        _check(mode, dw, rdw, 'dW', wgrad=True)
    assert names, names


# ---------------------------------------------------------------------------------------------- operands near and past 2^31 bytes
def _large(mode, n):
    """128 -> 128 at 512 x 512; dy is zero except on the first and last image, so the float64 reference needs only those two"""
    dt = BF if mode == 'bf16' else F32
    c, h, w = 128, 512, 512
    g = torch.Generator(device=DEV).manual_seed(n)
    xd = wd = y = None
    try:
        xd = torch.randn(n, c, h, w, device=DEV, generator=g, dtype=dt).contiguous(memory_format=CL)
        wt = (torch.randn(c, c, 3, 3, device=DEV, generator=g) / (3 * c ** 0.5))
        if dt == BF:
            wt = wt.to(BF).float()
        ends = torch.randn(2, c, h, w, device=DEV, generator=g).to(dt)
        dy = torch.zeros(n, c, h, w, device=DEV, dtype=dt).contiguous(memory_format=CL)
        dy[0], dy[-1] = ends[0], ends[1]
        x2 = torch.stack([xd[0], xd[-1]]).float()
        ry, rdx, rdw = _ref64(x2, wt, None, ends.float(), False)
        del ends
        ops.set_conv_products('bf16x3' if mode == 'bf16x3' else 'fp32')
        xd.requires_grad_(True)
        wd = wt.clone().contiguous(memory_format=CL).requires_grad_(True)
        ops.KERNEL_EVENTS = []
        try:
            y = ops.conv2d(xd, wd)
            y.backward(dy)
            torch.cuda.synchronize()
        finally:
            names, ops.KERNEL_EVENTS = [r[0] for r in ops.KERNEL_EVENTS], None
            ops.set_conv_products('fp32')
        del dy
        yy, dxx = torch.stack([y[0], y[-1]]).detach(), torch.stack([xd.grad[0], xd.grad[-1]])
        assert float(xd.grad[1:-1].abs().max()) == 0.0                # the zero images of dy reach nothing
        _check(mode, yy, ry, 'y')
        _check(mode, dxx, rdx, 'dx')
        _check(mode, wd.grad, rdw, 'dW', wgrad=True)
        if mode == 'bf16':
            # the label is the library's own launch plan: the matrix/auxiliary-wave kernel up to its 32-bit offset bound, the
            # stream kernel behind it (n = 33), forward and data gradient
            past_2g = n * c * h * w * 2 >= 0x7fffffff
            assert names.count('conv3x3_stream_kernel<bf16>' if past_2g else 'conv3x3_mx_kernel<bf16>') == 2, names
    finally:
        del xd, wd, y
        torch.cuda.empty_cache()


def test_large_bf16_mx_just_under_2g():
    _large('bf16', 31)


def test_large_bf16_stream_past_2g():
    _large('bf16', 33)


@pytest.mark.parametrize('mode', ['fp32', 'bf16x3'])
def test_large_fp32_past_2g(mode):
    _large(mode, 17)
