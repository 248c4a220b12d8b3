"""Every form of the VQ-GAN loss-path kernels (csrc/gan_ops.hip, ops via _ops_gan.py) against float64, at both sides of each
dispatch guard, in fp32 and bf16, first and second order.

Forms covered and the guard that selects each:
  minibatch stddev  mbstd_stat_kernel / mbstd_bwd_kernel: 256 threads at hw * c < 4096, 1024 from 4096 on;
                    mbstd_bwd_bwd_kernel (the R1 double backward): always 256; mbstd_concat_kernel: zero pad from c + 1 to cp
                    (cp - c = 1 and > 1).  G = min(group, N) in {1, 2, 4, 8}, N / G = 1 and > 1, 1 x 1 / 4 x 4 / looped maps,
                    nearly equal groups (sd near sqrt(1e-8)), the halves = 2 path; G > 8 raises (vqk_mbstd: group <= 8).
  act backward      act_bwd_vec_kernel: count % (4 fp32 | 8 bf16) == 0 and 16-byte aligned pointers; act_bwd_kernel otherwise
                    (ragged count through ActBwdFn, misaligned pointers through the C ABI); act_bwd_colsum_kernel at
                    c % v == 0 and c / v <= 256 (fp32 1024 served, 1028 not; bf16 2048 / 2056), slot counts that leave idle
                    lanes (48, 160), one block and > 2048 x 64 rows; act 0..3, y == 0 exactly, scale and colsum scale != 1.
  conv, twice       ops.conv_act, gx = d y / d x . dy with create_graph, then d<v, gx>/d(x, w, b, dy) (ConvDgradFn.backward,
                    ActBwdFn.backward): 3x3 stride 1 / pad 1, stride 2 / pad 0 (bf16 on both sides of
                    vqk_conv2d_s2_supported(backward=0), which both the forward and ConvDgradFn.backward consult), 1x1 on 1 x 1
                    maps (the FC layers), 3-channel fromrgb, weight gains != 1.
  discriminator R1  Discriminator(..., double_backward=True) against oracle.r1_penalty (float64): the golden size and a
                    512-channel one (mbstd 1024-thread form, 513 -> padded epilogue conv); Discriminator(256) in bf16 and fp32
                    against the reference's fp32 fixture (full_disc256.npz).
  losses / LPIPS    gan_loss_kernel (one block: N 1 .. 1000, logits +-40 and at the hinge kinks, upstream != 1), l1_sum /
                    sse / l1l2_bwd (ragged and >= 2^22 elements, recon == target), SumSqFn, LpipsTapsFn (five taps, the vector
                    and scalar forms in one call, the ppb clamp at > 8192 blocks), maxpool_kernel (ties: first maximum in
                    row-major order wins, as torch), channel_affine_kernel (with / without shift); odd maps raise in maxpool.

Inputs are made exact in the compute dtype first; references are float64 torch restatements of the reference formulas
(oracle/vqvae_oracle.py for the discriminator, pinned to tests/golden/gan.npz by tests/test_oracle_golden.py).

Error measures: ``rel`` relative l2 norm; ``max`` max |got - ref| / max |ref|; ``ulp`` (bf16 outputs) the worst element in units of
one bf16 rounding, 2^-8 * (|ref| + mean |ref|) (tests/test_gpu_conv_edges.py::_check_bf16).  Bounds (_BOUNDS) are about 10x the worst
error measured on MI355X over all cases of this file; the bf16 per-element rule is fixed at one rounding.

Measured worst errors over all cases on MI355X (each check prints its error: run with -s), and the bounds:
  check            measure          fp32 worst  bound     bf16 worst  bound
  mbstd stat       max / ulp        1.7e-7      2e-6      0.40        1 rounding
  mbstd dx         max / ulp        1.3e-7      2e-6      0.67        1 rounding
  mbstd dx, stat   max / rel        8.6e-6      1e-4      2.0e-3      2e-2    (dy zero on the pass-through channels)
  mbstd d2 x       max / rel        2.2e-5      2e-4      4.7e-3      5e-2    (fp32 worst: the nearly equal groups)
  mbstd d2 dy      max / ulp        6.3e-8      1e-6      0.12        1 rounding
  act t            max / ulp        1.1e-7      1e-6      0.90        1 rounding
  act colsum       rel              1.1e-6      1e-5      9.1e-7      1e-5
  conv2 gx         rel              2.2e-7      3e-6      2.8e-3      3e-2
  conv2 d2 w       rel              2.2e-7      3e-6      1.7e-3      2e-2
  conv2 d2 dy      rel              2.3e-7      3e-6      2.8e-3      3e-2
  R1 value         relative         1.7e-7      2e-6      6.9e-3      7e-2
  R1 image grad    rel              1.0e-6      1e-5      5.8e-2      0.5
  R1 d/dtheta      rel per param    3.0e-5      3e-4      -           -       (fp32 worst: a bias; weights 4.4e-7)
                   rel per layer    4.6e-7      5e-6      3.2e-2      0.3
  R1 256^2         value            2.5e-6      3e-5      1.1e-2      0.1     (against the reference's fp32 run:
                   image grad       2.0e-3      2e-2      0.11        0.5      the fp32 numbers are the fixture's own
                   d/dtheta param   1.3e-3      1.5e-2    -           -        rounding; bf16 weights and image are not
                   d/dtheta layer   1.9e-4      2e-3      0.11        0.5      rounded first)
  GAN loss         loss / grad      1.9e-7 / 1.1e-7 (grad relative to upstream / N): bounds 2e-6 / 1e-6
  recon loss       l1, l2 / grad    6.3e-7 / 1.3e-7  5e-6 / 1e-6   5.1e-7 / 0.81  5e-6 / 1 rounding
  sum of squares   value / grad     1.9e-10 / 4.0e-8 2e-9 / 4e-7   2.9e-8 / 0.62  3e-7 / 1 rounding
  LPIPS taps       value / dfy      1.5e-7 / 1.3e-7  1.5e-6 / 1.3e-6  8.2e-7 / 1.7e-3  1e-5 / 2e-2
  channel affine   y, dx            5.1e-8      5e-7      0.61        1 rounding
bf16 whole-discriminator numbers are the bf16 activations' own noise (the kernel-level bf16 checks above are 1e-3 level): a bias
reaches R1 only through the minibatch-stddev curvature, so its R1 gradient alone sits below bf16 resolution (0.07 .. 0.24
relative per bias at the small sizes, 0.4 .. 2.5 at 256^2); the bf16 parameter check is per layer, weight and bias together.
The 256^2 bf16 bounds are 5x the measured error, not 10x (1.0 would check little).
Hand mutations of gan_ops.hip that these tests catch: the svr term and aext of mbstd_bwd_bwd_kernel, the unbiased variance in
mbstd_stat_kernel, a non-zero pad in mbstd_concat_kernel, four waves only in mbstd_bwd_kernel's reduction, relu slope 0.2 in
act_bwd_vec_kernel, `y >= 0` in act_bwd_kernel, no `rlane < rstep` in act_bwd_colsum_kernel, the last maximum winning in
maxpool_kernel, `>=` at the hinge kink of gan_loss_kernel, sign(0) = 1 in l1l2_bwd_kernel.  Skipping the ppb clamp of
vqk_lpips_tap is not caught: it changes the grid only (8450 blocks instead of 7512), not a value.
"""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import vqvae_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import seeded as S  # noqa: E402
from test_gpu_gan import _lpips_tap_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
native = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd._native')
disc = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.modules.loss.discriminator')
DEV, F32, BF, CL = 'cuda:0', torch.float32, torch.bfloat16, torch.channels_last
BF_EPS = 2.0 ** -8
SQ2 = math.sqrt(2.0)

# error bounds per (check, dtype): module docstring
_BOUNDS = {
    ('mbstd.stat', F32): 2e-6, ('mbstd.stat', BF): 1.0,
    ('mbstd.dx', F32): 2e-6, ('mbstd.dx', BF): 1.0,
    ('mbstd.dx_stat', F32): 1e-4, ('mbstd.dx_stat', BF): 2e-2,
    ('mbstd.ddx', F32): 2e-4, ('mbstd.ddx', BF): 5e-2,
    ('mbstd.ddy', F32): 1e-6, ('mbstd.ddy', BF): 1.0,
    ('act.t', F32): 1e-6, ('act.t', BF): 1.0,
    ('act.colsum', F32): 1e-5, ('act.colsum', BF): 1e-5,
    ('conv2.gx', F32): 3e-6, ('conv2.gx', BF): 3e-2,
    ('conv2.dw', F32): 3e-6, ('conv2.dw', BF): 2e-2,
    ('conv2.ddy', F32): 3e-6, ('conv2.ddy', BF): 3e-2,
    ('r1.value', F32): 2e-6, ('r1.value', BF): 7e-2,
    ('r1.gimg', F32): 1e-5, ('r1.gimg', BF): 0.5,
    ('r1.grad', F32): 3e-4, ('r1.layer', F32): 5e-6, ('r1.layer', BF): 0.3,
    ('r1_256.value', F32): 3e-5, ('r1_256.value', BF): 0.1,
    ('r1_256.gimg', F32): 2e-2, ('r1_256.gimg', BF): 0.5, ('r1_256.grad', F32): 1.5e-2,
    ('r1_256.layer', F32): 2e-3, ('r1_256.layer', BF): 0.5,
    ('gan.loss', F32): 2e-6, ('gan.grad', F32): 1e-6,
    ('recon.loss', F32): 5e-6, ('recon.loss', BF): 5e-6,
    ('recon.d', F32): 1e-6, ('recon.d', BF): 1.0,
    ('sumsq.value', F32): 2e-9, ('sumsq.value', BF): 3e-7,
    ('sumsq.d', F32): 4e-7, ('sumsq.d', BF): 1.0,
    ('lpips.value', F32): 1.5e-6, ('lpips.value', BF): 1e-5,
    ('lpips.dfy', F32): 1.3e-6, ('lpips.dfy', BF): 2e-2,
    ('affine.y', F32): 5e-7, ('affine.y', BF): 1.0,
}


def _check(what, dt, err):
    bound = _BOUNDS[(what, dt)]
    print(f'GAN-FORMS {what} {str(dt)[6:]} {err:.3e}')
    assert err < bound, (what, dt, err, bound)


def _rel(got, ref, floor=1e-30):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / max(float(ref.norm()), floor))


def _max(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _ulp(got, ref):
    """bf16 output: the worst element in units of one bf16 rounding of its reference"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / (BF_EPS * (ref.abs() + ref.abs().mean()))).max())


def _elem(dt, got, ref):
    """per-element measure: fp32 max relative to the largest reference element, bf16 in roundings"""
    return _max(got, ref) if dt == F32 else _ulp(got, ref)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _cl(t, dt):
    return t.to(dt).to(DEV).contiguous(memory_format=CL)


def _epc(dt):
    return 4 if dt == F32 else 8


# ---------------------------------------------------------------------------------------------------- minibatch stddev
_MBSTD = [
    # dt, n, c, h, w, group, near-equal groups        hw * c: threads ; cp ; G ; N / G
    (F32, 4, 3, 4, 4, 4, False),                     # 48: 256 ; 4 (pad 0) ; 4 ; 1
    (F32, 8, 4, 4, 4, 4, False),                     # 64: 256 ; 8 (pad 3) ; 4 ; 2
    (F32, 8, 64, 8, 8, 8, False),                    # 4096: 1024 ; 68 ; 8 ; 1
    (F32, 2, 16, 4, 4, 4, False),                    # N < group: G = 2
    (F32, 6, 4, 1, 1, 2, False),                     # 1 x 1 map ; G 2 ; N / G 3
    (F32, 3, 12, 32, 32, 1, False),                  # G = 1 (sd = sqrt(1e-8) everywhere); 12288: 1024, 12 trips
    (F32, 4, 3, 32, 32, 4, False),                   # 3072: 256, 12 trips
    (F32, 8, 1023, 2, 2, 4, False),                  # 4092: 256 just below the switch ; cp 1024 (pad 0)
    (F32, 8, 8, 4, 4, 4, True),                      # nearly equal groups
    (BF, 4, 512, 4, 4, 4, False),                    # 8192: 1024 ; cp 520 (the discriminator epilogue)
    (BF, 8, 7, 4, 4, 4, False),                      # 112: 256 ; cp 8 (pad 0) ; N / G 2
    (BF, 16, 32, 8, 8, 8, False),                    # 2048: 256 ; G 8 ; N / G 2
    (BF, 2, 16, 16, 16, 4, False),                   # 4096 exactly: 1024 ; N < group
    (BF, 6, 8, 1, 1, 2, False),                      # 1 x 1 ; cp 16
    (BF, 8, 16, 4, 4, 4, True),                      # nearly equal groups
]


def _mbstd_data(dt, n, c, h, w, near, seed):
    gen = torch.Generator().manual_seed(seed)
    if near:                                         # the G members of a column differ by ~1e-4: sd ~ sqrt(var + 1e-8) ~ 1e-4
        cols = n // 4
        base = _randn(gen, cols, c, h, w) * 1e-2
        x = base.repeat(4, 1, 1, 1) + 1e-4 * _randn(gen, n, c, h, w)
        x[:, :, 0] = base.repeat(4, 1, 1, 1)[:, :, 0]            # ... and exactly equal along the first row
    else:
        x = _randn(gen, n, c, h, w)
    return x.to(dt)


@pytest.mark.parametrize('case', _MBSTD, ids=lambda c: f'{str(c[0])[6:]}-n{c[1]}c{c[2]}-{c[3]}x{c[4]}-g{c[5]}{"-near" if c[6] else ""}')
def test_mbstd_forward_backward_double_backward(case):
    dt, n, c, h, w, group, near = case
    cp = -(-(c + 1) // _epc(dt)) * _epc(dt)
    x = _mbstd_data(dt, n, c, h, w, near, 100 + n + c + h)
    gen = torch.Generator().manual_seed(7 + c)
    dy = _randn(gen, n, cp, h, w).to(dt)
    v = _randn(gen, n, c, h, w).to(dt)
    xd, dyd = _cl(x, dt).requires_grad_(True), _cl(dy, dt).requires_grad_(True)
    y = ops.MbstdFn.apply(xd, group)
    gx, = torch.autograd.grad(y, xd, dyd, create_graph=True)
    ddx, ddy = torch.autograd.grad(gx, [xd, dyd], _cl(v, dt))

    xr = x.double().requires_grad_(True)
    dyr = dy.double()[:, :c + 1].clone().requires_grad_(True)
    yr = O.mbstd(xr, group)
    gxr, = torch.autograd.grad(yr, xr, dyr, create_graph=True)
    ddxr, ddyr = torch.autograd.grad(gxr, [xr, dyr], v.double())

    y = y.detach().cpu()
    assert y.shape == (n, cp, h, w)
    assert torch.equal(y[:, :c], x)                              # pass-through channels: bit-equal
    assert not y[:, c + 1:].any()                                # zero pad
    _check('mbstd.stat', dt, _elem(dt, y[:, c], yr[:, c]))
    _check('mbstd.dx', dt, _elem(dt, gx, gxr))
    _check('mbstd.ddx', dt, _max(ddx, ddxr) if dt == F32 else _rel(ddx, ddxr))
    _check('mbstd.ddy', dt, _elem(dt, ddy[:, :c + 1], ddyr))
    assert not ddy[:, c + 1:].any()                              # the pad channels of d(dy)
    # the statistic's own gradient, without the pass-through term that hides it at large c * h * w
    dys = dy.clone()
    dys[:, :c] = 0
    gxs, = torch.autograd.grad(ops.MbstdFn.apply(xd, group), xd, _cl(dys, dt))
    gxsr, = torch.autograd.grad(O.mbstd(xr, group), xr, dys.double()[:, :c + 1])
    _check('mbstd.dx_stat', dt, _rel(gxs, gxsr, floor=1e-300) if dt == BF else _max(gxs, gxsr))


def test_mbstd_group_over_8_raises():
    """the kernels hold at most 8 group members in registers: group_size=None with N > 8 (and G = 16 explicitly) is an error,
    not a wrong value; N not a multiple of G is one too (the reference's reshape fails)"""
    x = _cl(torch.randn(16, 8, 4, 4), F32)
    with pytest.raises(RuntimeError):
        disc.MinibatchStdLayer(None)(x)
    with pytest.raises(RuntimeError):
        ops.MbstdFn.apply(x, 16)
    with pytest.raises(RuntimeError):
        ops.MbstdFn.apply(_cl(torch.randn(6, 8, 4, 4), F32), 4)
    y = disc.MinibatchStdLayer(None)(x[:8])                      # N = 8 = G: served
    assert torch.allclose(y[:, 8].double().cpu(), O.mbstd(x[:8].double().cpu(), None)[:, 8], rtol=1e-5, atol=0)


@pytest.mark.parametrize('dt', [F32, BF])
def test_mbstd_halves(dt):
    """real | fake in one pass (halves = 2): each half is grouped on its own, exactly as two separate calls"""
    gen = torch.Generator().manual_seed(21)
    cp = -(-9 // _epc(dt)) * _epc(dt)
    x = _randn(gen, 16, 8, 4, 4).to(dt)
    dy = _randn(gen, 16, cp, 4, 4).to(dt)
    xd = _cl(x, dt).requires_grad_(True)
    y = disc.MinibatchStdLayer(4)(xd, halves=2)
    gx, = torch.autograd.grad(y, xd, _cl(dy, dt))
    xr = x.double().requires_grad_(True)
    yr = torch.cat([O.mbstd(h, 4) for h in xr.chunk(2, 0)], 0)
    gxr, = torch.autograd.grad(yr, xr, dy.double()[:, :9])
    whole = O.mbstd(x.double(), 4)[:, 8]
    assert (whole - yr[:, 8]).abs().max() > 1e-2                 # (grouping across the halves would be visible)
    _check('mbstd.stat', dt, _elem(dt, y[:, 8], yr[:, 8]))
    _check('mbstd.dx', dt, _elem(dt, gx, gxr))


# ---------------------------------------------------------------------------------------------------- activation backward
def _slope(y, act):
    """bias_act.py:197-198 restated on the saved output: linear 1, tanh 1 - y^2, relu / lrelu by the sign of y (y == 0: the
    negative side)"""
    if act == 0:
        return torch.ones_like(y)
    if act == 1:
        return 1.0 - y * y
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.0 if act == 2 else 0.2))


def _act_data(dt, shape, act, seed):
    gen = torch.Generator().manual_seed(seed)
    dy = _randn(gen, *shape)
    y = _randn(gen, *shape)
    if act == 1:
        y = torch.tanh(y)
    y.view(-1)[::5] = 0.0                                        # exactly zero: the kernel's `y > 0` decides the slope
    y.view(-1)[1::10] = -0.0
    return dy.to(dt), y.to(dt)


_ACT = [
    # dt, (n, c, h, w), form
    (F32, (2, 8, 4, 4), 'vec'), (BF, (2, 8, 4, 4), 'vec'),
    (F32, (1, 3, 5, 7), 'scalar'), (BF, (1, 3, 5, 7), 'scalar'),             # 105 elements: not a whole number of vectors
    (BF, (1, 4, 3, 3), 'scalar'),                                           # 36: a multiple of 4, not of 8
    (F32, (3, 16, 33, 31), 'vec'), (BF, (3, 16, 33, 31), 'vec'),
]


@pytest.mark.parametrize('act', [0, 1, 2, 3])
@pytest.mark.parametrize('case', _ACT, ids=lambda c: f'{str(c[0])[6:]}-{"x".join(map(str, c[1]))}-{c[2]}')
def test_act_backward_plain(case, act):
    dt, shape, form = case
    n = int(np.prod(shape))
    assert (n % _epc(dt) == 0) == (form == 'vec')
    dy, y = _act_data(dt, shape, act, 3 + act)
    scale = 0.7 * SQ2
    dyd = _cl(dy, dt).requires_grad_(True)
    yd = _cl(y, dt)
    t = ops.ActBwdFn.apply(dyd, yd, act, scale)
    ref = dy.double() * scale * _slope(y.double(), act)
    _check('act.t', dt, _elem(dt, t, ref))
    v = _cl(torch.randn(shape, generator=torch.Generator().manual_seed(9)), dt)
    if act == 1:
        with pytest.raises(NotImplementedError):
            torch.autograd.grad(t, dyd, v)
        return
    g, = torch.autograd.grad(t, dyd, v)                          # the double backward: the same op on the cotangent
    assert torch.equal(g, ops.ActBwdFn.apply(v, yd, act, scale))
    _check('act.t', dt, _elem(dt, g, v.double().cpu() * scale * _slope(y.double(), act)))


@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('act', [2, 3])
def test_act_backward_misaligned_pointers(dt, act):
    """the scalar form entered by alignment: whole vectors, but every pointer one element past a 16-byte boundary"""
    n = 64 * 37
    dy, y = _act_data(dt, (n + 1,), act, 5)
    dyd, yd = dy.to(DEV), y.to(DEV)
    out = torch.full((n + 1,), 7.0, dtype=dt, device=DEV)
    es = dyd.element_size()
    assert dyd.data_ptr() % 16 == 0 and (dyd.data_ptr() + es) % 16 != 0
    native.check(native.lib().vqk_act_backward(ops.dcode(dt), dyd.data_ptr() + es, yd.data_ptr() + es, out.data_ptr() + es, n,
                                               act, 1.25, ops._stream()), 'act_backward')
    out = out.cpu()
    assert out[0] == 7.0                                         # nothing written before the range
    _check('act.t', dt, _elem(dt, out[1:], dy[1:].double() * 1.25 * _slope(y[1:].double(), act)))


_COLSUM = [
    # dt, (n, c, h, w), served: c % v == 0 and c / v <= 256 ; slots c / v
    (F32, (1, 1024, 4, 4), True),                    # 256 slots, one block of 16 rows
    (F32, (1, 1028, 4, 4), False),                   # 257
    (BF, (1, 2048, 4, 4), True),                     # 256
    (BF, (1, 2056, 4, 4), False),                    # 257
    (F32, (2, 192, 5, 7), True),                     # 48 slots: rstep 5, lanes 240..255 idle
    (BF, (2, 1280, 5, 7), True),                     # 160 slots: rstep 1, lanes 160..255 idle
    (F32, (1, 8, 359, 367), True),                   # 131753 rows > 2048 x 64: 65 rows per block
    (BF, (1, 16, 359, 367), True),
    (F32, (2, 12, 3, 3), True),                      # 3 slots: rstep 85, one block, 18 rows
]


@pytest.mark.parametrize('act', [0, 2, 3])
@pytest.mark.parametrize('case', _COLSUM, ids=lambda c: f'{str(c[0])[6:]}-{"x".join(map(str, c[1]))}')
def test_act_backward_colsum(case, act):
    """act_bwd_colsum_kernel: t as the plain form computes it, and colsum += colsum_scale * (the float64 column sums of t AS
    STORED) onto a non-zero buffer; where the guard refuses, ActBwdFn takes the plain form and leaves the buffer alone (the
    caller sums the columns itself: _conv_act_backward)"""
    dt, shape, served = case
    n, c, h, w = shape
    v = _epc(dt)
    assert (c % v == 0 and c // v <= 256) == served
    dy, y = _act_data(dt, shape, act, 11 + c)
    scale, cs_scale = 0.7 * SQ2, 0.37
    pre = torch.randn(c, generator=torch.Generator().manual_seed(c)).to(DEV)
    cs = pre.clone()
    dyd, yd = _cl(dy, dt), _cl(y, dt)
    t = ops.ActBwdFn.apply(dyd, yd, act, scale, cs, cs_scale)
    ref = dy.double() * scale * _slope(y.double(), act)
    _check('act.t', dt, _elem(dt, t, ref))
    if not served:
        assert torch.equal(cs, pre)
        st = native.lib().vqk_act_backward_colsum_scaled(ops.dcode(dt), dyd.data_ptr(), yd.data_ptr(), t.data_ptr(), n * h * w, c,
                                                         act, scale, cs_scale, cs.data_ptr(), ops._stream())
        assert st == native.ERR_SHAPE
        return
    want = t.detach().double().cpu().sum((0, 2, 3)) * cs_scale
    _check('act.colsum', dt, _rel(cs.double().cpu() - pre.double().cpu(), want))
    assert torch.equal(t, ops.ActBwdFn.apply(dyd, yd, act, scale))          # same values as the plain form


# ---------------------------------------------------------------------------------------------------- conv + bias + lrelu, twice
_CONV2 = [
    # dt, n, cin, cout, h, k, stride, pad, s2 served (vqk_conv2d_s2_supported, backward=0)
    (F32, 2, 32, 32, 8, 3, 1, 1, False),
    (BF, 2, 32, 32, 8, 3, 1, 1, False),
    (F32, 2, 32, 64, 9, 3, 2, 0, False),
    (BF, 2, 128, 128, 65, 3, 2, 0, True),            # 32 x 32 out: matrix forms (also the stride-2 dgrad phases)
    (BF, 2, 64, 128, 33, 3, 2, 0, True),             # forward form served, dgrad phases not
    (BF, 2, 128, 128, 17, 3, 2, 0, False),           # 8 x 8 out: the tile-width check refuses
    (BF, 2, 32, 64, 17, 3, 2, 0, False),             # cin % 64
    (F32, 4, 64, 32, 1, 1, 1, 0, False),             # fully connected: 1x1 on 1 x 1
    (BF, 4, 64, 32, 1, 1, 1, 0, False),
    (F32, 2, 3, 32, 16, 1, 1, 0, False),             # fromrgb (image padded to 4 channels)
    (BF, 2, 3, 32, 32, 1, 1, 0, False),              # fromrgb (padded to 8: the centre-tap 3x3 form)
]


@pytest.mark.parametrize('case', _CONV2, ids=lambda c: f'{str(c[0])[6:]}-n{c[1]}-{c[2]}to{c[3]}-{c[4]}-k{c[5]}s{c[6]}')
def test_conv_act_double_backward(case):
    """gx = d y / d x . dy (create_graph), then d<v, gx> / d(x, w, b, dy) against float64 F.conv2d autograd; the lrelu slope
    comes from the sign of the stored output (bias_act.py:182-198), so x and b receive nothing"""
    dt, n, cin, cout, h, k, stride, pad, served = case
    e = _epc(dt)
    cin_p = -(-cin // e) * e
    cout_p = -(-cout // e) * e
    h_out = (h + 2 * pad - k) // stride + 1
    assert ops._s2_served(dt, dt, n, h, h, h_out, h_out, cin_p, cout_p, k, stride, pad, False) == served
    gen = torch.Generator().manual_seed(cin + cout + h)
    x = torch.zeros(n, cin_p, h, h)
    x[:, :cin] = _randn(gen, n, cin, h, h)
    x = x.to(dt)
    w = _randn(gen, cout, cin, k, k).to(dt).float()
    b = _randn(gen, cout) * 0.5
    dy = torch.zeros(n, cout_p, h_out, h_out)
    dy[:, :cout] = _randn(gen, n, cout, h_out, h_out)
    dy = dy.to(dt)
    v = _randn(gen, n, cin_p, h, h).to(dt)
    wgain, gain = 1.0 / math.sqrt(cin * k * k), SQ2 * 0.75

    xd = _cl(x, dt).requires_grad_(True)
    wd = w.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True)
    dyd = _cl(dy, dt).requires_grad_(True)
    y = ops.conv_act(xd, wd, bd, k=k, stride=stride, pad=pad, act='lrelu', wgain=wgain, out_gain=gain)
    assert y.shape[1] == cout_p
    gx, = torch.autograd.grad(y, xd, dyd, create_graph=True)
    gd = torch.autograd.grad(gx, [xd, wd, bd, dyd], _cl(v, dt), allow_unused=True)

    xr = x.double()[:, :cin].requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    dyr = dy.double()[:, :cout].requires_grad_(True)
    lin = Fn.conv2d(xr, wr * wgain, br, stride=stride, padding=pad)
    yc = y.detach().double().cpu()[:, :cout]
    assert int(((lin.detach() > 0) != (yc > 0)).sum()) <= (0 if dt == F32 else 1e-3 * yc.numel())
    ref = lin * torch.where(yc > 0, torch.ones_like(yc), torch.full_like(yc, 0.2)) * gain
    gxr, = torch.autograd.grad(ref, xr, dyr, create_graph=True)
    gr = torch.autograd.grad(gxr, [xr, wr, br, dyr], v.double()[:, :cin], allow_unused=True)

    _check('conv2.gx', dt, _rel(gx[:, :cin], gxr))
    assert not gx[:, cin:].any()
    for got in (gd[0], gd[2]):                                   # piecewise-linear activation: no second-order term
        assert got is None or not got.any()
    assert gr[0] is None or not gr[0].any()
    _check('conv2.dw', dt, _rel(gd[1], gr[1]))
    _check('conv2.ddy', dt, _rel(gd[3][:, :cout], gr[3]))


# ---------------------------------------------------------------------------------------------------- whole-discriminator R1
def _disc_r1_case(d, x, dt, round_weights):
    """R1 of ``d`` on x in compute dtype ``dt`` against oracle.r1_penalty in float64 on the same (rounded) weights"""
    if round_weights:
        with torch.no_grad():
            for name, p in d.named_parameters():
                if name.endswith('weight'):
                    p.copy_(p.to(dt).float())
    p64 = {k: v.detach().double().clone() for k, v in d.state_dict().items()}
    names = [n for n, _ in d.named_parameters()]
    for nm in names:
        p64[nm].requires_grad_(True)
    r1r, _, gimgr = O.r1_penalty(x.double(), p64)
    grs = torch.autograd.grad(r1r, [p64[nm] for nm in names], allow_unused=True)

    d.compute_dtype = dt
    d = d.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    logits = d(xd, double_backward=True)
    gimg, = torch.autograd.grad(logits.sum(), xd, create_graph=True)
    r1 = 10.0 * ops.SumSqFn.apply(gimg) / gimg.shape[0]
    grads = torch.autograd.grad(r1, [p for _, p in d.named_parameters()], allow_unused=True)
    _check('r1.value', dt, abs(r1.item() - r1r.item()) / abs(r1r.item()))
    _check('r1.gimg', dt, _rel(gimg, gimgr))
    layers = {}
    for nm, got, want in zip(names, grads, grs):
        if want is None or not want.any():                       # float64 gradient identically zero (or not on the path)
            assert got is None or not got.any(), nm
            continue
        assert got is not None, nm
        if dt == F32:
            _check('r1.grad', dt, _rel(got, want))
        err2, ref2 = layers.get(nm.rsplit('.', 1)[0], (0.0, 0.0))
        layers[nm.rsplit('.', 1)[0]] = (err2 + float((got.double().cpu() - want).norm()) ** 2, ref2 + float(want.norm()) ** 2)
    # per layer (weight and bias together): a bias reaches R1 only through the minibatch-stddev curvature, a signal far
    # below bf16 resolution on its own (measured 0.07 .. 0.24 relative per bias in bf16, 3e-5 in fp32)
    for name, (err2, ref2) in layers.items():
        _check('r1.layer', dt, (err2 / ref2) ** 0.5)


@pytest.mark.parametrize('dt', [F32, BF])
def test_discriminator_r1_golden_size_vs_float64(golden, dt):
    g = golden('gan')
    d = disc.Discriminator(32, channel_base=1024, channel_max=64)
    d.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith('d.')})
    x = torch.from_numpy(g['d_in.x']).to(dt).float()
    _disc_r1_case(d, x, dt, dt == BF)


@pytest.mark.parametrize('dt', [F32, BF])
def test_discriminator_r1_512_channels_vs_float64(dt):
    """Discriminator(16) at the default channel_max: 512-channel blocks, the epilogue's 4 x 4 x 512 minibatch stddev on the
    1024-thread form and its 513 -> padded channel conv; N = 8: two group columns"""
    torch.manual_seed(5)
    d = disc.Discriminator(16)
    S.fill_named(list(d.named_parameters()), 505, 'discriminator')
    x = (torch.randn(8, 3, 16, 16, generator=torch.Generator().manual_seed(6)) * 0.5).to(dt).float()
    _disc_r1_case(d, x, dt, dt == BF)


@pytest.mark.parametrize('dt', [F32, BF])
def test_discriminator_256_r1_vs_reference(golden, dt):
    """Discriminator(256) (28.9 M parameters) R1 in fp32 and bf16 against what the reference computed in fp32
    (full_disc256.npz: value, image-gradient and parameter-gradient summaries)"""
    g = golden('full_disc256')
    i = S.disc256_inputs()
    d = disc.Discriminator(256)
    S.fill_named(list(d.named_parameters()), i['seed'], 'discriminator')
    d.compute_dtype = dt
    d = d.to(DEV)
    x = i['x'].to(DEV).requires_grad_(True)
    logits = d(x, double_backward=True)
    gimg, = torch.autograd.grad(logits.sum(), x, create_graph=True)
    r1 = 10.0 * ops.SumSqFn.apply(gimg) / gimg.shape[0]
    _check('r1_256.value', dt, abs(r1.item() - float(g['r1.value'])) / abs(float(g['r1.value'])))
    _check('r1_256.gimg', dt, _summary_err(gimg, g['r1.gimg_sum'], 'd256.gimg'))
    named = [(n, p) for n, p in d.named_parameters() if 'r1g.' + n in g]
    grads = torch.autograd.grad(r1, [p for _, p in named], allow_unused=True)
    layers = {}
    for (n, _), gr in zip(named, grads):
        ref = g['r1g.' + n]
        if not ref[1]:                                           # zero in the reference (after the minibatch stddev)
            assert gr is None or not gr.any(), n
            continue
        assert gr is not None, n
        if dt == F32:
            _check('r1_256.grad', dt, _summary_err(gr, ref, 'd256.r1g.' + n))
        err2, ref2 = layers.get(n.rsplit('.', 1)[0], (0.0, 0.0))
        layers[n.rsplit('.', 1)[0]] = (err2 + (_summary_err(gr, ref, 'd256.r1g.' + n) * ref[1]) ** 2, ref2 + ref[1] ** 2)
    for name, (err2, ref2) in layers.items():
        _check('r1_256.layer', dt, (err2 / ref2) ** 0.5)


def _summary_err(t, ref, name):
    """seeded.check_summary's measure: the worst projection error relative to the reference norm (a projection onto a unit
    variance direction has the error's norm as its standard deviation), and the error of the norm itself"""
    got = S.summary(t, name)
    norm = max(float(ref[1]), 1e-30)
    return max(float(np.abs(got[2:] - ref[2:]).max()) / norm, abs(got[1] - ref[1]) / norm)


# ---------------------------------------------------------------------------------------------------- losses
def _gan_ref(lr, lf, mode, which):
    """loss.py:11-51 in float64: hinge / non-saturating (BCE with logits == softplus), generator / discriminator"""
    if which == 0:
        return -lf.mean() if mode == 0 else Fn.softplus(-lf).mean()
    if mode == 0:
        return (Fn.relu(1.0 - lr) + Fn.relu(1.0 + lf)).mean()
    return (Fn.softplus(-lr) + Fn.softplus(lf)).mean()


@pytest.mark.parametrize('n', [1, 8, 255, 256, 257, 1000])
@pytest.mark.parametrize('mode', [0, 1], ids=['hinge', 'nonsat'])
@pytest.mark.parametrize('which', [0, 1], ids=['gen', 'disc'])
def test_gan_loss(n, mode, which):
    gen = torch.Generator().manual_seed(n + 10 * mode + 100 * which)
    lr, lf = _randn(gen, n, 1) * 3, _randn(gen, n, 1) * 3
    lr.view(-1)[1::7], lf.view(-1)[2::7] = 40.0, -40.0
    lr.view(-1)[3::7], lf.view(-1)[4::7] = -40.0, 40.0
    lr.view(-1)[::5], lf.view(-1)[::6] = 1.0, -1.0                 # at the hinge kinks: relu'(0) = 0, as torch
    if n == 1:
        lr[0], lf[0] = 1.0, -1.0
    up = 3.5
    ard, afd = lr.to(DEV).requires_grad_(True), lf.to(DEV).requires_grad_(True)
    loss = ops.GanLossFn.apply(ard if which else None, afd, mode, which)
    grads = torch.autograd.grad(loss * up, [ard, afd] if which else [afd])
    lrr, lfr = lr.double().requires_grad_(True), lf.double().requires_grad_(True)
    ref = _gan_ref(lrr, lfr, mode, which)
    refg = torch.autograd.grad(ref * up, [lrr, lfr] if which else [lfr])
    _check('gan.loss', F32, abs(loss.item() - ref.item()) / max(abs(ref.item()), 1e-30))
    for got, want in zip(grads, refg):
        _check('gan.grad', F32, float((got.double().cpu() - want).abs().max()) / (up / n))


@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('shape', [(2, 3, 37, 41), (2, 3, 1024, 700)], ids=['ragged', 'over-2^22'])
@pytest.mark.parametrize('weights', [(0.8, 0.3), (1.7, None)], ids=['l1+l2', 'l1-only'])
def test_recon_loss(dt, shape, weights):
    """ReconLossFn: (mean |t - r|, mean (t - r)^2) over the element count (l1_sum / sse, atomics across blocks), the gradient
    (l1l2_bwd twice: the second pass accumulates); recon == target exactly at a sixth of the elements, where the L1 gradient is
    sign(0) = 0 as torch's"""
    gen = torch.Generator().manual_seed(shape[2])
    r = _randn(gen, *shape).to(dt)
    t = _randn(gen, *shape)
    t.view(-1)[::6] = r.float().view(-1)[::6]
    numel = r.numel()
    assert numel % 2048 != 0 or numel >= 1 << 22
    rd = _cl(r, dt).requires_grad_(True)
    l1, l2 = ops.ReconLossFn.apply(rd, _cl(t, F32), float(numel))
    w1, w2 = weights
    loss = w1 * l1 + (w2 * l2 if w2 is not None else 0.0)
    dr, = torch.autograd.grad(loss, rd)
    rr = r.to(DEV).double().requires_grad_(True)
    td = t.to(DEV).double()
    l1r, l2r = (td - rr).abs().sum() / numel, (td - rr).pow(2).sum() / numel
    lossr = w1 * l1r + (w2 * l2r if w2 is not None else 0.0)
    drr, = torch.autograd.grad(lossr, rr)
    _check('recon.loss', dt, abs(l1.item() - l1r.item()) / l1r.item())
    _check('recon.loss', dt, abs(l2.item() - l2r.item()) / l2r.item())
    _check('recon.d', dt, _elem(dt, dr, drr))
    if w2 is None:                                               # only the L1 term: zero gradient where recon == target
        assert not dr.cpu()[r.float() == t].any()


@pytest.mark.parametrize('dt', [F32, BF])
def test_sumsq(dt):
    """SumSqFn (the R1 sum, loss.py:108) on a channels-last input: value and 2 g * upstream"""
    gen = torch.Generator().manual_seed(3)
    g = _randn(gen, 3, 8, 9, 7).to(dt)
    gd = _cl(g, dt).requires_grad_(True)
    s = ops.SumSqFn.apply(gd)
    d, = torch.autograd.grad(s * 0.37, gd)
    ref = g.double().pow(2).sum()
    _check('sumsq.value', dt, abs(s.item() - ref.item()) / ref.item())
    _check('sumsq.d', dt, _elem(dt, d, 2 * 0.37 * g.double()))


@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('hw', [64, 40])
def test_lpips_five_taps(dt, hw):
    """LpipsTapsFn as LPIPS.forward calls it: five taps of 64, 128, 256, 512, 512 channels with the map halving each time; in fp32
    the 512-channel taps have 128 lanes per pixel and take the scalar kernels in the same call; fx receives no gradient"""
    gen = torch.Generator().manual_seed(hw)
    chans = (64, 128, 256, 512, 512)
    fxs = [_randn(gen, 3, c, hw >> i, hw >> i).relu().to(dt) for i, c in enumerate(chans)]
    fys = [_randn(gen, 3, c, hw >> i, hw >> i).relu().to(dt) for i, c in enumerate(chans)]
    lins = [torch.rand(c, generator=gen) for c in chans]
    up = _randn(gen, 3)
    fxd = [_cl(t, dt).requires_grad_(True) for t in fxs]
    fyd = [_cl(t, dt).requires_grad_(True) for t in fys]
    out = ops.LpipsTapsFn.apply(5, *fxd, *fyd, *[l.to(DEV) for l in lins])
    (out * up.to(DEV)).sum().backward()
    fyr = [t.double().requires_grad_(True) for t in fys]
    ref = sum(_lpips_tap_ref(a.double(), b, l) for a, b, l in zip(fxs, fyr, lins))
    (ref * up.double()).sum().backward()
    _check('lpips.value', dt, _max(out, ref))
    for a, b in zip(fyd, fyr):
        _check('lpips.dfy', dt, _rel(a.grad, b.grad))
    assert all(t.grad is None for t in fxd)


def test_lpips_tap_ppb_clamp():
    """bf16, 512 channels (64 lanes per pixel, 4 pixels per block pass): 270400 pixels would take 8450 blocks of 32 pixels; the
    launcher clamps the grid to 8192 blocks by giving each block a larger whole number of passes (36 pixels)"""
    dt, npix, c = BF, 520 * 520, 512
    per_pass = 4 * (64 // (c // 8))
    assert -(-npix // (8 * per_pass)) > 8192                   # (vqk_lpips_tap: blocks before the clamp)
    gen = torch.Generator(device=DEV).manual_seed(1)
    fx = torch.randn(1, 512, 520, 520, device=DEV, generator=gen).relu().to(dt).contiguous(memory_format=CL)
    fy = torch.randn(1, 512, 520, 520, device=DEV, generator=gen).relu().to(dt).contiguous(memory_format=CL)
    lin = torch.rand(512, device=DEV, generator=gen)
    fyd = fy.clone().requires_grad_(True)
    out = ops.LpipsTapsFn.apply(1, fx, fyd, lin)
    out.backward(torch.full_like(out, 1.3))
    fyr = fy.double().requires_grad_(True)
    ref = _lpips_tap_ref(fx, fyr, lin)
    ref.backward(torch.full_like(ref, 1.3))
    _check('lpips.value', dt, _max(out, ref))
    _check('lpips.dfy', dt, _rel(fyd.grad, fyr.grad))


@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('c', [8, 64])
def test_maxpool_ties(dt, c):
    """MaxPool2x2Fn against float64 F.max_pool2d and its backward: ReLU zeros and duplicated values make ties; the gradient goes
    to the FIRST maximum of the window in row-major order, as torch routes it"""
    gen = torch.Generator().manual_seed(c)
    x = _randn(gen, 2, c, 6, 10).relu()
    x[:, :, 2:4, 1::2] = x[:, :, 2:4, 0::2]                       # equal horizontal pairs
    x[:, :, 1::2, 4:] = x[:, :, 0::2, 4:]                        # equal vertical pairs
    x[:, : c // 2, 4:6, 6:8] = 0.5                               # whole windows equal
    x = x.to(dt)
    dy = _randn(gen, 2, c, 3, 5).to(dt)
    xd = _cl(x, dt).requires_grad_(True)
    y = ops.MaxPool2x2Fn.apply(xd)
    dx, = torch.autograd.grad(y, xd, _cl(dy, dt))
    xr = x.double().requires_grad_(True)
    yr = Fn.max_pool2d(xr, 2, 2)
    dxr, = torch.autograd.grad(yr, xr, dy.double())
    assert torch.equal(y.detach().double().cpu(), yr.detach())
    assert torch.equal(dx.double().cpu(), dxr)


def test_maxpool_odd_map_raises():
    """vqk_maxpool2x2 rejects odd maps (torch floors); the discriminator / LPIPS resolutions never meet one"""
    with pytest.raises(RuntimeError):
        ops.MaxPool2x2Fn.apply(_cl(torch.randn(1, 8, 5, 6), F32))
    with pytest.raises(RuntimeError):
        ops.MaxPool2x2Fn.apply(_cl(torch.randn(1, 8, 6, 7), BF))


@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('shift', [True, False])
def test_channel_affine(dt, shift):
    """ChannelAffineFn (the LPIPS z-score): y = x * scale[c] + shift[c] in one fma, dx = dy * scale[c]"""
    gen = torch.Generator().manual_seed(2)
    x = _randn(gen, 2, 3, 7, 9).to(dt)
    scale, sh = torch.rand(3, generator=gen) + 0.5, _randn(gen, 3)
    dy = _randn(gen, 2, 3, 7, 9).to(dt)
    xd = _cl(x, dt).requires_grad_(True)
    y = ops.ChannelAffineFn.apply(xd, scale.to(DEV), sh.to(DEV) if shift else None)
    dx, = torch.autograd.grad(y, xd, _cl(dy, dt))
    yr = x.double() * scale.double().view(1, -1, 1, 1) + (sh.double().view(1, -1, 1, 1) if shift else 0.0)
    _check('affine.y', dt, _elem(dt, y, yr))
    _check('affine.y', dt, _elem(dt, dx, dy.double() * scale.double().view(1, -1, 1, 1)))
