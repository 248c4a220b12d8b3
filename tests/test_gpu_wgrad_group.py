"""The grouped 3x3 weight-gradient launch (include/vqk.h: vqk_conv3x3_wgrad_group; csrc/conv_wgmx.hip:
conv3x3_wgrad_mx_group_kernel) and the deferral that feeds it (ops.defer_wgrad / ops.flush_wgrads).

Kernel level: every item's dW against float64 ``F.conv2d`` on the bf16-exact operands plus a random pre-filled target (dW
ACCUMULATES), max|err| / max|ref| < 1e-5 -- the bound tests/test_gpu_conv_x3.py holds the one-layer bf16 kernel to -- and against
the one-layer launch on the same operands, relative Frobenius error < 2e-6 -- what tests/test_gpu_deterministic.py allows between
two orders of the same fp32 sum.  Both final passes are pinned through the launcher's own partition: a one-tile item has to be
split over K (fp32 atomics), a many-tile group must not be (plain adds: the same bits on every run).
Autograd level: two ResBlocks with arena targets, deferral on against off, eager and under graph capture + replay."""
import functools
import importlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
ae = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.modules.autoencoder')
native = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd._native')
DEV, BF, CL = 'cuda:0', torch.bfloat16, torch.channels_last
TOL_FP64, TOL_ORDER = 1e-5, 2e-6


@functools.lru_cache(maxsize=None)
def problem(n, cin, cout, h, w, seed=0):
    """(x, dy, pre, ref): bf16 nhwc operands, the random fp32 target [Cout][3][3][Cin] and float64 pre + wgrad(x, dy); built once
    per shape and shared by the tests (none of them writes to it: targets are cloned)"""
    g = torch.Generator(device=DEV).manual_seed(1000 * seed + cin + 2 * cout + 3 * h + 5 * w + n)
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).to(BF).contiguous(memory_format=CL)
    dy = torch.randn(n, cout, h, w, device=DEV, generator=g).to(BF).contiguous(memory_format=CL)
    pre = torch.randn(cout, 3, 3, cin, device=DEV, generator=g).permute(0, 3, 1, 2)
    wd = torch.zeros(cout, cin, 3, 3, device=DEV, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x.double(), wd, None, padding=1) * dy.double()).sum().backward()
    return x, dy, pre, wd.grad + pre.double()


def target(pre):
    t = pre.clone(memory_format=torch.preserve_format)
    assert t.permute(0, 2, 3, 1).is_contiguous()
    return t


def run_group(shapes):
    probs = [problem(*s) for s in shapes]
    tgts = [target(p[2]) for p in probs]
    status, splits, launches = ops.raw_conv_wgrad_group([(p[0], p[1], t) for p, t in zip(probs, tgts)])
    torch.cuda.synchronize()
    assert status == 0, status
    return probs, tgts, splits, launches


def max_err(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


def fro_err(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


MIXED = [(2, 64, 64, 8, 16), (1, 128, 64, 16, 16), (3, 64, 128, 16, 32), (2, 128, 128, 32, 32)]


def test_mixed_group_matches_fp64():
    probs, tgts, splits, launches = run_group(MIXED)
    assert launches == 1
    for s, p, t, k in zip(MIXED, probs, tgts, splits):
        e = max_err(t, p[3])
        print(s, 'splits', k, f'max err {e:.3e}')
        assert e < TOL_FP64, (s, e)


@pytest.mark.parametrize('shape', [(2, 64, 128, 8, 16), (2, 64, 64, 8, 32), (2, 128, 64, 24, 16)], ids=['8x16', '8x32', '24x16'])
def test_border_patches(shape):
    """8x16: the one patch of an image touches all four borders; 8x32 / 24x16: patches with a left or right / top or bottom border
    only and, at 24 rows, one with neither top nor bottom"""
    probs, tgts, _, _ = run_group([shape])
    e = max_err(tgts[0], probs[0][3])
    print(shape, f'max err {e:.3e}')
    assert e < TOL_FP64, e


def test_split_and_unsplit_final_pass():
    # one dW tile, 32 patches: alone in a launch it has to be split over K (the atomic final pass)
    one = [(4, 64, 64, 32, 32)]
    probs, tgts, splits, _ = run_group(one)
    assert splits[0] > 1, splits
    assert max_err(tgts[0], probs[0][3]) < TOL_FP64
    # 256 dW tiles of equal length: one block per tile over the whole K (the plain-add final pass), the same bits every run
    many = [(2, 512, 512, 16, 16, seed) for seed in range(4)]
    probs, tgts, splits, launches = run_group(many)
    assert splits == [1, 1, 1, 1] and launches == 1, (splits, launches)
    for p, t in zip(probs, tgts):
        assert max_err(t, p[3]) < TOL_FP64
    _, again, splits2, _ = run_group(many)
    assert splits2 == splits
    for a, b in zip(tgts, again):
        assert torch.equal(a, b)


def test_group_matches_per_layer_launch():
    probs, tgts, _, _ = run_group(MIXED)
    for s, p, t in zip(MIXED, probs, tgts):
        single = ops.raw_conv_wgrad(p[0], p[1], 3, False, out=target(p[2]))
        torch.cuda.synchronize()
        e = fro_err(t, single)
        print(s, f'grouped vs per-layer {e:.3e}')
        assert e < TOL_ORDER, (s, e)


def test_seventeen_items_take_two_launches():
    shapes = [(1, 64, 64, 8, 16, seed) for seed in range(17)]
    probs, tgts, splits, launches = run_group(shapes)
    assert launches == 2 and len(splits) == 17
    for p, t in zip(probs, tgts):
        assert max_err(t, p[3]) < TOL_FP64


@pytest.mark.parametrize('bad', ['w8', 'cin32', 'fp32'])
def test_refused_item_refuses_the_whole_call(bad):
    good = problem(1, 64, 64, 8, 16)
    g = torch.Generator(device=DEV).manual_seed(3)
    n, cin, cout, h, w, dt = {'w8': (1, 64, 64, 8, 8, BF), 'cin32': (1, 32, 64, 8, 16, BF), 'fp32': (1, 64, 64, 8, 16, torch.float32)}[bad]
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).to(dt).contiguous(memory_format=CL)
    dy = torch.randn(n, cout, h, w, device=DEV, generator=g).to(dt).contiguous(memory_format=CL)
    pre = torch.randn(cout, 3, 3, cin, device=DEV, generator=g).permute(0, 3, 1, 2)
    t_good, t_bad = target(good[2]), target(pre)
    status, _, _ = ops.raw_conv_wgrad_group([(good[0], good[1], t_good), (x, dy, t_bad)])
    torch.cuda.synchronize()
    assert status == native.ERR_SHAPE
    assert torch.equal(t_good, good[2]) and torch.equal(t_bad, pre)          # nothing was launched


# ---------------------------------------------------------------- autograd level
def mark_direct(blk):
    """what FlatAdamW does to its parameters (tests/test_gpu_resblock_schedule.py): zeroed arena-style gradients the kernels add to"""
    for p in blk.parameters():
        if p.dim() == 4:
            o, i, kh, kw = p.shape
            p.grad = torch.zeros(o, kh, kw, i, device=p.device).permute(0, 3, 1, 2)
        else:
            p.grad = torch.zeros_like(p)
        p._vqk_direct_grad = True


@pytest.fixture(scope='module')
def blocks():
    torch.manual_seed(11)
    blks = [ae.ResBlock(64, 64).to(DEV) for _ in range(2)]
    with torch.no_grad():
        for b in blks:
            b.norm1.weight.normal_(1.0, 0.2); b.norm1.bias.normal_(0.0, 0.2)
            b.norm2.weight.normal_(1.0, 0.2); b.norm2.bias.normal_(0.0, 0.2)
            for p in b.parameters():
                p.copy_(p.to(BF).float())
            mark_direct(b)
    x0 = torch.randn(2, 64, 16, 16, device=DEV).to(BF).contiguous(memory_format=CL)
    dy = torch.randn(2, 64, 16, 16, device=DEV).to(BF).contiguous(memory_format=CL)
    return blks, x0, dy


def step(blks, x0, dy):
    """zero the arena views, forward, backward; returns (x, parameters): gradients are read after a synchronize / replay"""
    params = [p for b in blks for p in b.parameters()]
    for p in params:
        p.grad.zero_()
    x = x0.clone().requires_grad_(True)
    y = x
    for b in blks:
        y = b(y)
    y.backward(dy)
    return x, params


def grads(x, params):
    torch.cuda.synchronize()
    return [x.grad.float().clone()] + [p.grad.float().clone() for p in params]


def counted_defer(monkeypatch):
    calls = []
    real = ops.defer_wgrad
    monkeypatch.setattr(ops, 'defer_wgrad', lambda *a: (calls.append(1), real(*a))[1])
    return calls


def test_autograd_deferred_matches_per_layer(blocks, monkeypatch):
    blks, x0, dy = blocks
    monkeypatch.setattr(ops, 'OVERLAP_WGRAD', True)
    monkeypatch.setattr(ops, 'WGRAD_GROUP_MAX_HW', 0)
    calls = counted_defer(monkeypatch)
    base = grads(*step(blks, x0, dy))
    assert not calls
    monkeypatch.setattr(ops, 'WGRAD_GROUP_MAX_HW', 1024)
    x, params = step(blks, x0, dy)
    assert len(calls) == 4 and ops.wgrads_pending() == 0            # four 3x3 convs deferred, flushed before .backward() returned
    eager = grads(x, params)
    for a, b in zip(eager, base):
        assert fro_err(a, b) < TOL_ORDER, fro_err(a, b)

    # the same step captured into a graph: the grouped launch is a node of it (its table sits in the kernel arguments)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops._stream()
        step(blks, x0, dy)                                           # settles the per-stream workspaces outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
        x, params = step(blks, x0, dy)
        assert ops.wgrads_pending() == 0
    for _ in range(2):
        graph.replay()
        for a, b in zip(grads(x, params), eager):
            assert fro_err(a, b) < TOL_ORDER, fro_err(a, b)


def test_deterministic_mode_defers_nothing(blocks, monkeypatch):
    blks, x0, dy = blocks
    monkeypatch.setattr(ops, 'OVERLAP_WGRAD', True)
    calls = counted_defer(monkeypatch)
    ops.set_deterministic(True)
    try:
        monkeypatch.setattr(ops, 'WGRAD_GROUP_MAX_HW', 0)
        base = grads(*step(blks, x0, dy))
        monkeypatch.setattr(ops, 'WGRAD_GROUP_MAX_HW', 1024)
        x, params = step(blks, x0, dy)
        assert not calls and ops.wgrads_pending() == 0
        for a, b in zip(grads(x, params), base):
            assert torch.equal(a, b)
        # ... and the library refuses the grouped launch itself in this mode
        p = problem(1, 64, 64, 8, 16)
        t = target(p[2])
        status, _, _ = ops.raw_conv_wgrad_group([(p[0], p[1], t)])
        torch.cuda.synchronize()
        assert status == native.ERR_SHAPE and torch.equal(t, p[2])
    finally:
        ops.set_deterministic(False)


def test_stale_items_are_dropped_at_the_next_forward(blocks):
    """what a backward that raised leaves behind: an item deferred with no end-of-call flush queued (here: outside any backward)"""
    blks, x0, dy = blocks
    p = problem(1, 64, 64, 8, 16)
    t = target(p[2])
    ops.defer_wgrad(p[0], p[1], t)
    assert ops.wgrads_pending() == 1
    with torch.no_grad():
        blks[0](x0)
    assert ops.wgrads_pending() == 0 and ops.flush_wgrads() == 0
    torch.cuda.synchronize()
    assert torch.equal(t, p[2])                                       # dropped, not launched
