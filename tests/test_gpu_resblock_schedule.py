"""The hand-scheduled backward of a ResBlock (ops.ResBlockFn.backward) with its weight gradients on the side stream and every
parameter gradient accumulated straight into an optimizer-style arena: the input gradient and all seven parameter gradients
against a float64 formulation of the block (oracle/vqvae_oracle.py: res_block, downsample) and against the same call under
``ops.no_direct_grad()``, which takes the sequential path and returns its gradients through autograd.

One case per path of the backward; each case counts the calls that tell the paths apart, so it fails if it took another one.
Tolerances: fp32 as tests/test_gpu_ops.py::test_res_block_golden, bf16 as tests/test_gpu_pooled_backward.py."""
import importlib

import numpy as np
import pytest
import torch

from oracle import vqvae_oracle as O

pytestmark = pytest.mark.gpu

ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
ae = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.modules.autoencoder')
DEV, BF, CL = 'cuda:0', torch.bfloat16, torch.channels_last
NAMES = ('norm1.weight', 'norm1.bias', 'conv1.weight', 'norm2.weight', 'norm2.bias', 'conv2.weight', 'conv_shortcut.weight')


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def mark_direct(blk):
    """what FlatAdamW does to its parameters: a zeroed gradient the kernels accumulate into (conv weights: [Cout][k][k][Cin] memory)"""
    for p in blk.parameters():
        if p.dim() == 4:
            o, i, kh, kw = p.shape
            p.grad = torch.zeros(o, kh, kw, i, device=p.device).permute(0, 3, 1, 2)
        else:
            p.grad = torch.zeros_like(p)
        p._vqk_direct_grad = True


def reference(blk, x, dy, pool):
    """float64 on the CPU, on the values the kernels see (the caller made input, cotangent and parameters exact in the compute dtype)"""
    p = {'b.' + k: v.detach().double().cpu().contiguous().requires_grad_(True) for k, v in blk.state_dict().items()}
    xr = x.detach().double().cpu().contiguous().requires_grad_(True)
    y = O.res_block(xr, p, 'b.')
    if pool:
        y = O.downsample(y)
    y.backward(dy.detach().double().cpu().contiguous())
    return xr.grad, {k[2:]: v.grad for k, v in p.items()}


# path: (calls of raw_gn_backward_pooled_add, raw_unpool, _side_stream) of the arena-target backward
CASES = [
    pytest.param(BF, 2, 128, 128, 32, 48, True, (1, 0, 1), id='bf16-pooled-fast-path'),
    pytest.param(BF, 2, 64, 128, 16, 16, False, (0, 0, 1), id='bf16-overlapped-shortcut-lowres'),
    pytest.param(torch.float32, 2, 64, 128, 16, 16, False, (0, 0, 1), id='fp32-overlapped-shortcut-lowres'),
    pytest.param(BF, 1, 128, 128, 24, 40, True, (0, 1, 1), id='bf16-pool-unpool-route'),
]


@pytest.mark.parametrize('dt,n,cin,cout,h,w,pool,path', CASES)
def test_resblock_backward_schedule(monkeypatch, dt, n, cin, cout, h, w, pool, path):
    torch.manual_seed(cin + h + w)
    blk = ae.ResBlock(cin, cout).to(DEV)
    with torch.no_grad():
        blk.norm1.weight.normal_(1.0, 0.2); blk.norm1.bias.normal_(0.0, 0.2)
        blk.norm2.weight.normal_(1.0, 0.2); blk.norm2.bias.normal_(0.0, 0.2)
        for p in blk.parameters():
            p.copy_(p.to(dt).float())
    mark_direct(blk)
    hp, wp = (h // 2, w // 2) if pool else (h, w)
    x0 = torch.randn(n, cin, h, w, device=DEV).to(dt).contiguous(memory_format=CL)
    dy = torch.randn(n, cout, hp, wp, device=DEV).to(dt).contiguous(memory_format=CL)
    want_dx, want = reference(blk, x0, dy, pool)
    names = [k for k in NAMES if k in want]
    assert len(names) == (7 if cin != cout else 6)

    calls = {'pooled_add': 0, 'unpool': 0, 'side': 0}

    def counted(key, fn):
        def run(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return run
    monkeypatch.setattr(ops, 'raw_gn_backward_pooled_add', counted('pooled_add', ops.raw_gn_backward_pooled_add))
    monkeypatch.setattr(ops, 'raw_unpool', counted('unpool', ops.raw_unpool))
    monkeypatch.setattr(ops, '_side_stream', counted('side', ops._side_stream))
    monkeypatch.setattr(ops, 'OVERLAP_WGRAD', True)

    # the scheduled backward: gradients land in the arena views, nothing but dx comes back through autograd
    x = x0.clone().requires_grad_(True)
    blk(x, pool=pool).backward(dy)
    torch.cuda.synchronize()
    assert (calls['pooled_add'], calls['unpool'], calls['side']) == path, calls
    got_dx = x.grad.float().clone()
    got = {k: dict(blk.named_parameters())[k].grad.float().clone() for k in names}

    # the sequential path: no arena targets, no side stream, the pooled gradient unpooled first
    for key in calls:
        calls[key] = 0
    x = x0.clone().requires_grad_(True)
    params = [dict(blk.named_parameters())[k] for k in names]
    with ops.no_direct_grad():
        seq = ops.autograd_grad(blk(x, pool=pool), [x] + params, dy)
    torch.cuda.synchronize()
    assert (calls['pooled_add'], calls['unpool'], calls['side']) == (0, int(pool), 0), calls
    for k, p in zip(names, params):
        assert torch.equal(p.grad.float(), got[k]), k          # the returned gradients did not touch the arena

    for tag, ref_dx, ref in (('float64', want_dx, want), ('sequential', seq[0], dict(zip(names, seq[1:])))):
        errs = {k: rel_err(got[k], ref[k]) for k in names}
        print(f'{tag}: dx {rel_err(got_dx, ref_dx):.3e} ' + ' '.join(f'{k} {e:.3e}' for k, e in errs.items()))
        if dt == torch.float32:
            np.testing.assert_allclose(got_dx.cpu().numpy(), ref_dx.detach().float().cpu().numpy(), rtol=1e-3, atol=3e-5)
            for k in names:
                assert errs[k] < 1e-4, (tag, k, errs[k])
        else:
            assert rel_err(got_dx, ref_dx) < 6e-3, (tag, rel_err(got_dx, ref_dx))
            for k in names:
                assert errs[k] < 6e-3, (tag, k, errs[k])
