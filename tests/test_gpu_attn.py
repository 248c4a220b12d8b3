"""Self-attention on the GPU (csrc/attn.hip, _ops_attn.py, AttnBlock, attn_resolutions) against the float64 closed forms of
tests/attn_reference.py.

Metric: max|got - want| / max|want| per quantity (mathematically zero quantities -- ``constant`` dq, dq / dk with one key, the block's
d k.bias -- against a neighbour's magnitude, see attn_reference.figures).  Bound: 4x the entry of attn_reference.TABLE / BLOCK_TABLE,
which is the same figure of the CPU restatement of the kernels' arithmetic (test_attn_cpu.py keeps the tables honest): the kernels
make the same roundings in another order.  For bf16 the float64 reference runs on the bf16-rounded inputs.  Every figure is printed
(``ATTNMEASURE gpu``) with its bound before it is asserted.

Measured on an MI355X, worst ratio of a figure to its bound (4x the table entry) over the seven shapes and four input kinds: fp32 o 0.36,
lse 0.39, dq 0.57 (``shifted``, four heads at d = 128: 1.0e-4 against 1.8e-4), dk 0.33, dv 0.55; bf16 o 0.25, lse 0.26, dq 0.25, dk 0.25,
dv 0.25 -- the bf16 figures sit at the restatement's own (a quarter of the bound): they are the roundings of P, dS and the outputs, not
of the summation order.  With one key o == v and dv == do bit for bit.  AttnBlock (output, dx, ten parameter
gradients; autograd and arena targets give the same figures): worst ratio 0.25 in fp32, 0.30 in bf16."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import attn_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
ae = importlib.import_module(PKG + '.modules.autoencoder')
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
CL = torch.channels_last
TDT = {'fp32': torch.float32, 'bf16': torch.bfloat16}
_REF: dict = {}


def reference(shape, kind, dtype):
    """inputs and float64 closed form of one case, computed once and shared (never modified)"""
    key = (shape, kind, dtype)
    if key not in _REF:
        inp = R.make_inputs(shape, kind, dtype)
        _REF[key] = (inp, R.closed_form(inp['q'], inp['k'], inp['v'], inp['do'], shape[3]))
    return _REF[key]


def fused_lse(q, k, v, heads):
    """(o, lse [B, heads, N]) straight from the autograd Function over the two entry points, [B, N, C] rows"""
    return ops.AttentionFn.apply(q, k, v, heads, float(q.shape[-1] // heads) ** -0.5)


def run(fn, inp, heads, dtype, packed=False):
    """fn(q, k, v, heads) -> o or (o, lse), forward and backward on the device; ``packed``: q, k, v are strided views of ONE
    [B, N, 3C] tensor (read in place), their gradients the slices of its gradient"""
    t = {n: inp[n].to(DEV).to(TDT[dtype]) for n in ('q', 'k', 'v', 'do')}
    c = t['q'].shape[-1]
    if packed:
        qkv = torch.cat([t['q'], t['k'], t['v']], dim=-1).requires_grad_(True)
        q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
        assert all(ops._rows(x).data_ptr() == x.data_ptr() and not x.is_contiguous() for x in (q, k, v))
    else:
        q, k, v = (t[n].clone().requires_grad_(True) for n in ('q', 'k', 'v'))
    out = fn(q, k, v, heads)
    o, lse = out if isinstance(out, tuple) else (out, None)
    o.backward(t['do'])
    torch.cuda.synchronize()
    if packed:
        g = qkv.grad
        got = dict(o=o.detach(), dq=g[..., :c], dk=g[..., c:2 * c], dv=g[..., 2 * c:])
    else:
        got = dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad)
    if lse is not None:
        got['lse'] = lse.detach()
    return {n: x.detach().to('cpu', torch.float64) for n, x in got.items()}


def check(tag, got, ref, kind, dtype, shape):
    fig = R.figures(got, ref, kind)
    line, worst = [], 0.0
    for n, f in fig.items():
        bound = 4.0 * R.TABLE[(kind, n, dtype)]
        worst = max(worst, f / bound)
        line.append(f'{n} {f:.2e}/{bound:.1e}')
    print(f'ATTNMEASURE gpu {tag} {dtype} {kind} {R.shape_id(shape)} ' + ' '.join(line) + f' worst-ratio {worst:.3f}')
    assert all(bool(torch.isfinite(x).all()) for x in got.values()), 'non-finite output'
    for n, f in fig.items():
        assert f <= 4.0 * R.TABLE[(kind, n, dtype)], (tag, n, f, 4.0 * R.TABLE[(kind, n, dtype)])


# ---------------------------------------------------------------------------------------------- 1. fused against float64
@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.SHAPES, ids=R.shape_id)
def test_fused_against_float64(shape, kind, dtype):
    assert ops.attn_fused_serves(TDT[dtype], shape[3], shape[4])
    inp, ref = reference(shape, kind, dtype)
    got = run(fused_lse, inp, shape[3], dtype)
    assert set(got) == set(R.QUANTS)
    check('fused', got, ref, kind, dtype, shape)
    if shape[1] * shape[2] == 1:                                # one key: the softmax is 1, nothing is rounded
        assert torch.equal(got['o'], inp['v']) and torch.equal(got['dv'], inp['do'])


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('kind', ['scale1', 'shifted'])
def test_fused_reads_packed_qkv_in_place(kind, dtype):
    shape = R.SHAPES[3]
    inp, ref = reference(shape, kind, dtype)
    got = run(fused_lse, inp, shape[3], dtype, packed=True)
    check('packed', got, ref, kind, dtype, shape)
    plain = run(fused_lse, inp, shape[3], dtype)
    assert all(torch.equal(got[n], plain[n]) for n in R.QUANTS)   # the same kernels on the same values: the same bits


def test_nhwc_maps_are_rows():
    """[B, C, H, W] in NHWC storage goes in as it is and comes back NHWC"""
    shape = R.SHAPES[2]
    b, h, w, heads, d = shape
    inp, ref = reference(shape, 'scale1', 'fp32')
    maps = {n: inp[n].to(DEV).float().view(b, h, w, d).permute(0, 3, 1, 2) for n in ('q', 'k', 'v')}
    assert all(m.is_contiguous(memory_format=CL) for m in maps.values())
    o = ops.attention(maps['q'], maps['k'], maps['v'], heads)
    assert tuple(o.shape) == (b, d, h, w) and o.is_contiguous(memory_format=CL)
    rows = o.permute(0, 2, 3, 1).reshape(b, h * w, d)
    assert torch.equal(rows, ops.attention(*(inp[n].to(DEV).float() for n in ('q', 'k', 'v')), heads))
    f = R.distance(rows.cpu(), ref['o'])
    print(f'ATTNMEASURE gpu nhwc o {f:.2e}')
    assert f <= 4.0 * R.TABLE[('scale1', 'o', 'fp32')]


# ---------------------------------------------------------------------------------------------- 2. fused / staged
@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.SHAPES, ids=R.shape_id)
def test_fused_against_staged(shape, kind, dtype, monkeypatch):
    inp, ref = reference(shape, kind, dtype)
    fused = run(ops.attention, inp, shape[3], dtype)
    monkeypatch.setattr(ops, 'ATTN_FUSED', False)
    calls = []
    monkeypatch.setattr(ops.AttentionFn, 'apply', lambda *a: calls.append(a))
    staged = run(ops.attention, inp, shape[3], dtype)
    assert not calls                                            # the switch took the staged path
    assert all(torch.equal(staged[n], x) for n, x in run(ops.attention_staged, inp, shape[3], dtype).items())
    check('staged', staged, ref, kind, dtype, shape)
    # fused against staged in the same metric and at the same bound, on the float64 magnitudes
    diff = {n: fused[n] - staged[n] + ref[n] for n in fused}
    check('fused-staged', diff, ref, kind, dtype, shape)


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', R.STAGED_SHAPES, ids=R.shape_id)
def test_staged_serves_other_head_dims(shape, kind, dtype):
    assert not ops.attn_fused_serves(TDT[dtype], shape[3], shape[4])
    inp, ref = reference(shape, kind, dtype)
    check('staged-d', run(ops.attention, inp, shape[3], dtype), ref, kind, dtype, shape)
    with pytest.raises(RuntimeError, match='attn_fwd failed'):           # the entry point itself refuses the head dim: nothing launched
        fused_lse(*(inp[n].to(DEV).float() for n in ('q', 'k', 'v')), shape[3])


# ---------------------------------------------------------------------------------------------- 3. the same bits on every run
@pytest.mark.parametrize('deterministic', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('shape', [R.SHAPES[2], R.SHAPES[4], R.SHAPES[6]], ids=R.shape_id)
def test_two_runs_are_bit_equal(shape, dtype, deterministic):
    inp, _ = reference(shape, 'peaked', dtype)
    ops.set_deterministic(deterministic)
    try:
        a = run(fused_lse, inp, shape[3], dtype)
        b = run(fused_lse, inp, shape[3], dtype)
    finally:
        ops.set_deterministic(False)
    assert set(a) == set(R.QUANTS) and all(torch.equal(a[n], b[n]) for n in a)
    if deterministic:                                           # one code path: the mode changes nothing
        c = run(fused_lse, inp, shape[3], dtype)
        assert all(torch.equal(a[n], c[n]) for n in a)


# ---------------------------------------------------------------------------------------------- 4. AttnBlock
def block_reference(case):
    if ('block', case) not in _REF:
        _REF[('block', case)] = (R.make_block(case), R.block_eval(case, 'f64'))
    return _REF[('block', case)]


def mark_direct(blk):
    """what FlatAdamW does to its parameters: a zeroed gradient the kernels accumulate into (conv weights: [Cout][k][k][Cin] memory)"""
    for p in blk.parameters():
        if p.dim() == 4 and p.shape[0] > 1:
            o, i, kh, kw = p.shape
            p.grad = torch.zeros(o, kh, kw, i, device=p.device).permute(0, 3, 1, 2)
        else:
            p.grad = torch.zeros_like(p)
        p._vqk_direct_grad = True


@pytest.mark.parametrize('direct', [False, True], ids=['autograd', 'direct'])
@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('case', R.BLOCK_CASES, ids=lambda c: 'B%d-C%d-%dx%d-h%d' % c)
def test_attn_block_against_float64(case, dtype, direct):
    b, c, h, w, heads = case
    vals, ref = block_reference(case)
    blk = ae.AttnBlock(c, heads).to(DEV)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            p.copy_(vals[n].to(DEV).float())
    if direct:
        mark_direct(blk)
    x = vals['x'].to(DEV).to(TDT[dtype]).contiguous(memory_format=CL).requires_grad_(True)
    dy = vals['dy'].to(DEV).to(TDT[dtype]).contiguous(memory_format=CL)
    y = blk(x)
    assert y.dtype == TDT[dtype] and tuple(y.shape) == (b, c, h, w)
    y.backward(dy)
    torch.cuda.synchronize()
    got = {'out': y.detach(), 'dx': x.grad}
    got.update({n: p.grad for n, p in blk.named_parameters()})
    got = {n: t.detach().to('cpu', torch.float64) for n, t in got.items()}
    fig = R.block_figures(got, ref)
    print(f'ATTNMEASURE gpu block {dtype} {case} direct={int(direct)} ' +
          ' '.join(f'{n} {f:.2e}/{4 * R.BLOCK_TABLE[(dtype, n)]:.1e}' for n, f in fig.items()) +
          f' worst-ratio {max(f / (4 * R.BLOCK_TABLE[(dtype, n)]) for n, f in fig.items()):.3f}')
    assert set(fig) == {'out', 'dx', *R.BLOCK_PARAMS}
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    for n, f in fig.items():
        assert f <= 4.0 * R.BLOCK_TABLE[(dtype, n)], (n, f, 4.0 * R.BLOCK_TABLE[(dtype, n)])


# ---------------------------------------------------------------------------------------------- 5. model
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
QC = dict(num_embeddings=64, embedding_dim=32, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))


def _images(seed=3, b=4):
    return torch.rand(b, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize('dtype,heads', [(torch.float32, 1), (torch.bfloat16, 1), ('bf16x3', 1), (torch.float32, 2)],
                         ids=['fp32', 'bf16', 'bf16x3', 'fp32-heads2-staged'])
def test_model_step_tokens_roundtrip_and_checkpoint(dtype, heads, tmp_path, monkeypatch):
    conf = dict(AE, attn_resolutions=[8], attn_heads=heads)
    fused = []
    real = ops.AttentionFn.apply
    monkeypatch.setattr(ops.AttentionFn, 'apply', lambda *a: (fused.append(a[3]), real(*a))[1])
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, conf, QC, None, TC, compute_dtype=dtype).to(DEV).train()
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    m.on_train_start()
    images = _images()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss = tr.train_batch(m, images, 0)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
    # heads 1: d = 64 in final_residual / initial_residual (the fused kernels), d = 32 at the decoder's narrowed 8x8 level and with
    # heads 2 everywhere (the staged path)
    assert len(fused) == (2 if heads == 1 else 0)
    after = m.state_dict()
    for k in ('encoder.final_residual.1.q.weight', 'decoder.initial_residual.1.proj_out.weight', 'decoder.blocks.1.k.bias',
              'encoder.final_residual.1.norm.weight', 'encoder.conv_in.weight'):
        assert not torch.equal(before[k], after[k]), k
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    m.eval()
    with torch.no_grad():
        tokens = m.get_tokens(images)
        assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (4, 64)
        ops.set_deterministic(True)
        try:
            tokens_det = m.get_tokens(images)
            assert torch.equal(m.reconstruct_from_tokens(tokens_det), m.reconstruct(images))
        finally:
            ops.set_deterministic(False)
    path = str(tmp_path / 'attn.ckpt')
    tr.save_checkpoint(m, path)
    torch.manual_seed(1)
    m2 = model_mod.VQVAE(32, conf, QC, None, TC, compute_dtype=dtype).to(DEV)
    t2 = trainer_mod.MiniTrainer(num_training_batches=10)
    t2.attach(m2)
    t2.load_checkpoint(m2, path)
    m2.eval()
    assert torch.equal(m2.get_tokens(images), tokens)
    assert torch.equal(m2.decoder.blocks[1].q.weight, m.decoder.blocks[1].q.weight)


# ---------------------------------------------------------------------------------------------- 6. train.py / evaluate.py
SMALL = ['--set', 'image_size=32', '--set', 'autoencoder.channels=32', '--set', 'autoencoder.num_res_blocks=1',
         '--set', 'autoencoder.channel_multipliers=[1, 2]', '--set', 'autoencoder.attn_resolutions=[8]',
         '--set', 'quantizer.num_embeddings=64', '--set', 'quantizer.embedding_dim=32', '--set', 'training.cumulative_bs=4']


def test_entry_points(tmp_path, capsys):
    train = importlib.import_module(PKG + '.train')
    ev = importlib.import_module(PKG + '.evaluate')
    conf = os.path.join(ROOT, 'example_confs', 'attn_vqgan.yaml')
    args = ['--params_file', conf] + SMALL + ['--max_epochs', '1', '--batches_per_epoch', '2', '--seed', '0', '--dtype', 'bf16',
                                              '--save_path', str(tmp_path), '--run_name', 'attn']
    capsys.readouterr()
    loss = train.main(args)
    out = capsys.readouterr().out
    assert loss is not None and np.isfinite(loss)
    assert 'eager launches' not in out                          # the step with its attention blocks was captured, not given up
    ckpt = str(tmp_path / 'attn' / 'epoch=00.ckpt')
    assert os.path.exists(ckpt)
    sd = torch.load(ckpt, map_location='cpu', weights_only=False)['state_dict']
    assert 'encoder.final_residual.1.q.weight' in sd and 'decoder.blocks.1.proj_out.bias' in sd
    small = tmp_path / 'conf.yaml'
    small.write_text('image_size: 32\nautoencoder:\n  channels: 32\n  num_res_blocks: 1\n  channel_multipliers: [1, 2]\n'
                     '  attn_resolutions: [8]\nquantizer:\n  num_embeddings: 64\n  embedding_dim: 32\n  type: gumbel\n  params:\n'
                     '    straight_through: False\n    temp: 1.0\n    kl_cost: 0.00859375\n  reinit_every_n_epochs:\n')
    pt = str(tmp_path / 'test.pt')
    torch.save(torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(5)), pt)
    capsys.readouterr()
    res = ev.main(['--params_file', str(small), '--batch_size', '4', '--seed', '0', '--loading_path', ckpt, '--dtype', 'bf16',
                   '--dataset_path', pt])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert json.loads(lines[-1]) == res
    assert {'mse', 'psnr', 'ssim', 'used_codebook', 'perplexity'} <= set(res) and np.isfinite(res['mse'])


# ---------------------------------------------------------------------------------------------- 7. absent keys: today's model
def test_absent_keys_change_nothing():
    torch.manual_seed(0)
    base = model_mod.VQVAE(32, dict(AE), QC, None, TC, load_loss=False)
    keys = list(base.state_dict().keys())
    assert not any('q.' in k or 'proj_out' in k for k in keys)
    for extra in (dict(attn_resolutions=None), dict(attn_resolutions=[]), dict(attn_resolutions=[7])):
        m = model_mod.VQVAE(32, dict(AE, **extra), QC, None, TC, load_loss=False)
        assert list(m.state_dict().keys()) == keys, extra
    launches = []
    real = ops.AttentionFn.apply
    ops.AttentionFn.apply = lambda *a: (launches.append(1), real(*a))[1]
    try:
        base.to(DEV).eval()
        with torch.no_grad():
            base.reconstruct(_images())
    finally:
        ops.AttentionFn.apply = real
    assert not launches
