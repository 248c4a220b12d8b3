"""Self-attention without a GPU: the float64 closed forms of tests/attn_reference.py against float64 autograd, the CPU restatement of
the kernels' arithmetic against float64 on every (shape, kind, dtype) -- the figures the tolerance tables hold, so the tables cannot
drift from the code --, the input kinds, ``AttnBlock`` / ``VQVAE`` construction and config validation, the shipped config, and the
argument validation of vqk_attn_fwd / vqk_attn_bwd.

Every figure is printed (``ATTNMEASURE cpu``) before it is asserted.  Bound of the closed-form check: both sides are float64, the
sums run over at most 1056 keys or 512 channels of O(1) to O(100) terms; measured 1e-13 or below relative to the largest element, 1e-10
leaves three decades and is four below an fp32 slip."""
import ctypes
import importlib
import os

import pytest
import torch
import yaml

from tests import attn_reference as R

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ae = importlib.import_module(PKG + '.modules.autoencoder')
model_mod = importlib.import_module(PKG + '.model')
native = importlib.import_module(PKG + '._native')

AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
QC = dict(num_embeddings=64, embedding_dim=32, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
TC = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)


def build(ae_conf, image_size=32):
    return model_mod.VQVAE(image_size, ae_conf, QC, None, TC, load_loss=False)


# ---------------------------------------------------------------------------------------------- closed forms vs autograd
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', [R.SHAPES[0], R.SHAPES[2], R.SHAPES[3], R.STAGED_SHAPES[0]], ids=R.shape_id)
def test_closed_form_matches_autograd(shape, kind):
    heads = shape[3]
    inp = R.make_inputs(shape, kind)
    q, k, v = (inp[n].clone().requires_grad_(True) for n in ('q', 'k', 'v'))
    qh, kh, vh = (R._heads(t, heads) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * shape[4] ** -0.5
    o = R._rows(torch.softmax(s, dim=-1) @ vh)
    o.backward(inp['do'])
    ref = R.closed_form(inp['q'], inp['k'], inp['v'], inp['do'], heads)
    got = dict(o=o.detach(), lse=torch.logsumexp(s, dim=-1).detach(), dq=q.grad, dk=k.grad, dv=v.grad)
    fig = R.figures(got, ref, kind)
    print('ATTNMEASURE cpu closed-form', R.shape_id(shape), kind, ' '.join(f'{n} {f:.2e}' for n, f in fig.items()))
    assert all(f < 1e-10 for f in fig.values()), fig


def test_closed_form_special_cases():
    """one key: o == v, dv == do, dq == dk == 0; constant keys: the softmax is uniform, dq == 0"""
    inp = R.make_inputs(R.SHAPES[0], 'scale1')
    ref = R.closed_form(inp['q'], inp['k'], inp['v'], inp['do'], 1)
    assert torch.equal(ref['o'], inp['v']) and torch.equal(ref['dv'], inp['do'])
    assert float(ref['dq'].abs().max()) < 1e-13 and float(ref['dk'].abs().max()) < 1e-13
    inp = R.make_inputs(R.SHAPES[2], 'constant')
    ref = R.closed_form(inp['q'], inp['k'], inp['v'], inp['do'], 1)
    assert float((ref['o'] - inp['v'].mean(1, keepdim=True)).abs().max()) < 1e-13
    assert float(ref['dq'].abs().max()) < 1e-13 < float(ref['dk'].abs().max())


def test_input_kinds_reach_large_logits():
    """what the kinds are for: without the running maximum exp overflows (fp32 exp overflows at 88.7)"""
    for kind, lo, hi in (('scale1', 2.0, 8.0), ('peaked', 120.0, 200.0), ('shifted', 250.0, 400.0)):
        inp = R.make_inputs(R.SHAPES[3], kind)
        s = (R._heads(inp['q'], 2) @ R._heads(inp['k'], 2).transpose(-1, -2)) * 64 ** -0.5
        print('ATTNMEASURE cpu logits', kind, f'{float(s.abs().max()):.1f}')
        assert lo < float(s.abs().max()) < hi
        ref = R.closed_form(inp['q'], inp['k'], inp['v'], inp['do'], 2)
        assert all(bool(torch.isfinite(t).all()) for t in ref.values())


# ---------------------------------------------------------------------------------------------- the tables bound the restatement
@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('kind', R.KINDS)
def test_table_bounds_restatement(kind, dtype):
    worst = {}
    for shape in R.SHAPES:
        inp = R.make_inputs(shape, kind, dtype)
        ref = R.closed_form(inp['q'], inp['k'], inp['v'], inp['do'], shape[3])
        got = R.restate(inp['q'], inp['k'], inp['v'], inp['do'], shape[3], dtype)
        assert all(bool(torch.isfinite(t).all()) for t in got.values())
        fig = R.figures(got, ref, kind)
        print('ATTNMEASURE cpu restate', dtype, kind, R.shape_id(shape), ' '.join(f'{n} {f:.2e}' for n, f in fig.items()))
        for n, f in fig.items():
            worst[n] = max(worst.get(n, 0.0), f)
    for n, f in worst.items():
        entry = R.TABLE[(kind, n, dtype)]
        print('ATTNMEASURE cpu table', dtype, kind, n, f'measured {f:.3e} entry {entry:.1e}')
        assert f <= entry, (kind, n, dtype, f, entry)
        assert entry <= 2 * f + 1e-300, 'a table entry far above what is measured licenses nothing: re-measure it'


def test_bf16_matmul_logits_are_not_the_restatement():
    """why the bf16 restatement keeps fp32 logits: torch's bf16 matmul rounds the logits themselves and is off by percents on ``peaked``"""
    shape = R.SHAPES[3]
    inp = R.make_inputs(shape, 'peaked', 'bf16')
    ref = R.closed_form(inp['q'], inp['k'], inp['v'], inp['do'], shape[3])
    qh, kh, vh = (R._heads(inp[n].to(torch.bfloat16), shape[3]) for n in ('q', 'k', 'v'))
    o = R._rows(torch.softmax((qh @ kh.transpose(-1, -2)).float() * shape[4] ** -0.5, dim=-1).to(torch.bfloat16) @ vh)
    f = R.distance(o, ref['o'])
    print('ATTNMEASURE cpu bf16-matmul-logits o', f'{f:.3e}', 'table', R.TABLE[('peaked', 'o', 'bf16')])
    assert f > 4 * R.TABLE[('peaked', 'o', 'bf16')]


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_block_table_bounds_restatement(dtype):
    worst = {}
    for case in R.BLOCK_CASES:
        ref = R.block_eval(case, 'f64')
        fig = R.block_figures(R.block_eval(case, dtype), ref)
        print('ATTNMEASURE cpu block', dtype, case, ' '.join(f'{n} {f:.2e}' for n, f in fig.items()))
        for n, f in fig.items():
            worst[n] = max(worst.get(n, 0.0), f)
    assert set(worst) == {'out', 'dx', *R.BLOCK_PARAMS}
    for n, f in worst.items():
        assert f <= R.BLOCK_TABLE[(dtype, n)] <= 2 * f, (dtype, n, f, R.BLOCK_TABLE[(dtype, n)])


# ---------------------------------------------------------------------------------------------- module, model, config
def test_attn_block_parameters():
    blk = ae.AttnBlock(64, heads=2)
    assert [n for n, _ in blk.named_parameters()] == list(R.BLOCK_PARAMS)
    assert blk.q.weight.shape == (64, 64, 1, 1) and blk.proj_out.bias.shape == (64,) and blk.norm.weight.shape == (1, 64, 1, 1)
    assert blk.norm.num_groups == 32 and blk.norm.eps == 1e-6
    with pytest.raises(ValueError, match='attn_heads'):
        ae.AttnBlock(64, heads=3)
    with pytest.raises(ValueError, match='32'):
        ae.AttnBlock(48)


def test_absent_keys_change_nothing():
    torch.manual_seed(0)
    base = build(dict(AE))
    keys = list(base.state_dict().keys())
    for extra in (dict(attn_resolutions=None), dict(attn_resolutions=[]), dict(attn_resolutions=[7]), dict(attn_heads=2),
                  dict(attn_resolutions=None, attn_heads=None)):
        torch.manual_seed(0)
        m = build(dict(AE, **extra))
        assert list(m.state_dict().keys()) == keys, extra
        assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), base.state_dict().values())), extra
        assert [type(x).__name__ for x in m.modules()] == [type(x).__name__ for x in base.modules()]
    assert not any('q.' in k or 'proj_out' in k for k in keys)


def test_placement_small():
    m = build(dict(AE, attn_resolutions=[8]))
    names = lambda seq: [type(x).__name__ for x in seq]       # noqa: E731
    # 32 -> 16 -> 8: the encoder's levels run at 32 and 16, its final_residual at 8; the decoder starts at 8
    assert names(m.encoder.blocks) == ['ResBlock', 'Downsample', 'ResBlock', 'Downsample']
    assert names(m.encoder.final_residual) == ['ResBlock', 'AttnBlock']
    assert names(m.decoder.initial_residual) == ['ResBlock', 'AttnBlock']
    assert names(m.decoder.blocks) == ['ResBlock', 'AttnBlock', 'Upsample', 'ResBlock', 'Upsample']
    sd = m.state_dict()
    assert sd['encoder.final_residual.1.q.weight'].shape == (64, 64, 1, 1)
    assert 'decoder.initial_residual.1.proj_out.weight' in sd and 'decoder.blocks.1.norm.weight' in sd
    assert m.encoder.final_residual[1].heads == 1
    assert build(dict(AE, attn_resolutions=[8], attn_heads=2)).decoder.blocks[1].heads == 2
    # an attention level inside the encoder's walk: ResBlock, AttnBlock, Downsample -- and shallow_split still finds a Downsample
    m = build(dict(AE, attn_resolutions=[16, 8]))
    assert names(m.encoder.blocks) == ['ResBlock', 'Downsample', 'ResBlock', 'AttnBlock', 'Downsample']
    split = m.encoder.shallow_split(1.0)
    assert split is None or isinstance(m.encoder.blocks[split], ae.Downsample)
    decay, no_decay = m.optimizer_groups()
    assert 'encoder.blocks.3.q.weight' in dict(decay) and 'encoder.blocks.3.q.bias' in dict(no_decay)
    assert 'encoder.blocks.3.norm.weight' in dict(no_decay)


def test_placement_shipped_config():
    with open(os.path.join(ROOT, 'example_confs', 'attn_vqgan.yaml')) as f:
        conf = yaml.safe_load(f)
    with open(os.path.join(ROOT, 'example_confs', 'gumbel_vqgan.yaml')) as f:
        base = yaml.safe_load(f)
    assert conf['autoencoder']['attn_resolutions'] == [16] and conf['autoencoder'].get('attn_heads', 1) == 1
    assert {k: v for k, v in conf['autoencoder'].items() if not k.startswith('attn_')} == base['autoencoder']
    assert {k: conf[k] for k in conf if k != 'autoencoder'} == {k: base[k] for k in base if k != 'autoencoder'}
    a = conf['autoencoder']
    kw = dict(attn_resolutions=a['attn_resolutions'], attn_heads=a['attn_heads'], image_size=conf['image_size'])
    with torch.device('meta'):
        enc = ae.Encoder(a['channels'], a['num_res_blocks'], tuple(a['channel_multipliers']), 256, **kw)
        dec = ae.Decoder(a['channels'], a['num_res_blocks'], tuple(a['channel_multipliers']), 256, **kw)
    count = lambda seq: sum(isinstance(x, ae.AttnBlock) for x in seq)      # noqa: E731
    assert (count(enc.blocks), count(enc.final_residual), count(dec.initial_residual), count(dec.blocks)) == (0, 2, 2, 2)
    assert [type(x).__name__ for x in dec.blocks][:5] == ['ResBlock', 'AttnBlock', 'ResBlock', 'AttnBlock', 'Upsample']
    # the decoder's 16x16 level already narrows to channels x 2: d = 512 in final_residual / initial_residual, 256 there
    assert [x.in_channels for x in enc.final_residual if isinstance(x, ae.AttnBlock)] == [512, 512]
    assert [x.in_channels for x in dec.modules() if isinstance(x, ae.AttnBlock)] == [512, 512, 256, 256]
    assert all(x.heads == 1 for x in dec.modules() if isinstance(x, ae.AttnBlock))


@pytest.mark.parametrize('extra,match', [(dict(attn_resolutions=8), 'list'), (dict(attn_resolutions='8'), 'list'),
                                         (dict(attn_resolutions=[8.0]), 'positive integers'), (dict(attn_resolutions=[0]), 'positive'),
                                         (dict(attn_resolutions=[8], attn_heads=3), 'attn_heads'),
                                         (dict(attn_resolutions=[8], attn_heads=0), 'attn_heads')])
def test_config_validation(extra, match):
    with pytest.raises(ValueError, match=match):
        build(dict(AE, **extra))


def test_operators_refuse_cpu_tensors():
    ops = importlib.import_module(PKG + '.ops')
    x = torch.zeros(1, 4, 64)
    for fn in (ops.attention, ops.attention_staged):
        with pytest.raises(RuntimeError, match='GPU only'):
            fn(x, x, x, 1)
    assert ops.attn_fused_serves(torch.float32, 1, 512) and ops.attn_fused_serves(torch.bfloat16, 8, 64)
    assert not ops.attn_fused_serves(torch.float32, 2, 32) and not ops.attn_fused_serves(torch.float32, 1, 96)
    assert not ops.attn_fused_serves(torch.float16, 1, 64)
    assert ops.ATTN_FUSED is True


# ---------------------------------------------------------------------------------------------- the entry points validate without a GPU
def test_entry_points_reject_bad_arguments():
    lib = native.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    E = dict(shape=-1, dtype=-2, align=-3, arg=-5)

    def fwd(dtype=0, q=p, k=p, v=p, o=p, lse=p, b=1, n=4, heads=1, d=64, ldq=64, ldk=64, ldv=64, ldo=64):
        return lib.vqk_attn_fwd(dtype, q, k, v, o, lse, b, n, heads, d, ldq, ldk, ldv, ldo, 0.125, None)

    def bwd(dtype=0, q=p, do=p, dq=p, delta=p, n=4, heads=1, d=64, lddo=64, lddk=64):
        return lib.vqk_attn_bwd(dtype, q, p, p, p, p, do, dq, p, p, delta, 1, n, heads, d, 64, 64, 64, 64, lddo, 64, lddk, 64, 0.125, None)

    assert fwd(dtype=2) == E['dtype'] and bwd(dtype=-1) == E['dtype']
    for d in (0, 32, 96, 1024):
        assert fwd(d=d, ldq=2048, ldk=2048, ldv=2048, ldo=2048) == E['shape'], d
        assert bwd(d=d) == E['shape'], d
    assert fwd(n=0) == E['shape'] and fwd(b=0) == E['shape'] and fwd(heads=0) == E['shape'] and fwd(b=70000) == E['shape']
    assert bwd(n=0) == E['shape']
    assert fwd(q=None) == E['arg'] and fwd(lse=None) == E['arg'] and bwd(delta=None) == E['arg'] and bwd(dq=None) == E['arg']
    assert fwd(ldq=63) == E['shape']                          # shorter than heads * d
    assert fwd(ldv=66) == E['shape'] and bwd(lddo=66) == E['shape']       # 264 bytes: not a multiple of 16
    assert fwd(dtype=1, ldo=68) == E['shape']                 # bf16: 136 bytes
    assert fwd(heads=2, ldk=64) == E['shape'] and bwd(heads=2) == E['shape']
    assert fwd(q=p + 4) == E['align'] and fwd(o=p + 8) == E['align'] and bwd(do=p + 4) == E['align'] and bwd(dq=p + 2) == E['align']
    assert {'vqk_attn_fwd', 'vqk_attn_bwd'} <= set(native.EXPORTS)
