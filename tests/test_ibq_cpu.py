"""The index-backpropagation (IBQ) quantizer without a GPU: the float64 closed forms (tests/ibq_reference.py) against torch.autograd
on the literal formulation (Ind = hard - sg[P] + P, three loss terms), the error table of the fp32 restatement re-measured, the
token-margin condition of the shared inputs, the argument validation of the entry points, ``IBQuantizer`` / ``VQVAE`` construction on
the CPU with the shipped config, the state dict and the config refusals.

Bounds.  Closed forms against autograd: both sides float64, sums over at most 96 O(1) terms that differ in association only -- about
1e-14; 1e-10 (relative to the quantity's maximum) leaves four decades.  TABLE: an entry must bound what is measured here and may not
be more than 1.5 x above it (it is the measured figure rounded up to two digits -- the slack covers exp / log of another libm).
Margin: eta = (D + 1) 2^-24 |z_i| max_j |e_j| / T per row (ibq_reference.eta); at least 99 % of the rows of every GPU shape of the
'normal', 'init' and 'scaled' kinds have their float64 top-two logits more than 2 eta apart."""
import importlib
import os

import pytest
import torch

from tests import ibq_reference as R

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)


def q_conf(k=64, dim=64, reinit=None, qtype='ibq', init=None, **params):
    conf = dict(num_embeddings=k, embedding_dim=dim, reinit_every_n_epochs=reinit, type=qtype, params=dict(commitment_cost=0.25, **params))
    if init is not None:
        conf['codebook_init'] = init
    return conf


# ---------------------------------------------------------------------------------------------- closed forms vs torch.autograd
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('temperature', R.TEMPS)
def test_closed_forms_match_autograd_on_the_literal_formulation(kind, temperature):
    z, e, g = R.make_case(65, 96, 64, kind)
    lit = R.literal(z, e, g, R.SCALE, R.BETA, temperature)
    cf = R.closed_form(z, e, None, g, R.SCALE, R.BETA, temperature)
    assert torch.equal(lit['idx'], cf['idx'])
    if kind == 'collapsed':
        assert int(cf['idx'].max()) < 4                                       # the smallest index of the winning group
    assert abs(float(lit['loss'] - cf['loss'])) <= 1e-10 * float(cf['loss'])
    for name in ('dz', 'de'):
        fig = R.distance(cf[name], lit[name])
        print(f'IBQMEASURE closed form vs autograd {kind} T={temperature} {name}: {fig:.3e} (bound 1e-10)')
        assert fig <= 1e-10, name


def test_absent_cotangents_give_zero():
    z, e, g = R.make_case(65, 96, 64, 'normal')
    cf = R.closed_form(z, e, None, None, None)
    assert float(cf['dz'].abs().max()) == 0.0 and float(cf['de'].abs().max()) == 0.0


def test_out_of_range_tokens_have_no_hard_terms():
    z, e, g = R.make_case(65, 96, 64, 'normal')
    idx = R.closed_form(z, e)['idx'].clone()
    bad = idx.clone()
    bad[3], bad[40] = -1, 96
    a, b = R.closed_form(z, e, idx, g, R.SCALE), R.closed_form(z, e, bad, g, R.SCALE)
    rows = torch.ones(65, dtype=torch.bool)
    rows[3] = rows[40] = False
    assert torch.equal(a['lse'], b['lse']) and torch.equal(a['ebar'], b['ebar'])
    # the other rows' dz is untouched; the two rows keep only their soft part with G = g
    assert R.distance(b['dz'][rows], a['dz'][rows]) <= 1e-12
    only_g = R.closed_form(z[[3, 40]], e, torch.tensor([-1, 96]), g[[3, 40]], None)
    assert R.distance(b['dz'][~rows], only_g['dz']) <= 1e-12


# ---------------------------------------------------------------------------------------------- the table cannot drift
def test_table_bounds_restatement():
    worst = {}
    for case in R.TABLE_CASES:
        for quant, fig in R.measure(case).items():
            key = (case[1], quant)
            worst[key] = max(worst.get(key, 0.0), fig)
    assert set(worst) == set(R.TABLE)
    for key, fig in sorted(worst.items()):
        print(f'IBQMEASURE restatement {key}: {fig:.3e} (table {R.TABLE[key]:.2g})')
    for key, fig in worst.items():
        assert fig <= R.TABLE[key] <= 1.5 * fig, key


def test_restatement_tokens_are_accepted():
    for kind in R.KINDS:
        z, e, g = R.make_case(130, 200, 256, kind)
        r = R.restate(z, e, g, R.SCALE)
        R.check_acceptance(z, e, r['idx'])
        if kind == 'collapsed':
            assert int(r['idx'].max()) < 4


# ---------------------------------------------------------------------------------------------- the token-margin condition
@pytest.mark.parametrize('shape', R.SHAPES, ids=R.shape_id)
def test_rows_are_separated(shape):
    for kind in R.MARGIN_KINDS:
        z, e, _ = R.make_case(*shape, kind)
        _, _, _, gap, eta2 = R.margins(z, e)                   # (the gap and eta both scale with 1 / T: one temperature decides)
        sep = float((gap > eta2).double().mean())
        print(f'IBQMEASURE separated rows {R.shape_id(shape)} {kind}: {sep:.4f} (bound >= 0.99)')
        assert sep >= 0.99, (shape, kind)


# ---------------------------------------------------------------------------------------------- module, model, config
def test_module_state_dict_and_argument_checks():
    vqm = importlib.import_module(PKG + '.modules.vector_quantizers')
    ops = importlib.import_module(PKG + '.ops')
    q = vqm.IBQuantizer(96, 64)
    assert (q.commitment_cost, q.temperature) == (0.25, 1.0)
    assert set(q.state_dict()) == {'codebook.weight'} and tuple(q.state_dict()['codebook.weight'].shape) == (96, 64)
    assert q.codebook.weight.requires_grad
    q.init_codebook()
    assert float(q.codebook.weight.detach().abs().max()) <= 1.0 / 96                    # +- 1 / K, the standard quantizer's start
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='temperature'):
            vqm.IBQuantizer(96, 64, 0.25, bad)
    with pytest.raises(RuntimeError, match='dot products'):
        q.init_codebook_from_data(torch.zeros(128, 64), 1, torch.zeros(96, dtype=torch.float64))
    for call in (lambda: q(torch.zeros(1, 64, 2, 2)), lambda: q.vec_to_codes(torch.zeros(1, 64, 2, 2))):
        with pytest.raises(RuntimeError, match='GPU only'):
            call()
    assert torch.equal(q.codes_to_vec(torch.tensor([[1, 5]])), q.codebook.weight[torch.tensor([[1, 5]])])
    assert ops.ibq_fused_serves(q.codebook.weight) is False                             # a CPU tensor is never served by the kernels
    assert ops.IBQ_FUSED is True
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.ibq_assign(torch.zeros(4, 64), torch.zeros(8, 64))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.ibq_staged(torch.zeros(4, 64), torch.zeros(8, 64))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.IBQLookupFn.apply(torch.zeros(1, 64, 2, 2), torch.zeros(8, 64), 0.25, 1.0, torch.float32)


def test_model_builds_parses_and_refuses():
    model_mod = importlib.import_module(PKG + '.model')
    m = model_mod.VQVAE(32, AE, q_conf(temperature=0.5), None, TC)
    qz = m.quantizer
    assert type(qz).__name__ == 'IBQuantizer' and m.latent_dim == 64 and m.cb_size == 64 and qz.temperature == 0.5
    assert m.encoder.conv_out.weight.shape[0] == 64
    std = model_mod.VQVAE(32, AE, q_conf(qtype='standard'), None, TC)
    assert set(m.state_dict()) == set(std.state_dict())                                 # no new state-dict key
    assert model_mod.VQVAE(32, AE, q_conf(), None, TC).quantizer.temperature == 1.0
    assert model_mod.VQVAE(32, AE, q_conf(reinit=10), None, TC).reinit_every_n_epochs == 10     # allowed
    with pytest.raises(ValueError, match='dot products'):
        model_mod.VQVAE(32, AE, q_conf(init=dict(method='kmeans', samples=256, iters=2)), None, TC)
    for gradient in ('rotation', 'straight_through'):
        with pytest.raises(ValueError, match='gradient estimator'):
            model_mod.VQVAE(32, AE, q_conf(gradient=gradient), None, TC)
    with pytest.raises(ValueError, match='temperature'):
        model_mod.VQVAE(32, AE, q_conf(temperature=0.0), None, TC)


def test_shipped_config():
    train = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    conf = train.get_model_conf(os.path.join(ROOT, 'example_confs', 'ibq_vqvae.yaml'))
    q = conf['quantizer']
    assert (q['type'], q['num_embeddings'], q['embedding_dim'], q['reinit_every_n_epochs']) == ('ibq', 16384, 256, None)
    assert q['params'] == dict(commitment_cost=0.25, temperature=1.0)
    std = train.get_model_conf(os.path.join(ROOT, 'example_confs', 'standard_vqvae.yaml'))
    assert conf['autoencoder'] == std['autoencoder'] and conf['training'] == std['training'] and conf['image_size'] == std['image_size']
    run = train.derive_run_config(conf, 8, {'autoencoder.channels': 32, 'quantizer.num_embeddings': 64})
    m = model_mod.VQVAE(run['image_size'], run['ae_conf'], run['q_conf'], run['l_conf'], run['t_conf'])
    assert type(m.quantizer).__name__ == 'IBQuantizer'
    assert (m.quantizer.num_embeddings, m.quantizer.embedding_dim) == (64, 256)


# ---------------------------------------------------------------------------------------------- the entry points, no device
def test_entry_points_validate_without_gpu():
    native = importlib.import_module(PKG + '._native')
    native.build()
    lib = native.lib()
    for name in ('vqk_ibq_forward_ws_bytes', 'vqk_ibq_forward_f32', 'vqk_ibq_backward_ws_bytes', 'vqk_ibq_backward_f32'):
        assert hasattr(lib, name) and name in native.EXPORTS
    p = 4096                                                  # a non-NULL, 16-byte aligned address: validation never dereferences it
    big = 1 << 40

    def fwd(z=p, e=p, n=64, k=100, d=128, inv_t=1.0, idx=p, lse=p, ebar=p, q32=p, qlo=p, sse=p, hist=p, ws=p, ws_bytes=big):
        return lib.vqk_ibq_forward_f32(z, e, n, k, d, inv_t, idx, lse, ebar, q32, qlo, sse, hist, ws, ws_bytes, 0)

    def bwd(z=p, e=p, idx=p, lse=p, ebar=p, dq=p, dtype=0, n=64, k=100, d=128, inv_t=1.0, dz=p, de=p, ws=p, ws_bytes=big):
        return lib.vqk_ibq_backward_f32(z, e, idx, lse, ebar, dq, dtype, n, k, d, inv_t, 0.1, 0.1, 0, dz, de, ws, ws_bytes, 0)

    for d in (0, 8, 32, 48, 96, 192, 512):
        assert fwd(d=d) == -1 and bwd(d=d) == -1 and lib.vqk_ibq_backward_ws_bytes(64, d) == -1, d       # served: 64, 128, 256
    assert fwd(k=0) == -1 and fwd(n=0) == -1 and fwd(n=1 << 31) == -1 and bwd(k=0) == -1 and bwd(n=0) == -1 and bwd(n=1 << 31) == -1
    assert lib.vqk_ibq_forward_ws_bytes(-1) == -1 and lib.vqk_ibq_forward_ws_bytes(1 << 31) == -1
    assert lib.vqk_ibq_backward_ws_bytes(-1, 64) == -1 and lib.vqk_ibq_backward_ws_bytes(1 << 31, 64) == -1
    for name in ('z', 'e', 'idx'):
        assert fwd(**{name: 0}) == -5, name
    assert fwd(lse=0) == -5 and fwd(ebar=0) == -5                        # both or neither
    assert fwd(inv_t=0.0) == -5 and fwd(inv_t=float('inf')) == -5 and bwd(inv_t=-1.0) == -5
    for name in ('z', 'e', 'ebar', 'q32', 'ws'):
        assert fwd(**{name: p + 4}) == -3, name
    assert fwd(qlo=p + 4) == -3 and fwd(qlo=p + 8, ws=0) == -6           # a bf16 q: 8-byte alignment
    for name in ('z', 'e', 'idx', 'lse', 'ebar', 'dz'):
        assert bwd(**{name: 0}) == -5, name
    for name in ('z', 'e', 'ebar', 'dz', 'de', 'ws', 'dq'):
        assert bwd(**{name: p + 4}) == -3, name
    assert bwd(dq=p + 8, dtype=1, ws=0) == -6 and bwd(dq=p + 4, dtype=1) == -3
    assert bwd(dtype=7) == -2
    for n in (1, 64, 65, 2051, 8192):
        need = ((n + 63) // 64 + 1) * 4
        assert lib.vqk_ibq_forward_ws_bytes(n) == need
        assert fwd(n=n, ws_bytes=need - 1) == -6 and fwd(n=n, ws=0) == -6            # short / missing: refused before any launch
        for d in (64, 128, 256):
            need = (2 * n * d + (n + 3) // 4 * 4) * 4
            assert lib.vqk_ibq_backward_ws_bytes(n, d) == need
            assert bwd(n=n, d=d, ws_bytes=need - 1) == -6 and bwd(n=n, d=d, ws=0) == -6
