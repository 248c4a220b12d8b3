"""``decoder_norm: spatial`` through the model on a tiny VQ-VAE (32x32 images, channels 32, multipliers [1, 2], one res block, attention
at the 8x8 maps): the decoder on the fused kernels against the staged torch formulation, a training step eager and under
``MiniTrainer`` capture + replay, the checkpoint round trip, the adaptive generator weight, and ``decoder_norm: group`` unchanged.

Bound of the decoder comparison: both routes compute in fp32 and differ only inside the nine spatial norms; each is within 5e-6 of
float64 in every measure (tests/test_gpu_spnorm.py), forward and backward cross all nine, the convs between them have gains of O(1):
9 norms x 2 passes x 5e-6 = 9e-5 -- 1e-4 in relative norm for the output and every gradient."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ae = importlib.import_module(PKG + '.modules.autoencoder')
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
ops = importlib.import_module(PKG + '.ops')
spn = importlib.import_module(PKG + '._ops_spnorm')
DEV = 'cuda:0'
S, B = 32, 4
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2), attn_resolutions=[8])
AE_SP = dict(AE, decoder_norm='spatial')
TC = dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
QC = dict(num_embeddings=64, embedding_dim=32, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
LC_GAN = dict(l1_weight=0.8, l2_weight=0.2, perc_weight=1.0,
              adversarial_params=dict(start_epoch=0, loss_type='hinge', g_weight=0.1, use_adaptive=True, r1_reg_weight=10.0,
                                      r1_reg_every=2))


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.set_deterministic(False)


def _batches(count, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(B, 3, S, S, generator=g).to(DEV) for _ in range(count)]


def _model(conf=AE_SP, lc=None, dtype=torch.float32, seed=0):
    torch.manual_seed(seed)
    return model_mod.VQVAE(S, conf, QC, lc, TC, compute_dtype=dtype).to(DEV).train()


def _relnorm(a, r):
    return float((a.double() - r.double()).norm() / (r.double().norm() + 1e-300))


# ---------------------------------------------------------------------------------------------- decoder: fused against staged
def test_decoder_fused_matches_staged(monkeypatch):
    torch.manual_seed(0)
    dec = ae.Decoder(32, 1, (1, 2), 32, attn_resolutions=[8], image_size=S, norm='spatial').to(DEV)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():                          # a norm at its initial affine (1, 0) would leave dbeta / dgamma untested in scale
        for n, p in dec.named_parameters():
            if 'norm_layer' in n:
                p.add_(0.2 * torch.randn(p.shape, generator=g).to(DEV))
    zq0 = torch.randn(B, 32, 8, 8, generator=g).to(DEV)
    dy = torch.randn(B, 3, S, S, generator=g).to(DEV)
    calls = []
    real = spn.raw_spnorm_forward
    monkeypatch.setattr(spn, 'raw_spnorm_forward', lambda *a: (calls.append(a[0].shape), real(*a))[1])

    def run():
        zq = zq0.clone().requires_grad_(True)
        for p in dec.parameters():
            p.grad = None
        out = dec(zq)
        out.backward(dy)
        torch.cuda.synchronize()
        res = {'out': out.detach().clone(), 'dzq': zq.grad.clone()}
        res.update({n: p.grad.clone() for n, p in dec.named_parameters()})
        return res

    fused = run()
    # every decoder norm: 2 per ResBlock (3 blocks), 2 attention norms, the final norm -- at r = 1, 1, 1, 1, 1, 2, 2, 4 ... of the map
    assert len(calls) == 9 and {s[2] for s in calls} == {8, 16, 32}
    monkeypatch.setattr(ops, 'SPNORM_FUSED', False)
    staged = run()
    assert len(calls) == 9
    assert set(fused) == set(staged) and all(v is not None for v in fused.values())
    assert tuple(fused['out'].shape) == (B, 3, S, S) and tuple(fused['dzq'].shape) == (B, 32, 8, 8)
    # gradients that are exactly zero in real arithmetic -- a key bias shifts every logit of a query alike (softmax ignores it); the
    # bias of the last Upsample conv shifts whole channels of a map that only the final norm reads, at one channel per group (the
    # mean takes it out) -- are rounding noise on both routes: measured against the same layer's neighbour instead of each other
    zero = {'initial_residual.1.k.bias': 'initial_residual.1.q.bias', 'blocks.1.k.bias': 'blocks.1.q.bias', 'blocks.4.conv.bias': 'blocks.2.conv.bias'}
    fig = {k: _relnorm(fused[k], staged[k]) for k in fused if k not in zero}
    for k, near in zero.items():
        fig[k] = max(float(r[k].norm() / staged[near].norm()) for r in (fused, staged))
    worst = max(fig, key=fig.get)
    print('SPNMEASURE gpu decoder fused-vs-staged', ' '.join(f'{k} {v:.2e}' for k, v in fig.items()), 'worst', worst, f'{fig[worst]:.2e}')
    assert all(bool(torch.isfinite(v).all()) for v in fused.values())
    assert all(float(staged[k].abs().max()) > 0 for k in staged if k not in zero)
    assert all(v < 1e-4 for v in fig.values()), {k: v for k, v in fig.items() if v >= 1e-4}


# ---------------------------------------------------------------------------------------------- training step: eager and replayed
def _train(graphed, dtype, steps=4):
    m = _model(dtype=dtype, seed=3)
    tr = trainer_mod.MiniTrainer(max_epochs=2, num_training_batches=2, deterministic=True)
    tr.attach(m)
    m.on_train_start()
    feed = _batches(2, seed=15)
    if graphed:
        tr.capture(m, feed[0], warmup=1, preserve_state=True)
    step = tr.train_batch_graphed if graphed else tr.train_batch
    losses = []
    for k in range(steps):
        m.current_epoch = k // 2
        losses.append(float(step(m, feed[k % 2], k % 2).detach()))
    torch.cuda.synchronize()
    ops.check_kernel_health()
    return losses, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, m, tr


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_training_step_eager_and_replayed_give_the_same_bits(dtype):
    """deterministic mode: four steps eager and four steps replayed from the captured graph -- the same weights after every step
    count and the same last gradients, bit for bit; the new parameters are trained (they move).  The REPORTED loss is the project's
    MSE scalar, whose block sums meet in one fp32 atomic in every mode (csrc/pointwise.hip: sse_kernel; 8 blocks here): the same
    reconstruction can report a loss that differs in the last bits -- at most 8 roundings of 2^-24, 5e-7 relative; 1e-6 is asked."""
    first = {k: v.detach().cpu().clone() for k, v in _model(dtype=dtype, seed=3).state_dict().items()}
    eager, w_eager, m_e, t_e = _train(False, dtype)
    replay, w_replay, m_r, t_r = _train(True, dtype)
    print('SPNMEASURE gpu train losses', dtype, eager, replay)
    assert all(np.isfinite(eager))
    np.testing.assert_allclose(replay, eager, rtol=1e-6, atol=0)
    assert set(w_eager) == set(w_replay) and all(torch.equal(w_eager[k], w_replay[k]) for k in w_eager)
    assert torch.equal(t_e.optimizers[0].flat_g, t_r.optimizers[0].flat_g) and float(t_e.optimizers[0].flat_g.abs().max()) > 0
    for k in ('decoder.norm.conv_y.weight', 'decoder.norm.conv_b.bias', 'decoder.norm.norm_layer.weight', 'decoder.norm.norm_layer.bias',
              'decoder.blocks.0.norm1.conv_y.weight', 'decoder.initial_residual.1.norm.conv_b.weight',
              'decoder.initial_residual.0.norm2.norm_layer.weight', 'decoder.conv_in.weight', 'encoder.conv_in.weight'):
        assert not torch.equal(first[k], w_eager[k]), k


def test_split_backward_cuts_at_the_decoder_input():
    """the data-parallel form of the step runs the decoder's backward first, down to a detached leaf at the decoder input, and hands
    that leaf's gradient on (trainer.MiniTrainer._split_step; forced here, its collectives are no-ops without a process group).  zq
    is read by conv_in AND by every conv_y / conv_b: the leaf collects all of them.  The decoder's gradients depend on nothing behind
    the cut, so after one step its weights equal the unsplit step's bit for bit (deterministic mode); the encoder moves as well."""
    feed = _batches(1, seed=15)[0]
    weights = {}
    for form in ('whole', 'split'):
        m = _model(seed=3)
        tr = trainer_mod.MiniTrainer(num_training_batches=2, deterministic=True)
        if form == 'split':
            tr._use_split = lambda model, opt: True
        tr.attach(m)
        m.on_train_start()
        before = m.encoder.conv_in.weight.detach().clone()
        loss = tr.train_batch(m, feed, 0)
        torch.cuda.synchronize()
        ops.check_kernel_health()
        assert np.isfinite(float(loss.detach())) and not torch.equal(before, m.encoder.conv_in.weight)
        weights[form] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    dec = [k for k in weights['whole'] if k.startswith('decoder.')]
    assert any('conv_y' in k for k in dec) and all(torch.equal(weights['whole'][k], weights['split'][k]) for k in dec)


def test_new_parameters_live_in_the_arena():
    m = _model()
    tr = trainer_mod.MiniTrainer(num_training_batches=2)
    opt = tr.attach(m)[0]
    lo, hi = opt.flat_p.data_ptr(), opt.flat_p.data_ptr() + opt.flat_p.numel() * opt.flat_p.element_size()
    inside = [n for n, p in m.decoder.named_parameters() if lo <= p.data_ptr() < hi]
    assert len(inside) == len(list(m.decoder.parameters())) and any('conv_y' in n for n in inside) and any('norm_layer' in n for n in inside)
    assert all(getattr(p, '_vqk_direct_grad', False) for p in m.decoder.parameters())


# ---------------------------------------------------------------------------------------------- checkpoint
def test_checkpoint_round_trip_reproduces_the_reconstruction(tmp_path):
    _, _, m, tr = _train(False, torch.float32, steps=2)
    images = _batches(1, seed=9)[0]
    m.eval()
    with torch.no_grad():
        recon = m.reconstruct(images).clone()
    path = str(tmp_path / 'movq.ckpt')
    tr.save_checkpoint(m, path)
    sd = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    assert sd['decoder.norm.conv_y.weight'].shape == (32, 32, 1, 1) and sd['decoder.blocks.0.norm1.norm_layer.weight'].shape == (1, 64, 1, 1)
    assert set(sd) == set(m.state_dict())
    m2 = _model(seed=1)
    t2 = trainer_mod.MiniTrainer(num_training_batches=2, deterministic=True)
    t2.attach(m2)
    t2.load_checkpoint(m2, path)
    m2.eval()
    with torch.no_grad():
        again = m2.reconstruct(images)
    torch.cuda.synchronize()
    assert torch.equal(again, recon)
    assert torch.equal(m2.decoder.norm.conv_b.weight, m.decoder.norm.conv_b.weight)


# ---------------------------------------------------------------------------------------------- VQ-GAN step: adaptive generator weight
def test_gan_step_with_adaptive_weight():
    """last_layer = decoder.conv_out.weight and the backward cut at the decoder input work as they are: zq is the one input tensor"""
    m = _model(lc=LC_GAN)
    assert m.criterion is not None
    tr = trainer_mod.MiniTrainer(num_training_batches=4)
    tr.attach(m)
    m.on_train_start()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    feed = _batches(2, seed=21)
    for i in range(2):
        tr.train_batch(m, feed[i], i)
    torch.cuda.synchronize()
    ops.check_kernel_health()
    after = m.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values() if v.is_floating_point())
    for k in ('decoder.norm.conv_y.weight', 'decoder.blocks.0.norm2.norm_layer.bias', 'decoder.conv_out.weight', 'encoder.conv_in.weight'):
        assert not torch.equal(before[k], after[k]), k


# ---------------------------------------------------------------------------------------------- decoder_norm: group is today's model
def test_group_is_unchanged(monkeypatch):
    torch.manual_seed(0)
    base = model_mod.VQVAE(S, AE, QC, None, TC).to(DEV)
    torch.manual_seed(0)
    grp = model_mod.VQVAE(S, dict(AE, decoder_norm='group'), QC, None, TC).to(DEV)
    assert list(base.state_dict()) == list(grp.state_dict())
    assert not any('norm_layer' in k or 'conv_y' in k or 'conv_b' in k for k in grp.state_dict())
    assert [type(x).__name__ for x in grp.modules()] == [type(x).__name__ for x in base.modules()]

    def refuse(*a, **k):
        raise AssertionError('decoder_norm: group reached the spatial norm')
    monkeypatch.setattr(spn, 'raw_spnorm_forward', refuse)
    monkeypatch.setattr(spn, 'spatial_norm_staged', refuse)
    images = _batches(1, seed=4)[0]
    base.eval()
    grp.eval()
    ops.set_deterministic(True)
    with torch.no_grad():
        assert torch.equal(base.reconstruct(images), grp.reconstruct(images))
