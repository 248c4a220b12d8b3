"""The step guard without a GPU: the float64 reference (tests/stepguard_reference.py) against torch.optim.AdamW +
torch.nn.utils.clip_grad_norm_ with GradScaler-style skipped steps, hand-worked verdicts, argument validation of the two entry
points, FlatAdamW.enable_guard's argument checks, the train.py flags and the log record's guard/* keys.

Bound of the reference check: both sides are float64 (unit roundoff 1.1e-16); a step is about twenty roundings per element in either
formulation (torch folds the same arithmetic differently: lerp, addcdiv, per-tensor norms), 24 steps, and the update m / (sqrt(v) +
eps) has a condition number of a few -- below 1e-12 relative.  rtol = 1e-10 (atol 1e-14 for elements that pass through zero) leaves
two decades and is six decades below anything a float32 slip would show."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

from tests import stepguard_reference as R

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
optim = importlib.import_module(PKG + '.optim')
native = importlib.import_module(PKG + '._native')


# ---------------------------------------------------------------------------------------------- reference vs torch
@pytest.mark.parametrize('betas', [(0.0, 0.99), (0.9, 0.999)])
@pytest.mark.parametrize('max_norm', [None, 0.75])
def test_reference_matches_torch_adamw_with_skipped_steps(betas, max_norm):
    """24 steps, two weight-decay groups (the reference's split: decay on conv weights only); on the chosen steps ``step()`` is not
    called -- what GradScaler does on an Inf / NaN -- and the torch optimizer's own step count does not advance"""
    rng = np.random.default_rng(11)
    shapes, wds = [(7, 5), (13,), (3, 4, 2), (9,)], [1e-2, 0.0, 1e-2, 0.0]
    params = [torch.tensor(rng.standard_normal(s), dtype=torch.float64, requires_grad=True) for s in shapes]
    lr, eps = 3e-3, 1e-8
    topt = torch.optim.AdamW([dict(params=[params[0], params[2]], weight_decay=1e-2), dict(params=[params[1], params[3]], weight_decay=0.0)],
                             lr=lr, betas=betas, eps=eps)
    flat = np.concatenate([p.detach().numpy().ravel() for p in params])
    wd = np.concatenate([np.full(int(np.prod(s)), w) for s, w in zip(shapes, wds)])
    ref = R.GuardedAdamW(flat, wd, lr, betas, eps, skip_nonfinite=True, max_norm=max_norm)
    skipped_steps = {2, 3, 9, 17, 18, 19}
    coefs = []
    for t in range(24):
        grads = [rng.standard_normal(s) * (10.0 ** rng.uniform(-2, 0.5)) for s in shapes]
        g = np.concatenate([x.ravel() for x in grads])
        if t in skipped_steps:
            g[(7 * t) % g.size] = (math.nan, math.inf, -math.inf)[t % 3]
        apply, coef = ref.step(g)
        assert apply == (t not in skipped_steps)
        if apply:                                                     # GradScaler: step() is called only for finite gradients
            for p, x in zip(params, grads):
                p.grad = torch.tensor(x, dtype=torch.float64)
            if max_norm is not None:
                total = torch.nn.utils.clip_grad_norm_(params, max_norm)
                assert abs(float(total) - ref.last_norm) <= 1e-12 * ref.last_norm
            topt.step()
            coefs.append(coef)
        got = torch.cat([p.detach().reshape(-1) for p in params]).numpy()
        np.testing.assert_allclose(ref.p, got, rtol=1e-10, atol=1e-14)
    assert ref.applied == 18 and ref.skipped == 6 and ref.max_run == 3 and ref.run == 0
    assert float(topt.state[params[0]]['step']) == 18.0
    np.testing.assert_allclose(ref.v, torch.cat([topt.state[p]['exp_avg_sq'].reshape(-1) for p in params]).numpy(), rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(ref.m, torch.cat([topt.state[p]['exp_avg'].reshape(-1) for p in params]).numpy(), rtol=1e-10, atol=1e-14)
    if max_norm is None:
        assert ref.clipped == 0 and ref.coef_min == 1.0 and ref.coef_sum == 18.0
    else:
        assert ref.clipped == sum(c < 1.0 for c in coefs) > 0 and ref.coef_min == min(coefs) < 1.0


def test_hand_worked_verdicts():
    # norm 5 (3-4-5) against max_norm above, at and below it
    assert R.verdict(25.0, 0.0, True, 10.0) == (True, 1.0, 5.0)
    apply, coef, norm = R.verdict(25.0, 0.0, True, 5.0)               # at: 5 / (5 + 1e-6) is just below 1, as clip_grad_norm_ gives it
    assert apply and norm == 5.0 and coef == 5.0 / 5.000001 and coef < 1.0
    assert R.verdict(25.0, 0.0, True, 5.000001) == (True, 1.0, 5.0)   # max_norm = norm + 1e-6: exactly 1
    apply, coef, _ = R.verdict(25.0, 0.0, True, 2.5)
    assert apply and coef == 2.5 / 5.000001
    # non-finite elements: skipped only when asked to
    assert R.verdict(25.0, 1.0, True, None) == (False, 1.0, 5.0)
    assert R.verdict(25.0, 3.0, False, None) == (True, 1.0, 5.0)
    assert R.verdict(25.0, 1.0, False, 2.5) == (True, 2.5 / 5.000001, 5.0)
    assert R.verdict(25.0, 1.0, True, 2.5)[0] is False
    # clipping off: None, and the ABI's "<= 0"
    assert R.verdict(1e12, 0.0, True, None) == (True, 1.0, 1e6) and R.verdict(1e12, 0.0, True, 0.0)[1] == 1.0
    assert R.verdict(0.0, 0.0, True, 1.0) == (True, 1.0, 0.0)         # zero gradients: 1 / 1e-6 clamps to 1
    assert R.arena_row([3.0, math.nan, -4.0, math.inf], 1.0) == (25.0, 4.0, 2.0)
    assert R.arena_row([3.0, math.nan, -4.0, 7.0], 0.5, mask=[1, 0, 1, 0]) == (6.25, 2.0, 0.0)
    assert R.eff_scale(0.5, 0.5) == np.float32(0.25)


def test_reference_counters():
    ref = R.GuardedAdamW(np.ones(4), 0.0, 1e-3, (0.0, 0.99), 1e-8, skip_nonfinite=True, max_norm=1.0)
    bad = np.array([1.0, math.nan, 0.0, 0.0])
    for g in (np.full(4, 0.1), bad, bad, np.full(4, 3.0), bad, np.full(4, 0.2)):
        ref.step(g)
    blk = ref.state_block()
    assert blk[:5] == [3.0, 3.0, 1.0, 0.0, 2.0] and blk[6] == 1.0 / (6.0 + 1e-6) and blk[5] == 2.0 + blk[6] and blk[7] == math.sqrt(0.2 * 0.2 * 4)


# ---------------------------------------------------------------------------------------------- the ABI without a device
def test_entry_points_validate_without_gpu():
    """every refusal happens before a launch; 64 / 128 stand for non-NULL, aligned device pointers that are never followed"""
    lib = native.lib()
    ARG, ALIGN = -5, -3
    ok_guard = dict(row=64, skip=1, max_norm=1.0, lr=1e-3, scale=1.0, table=64, n=4, state=64, ctrl=64)

    def guard(**kw):
        a = dict(ok_guard, **kw)
        return lib.vqk_step_guard(a['row'], a['skip'], a['max_norm'], a['lr'], a['scale'], a['table'], a['n'], a['state'], a['ctrl'], 0)
    for name in ('row', 'table', 'state', 'ctrl'):
        assert guard(**{name: 0}) == ARG, name
    assert guard(max_norm=math.nan) == ARG and guard(max_norm=math.inf) == ARG and guard(max_norm=-math.inf) == ARG
    assert guard(lr=math.nan) == ARG and guard(lr=math.inf) == ARG and guard(scale=math.nan) == ARG
    assert guard(n=0) == ARG and guard(skip=2) == ARG
    assert guard(ctrl=72) == ALIGN and guard(state=68) == ALIGN

    ok = dict(p=64, g=64, m=64, v=64, n=128, seg_end=64, seg_wd=64, nseg=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, ctrl=64, shadow=0)

    def adamw(**kw):
        a = dict(ok, **kw)
        return lib.vqk_adamw_guarded(a['p'], a['g'], a['m'], a['v'], a['n'], a['seg_end'], a['seg_wd'], a['nseg'], a['lr'], a['b1'],
                                     a['b2'], a['eps'], a['ctrl'], a['shadow'], 0)
    for name in ('p', 'g', 'v', 'seg_end', 'seg_wd', 'ctrl'):
        assert adamw(**{name: 0}) == ARG, name
    assert adamw(nseg=0) == ARG and adamw(nseg=-1) == ARG and adamw(n=-1) == ARG
    assert adamw(m=0) == ARG                                          # m == NULL with beta1 != 0
    assert adamw(m=0, b1=0.0, n=0) == 0                               # ... allowed with beta1 == 0 (n == 0: nothing to launch)
    assert adamw(lr=math.nan) == ARG and adamw(lr=math.inf) == ARG
    assert adamw(ctrl=68) == ALIGN
    assert adamw(n=0) == 0
    # the unguarded entry point refuses what it always refused
    assert lib.vqk_adamw(0, 0, 0, 0, 16, 0, 0, 1, 1e-3, 0.0, 0.99, 1e-8, 1, 1.0, 0, 0) == ARG


@pytest.mark.parametrize('betas', [(0.0, 0.99), (0.9, 0.999), (0.5, 0.0)])
def test_bias_table_is_the_host_formula_and_saturates(betas):
    """entry t - 1 holds 1 - (double)(float)beta^t as vqk_adamw computes it; the table ends at the first t where both are exactly 1"""
    table = optim.bias_table(*betas)
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    n = table.shape[0]
    assert table.dtype == torch.float64 and table.shape == (n, 2) and n >= 1
    for t in sorted({1, 2, 3, 10, n // 2 or 1, n - 1 or 1, n}):
        assert table[t - 1, 0].item() == 1.0 - math.pow(b1, t) and table[t - 1, 1].item() == 1.0 - math.pow(b2, t), t
    assert table[n - 1].tolist() == [1.0, 1.0]
    if n > 1:
        assert table[n - 2].tolist() != [1.0, 1.0]
    assert 1.0 - math.pow(b1, n + 1) == 1.0 and 1.0 - math.pow(b2, 10 * n) == 1.0
    lib = native.lib()
    assert lib.vqk_adamw_bias_table(1.0, 0.5, 0, 0) == -1 and lib.vqk_adamw_bias_table(0.5, -0.1, 0, 0) == -1
    assert lib.vqk_adamw_bias_table(0.5, math.nan, 0, 0) == -1
    if betas == (0.0, 0.99):
        assert 3000 < n < 4000                                        # 0.99^t < 2^-54 from t = 3725 on


# ---------------------------------------------------------------------------------------------- optimizer, flags, record
def _cpu_opt():
    w, b = torch.nn.Parameter(torch.randn(8, 4)), torch.nn.Parameter(torch.zeros(8))
    return optim.FlatAdamW([dict(params=[w], weight_decay=1e-2), dict(params=[b], weight_decay=0.0)], lr=1e-3, betas=(0.0, 0.99))


@pytest.mark.parametrize('bad', [0.0, -1.0, math.inf, -math.inf, math.nan])
def test_enable_guard_refuses_bad_clip_values(bad):
    opt = _cpu_opt()
    with pytest.raises(ValueError, match='max_grad_norm'):
        opt.enable_guard(max_grad_norm=bad)
    assert opt.guard is None


def test_guard_is_off_by_default_and_gpu_only():
    opt = _cpu_opt()
    assert opt.guard is None and opt.guard_state() is None and opt.guard_snapshot() is None and opt.guard_epoch_end('autoencoder') is None
    opt.step_count = 7
    assert opt.applied_steps() == 7 and float(opt.state_dict()['state'][0]['step']) == 7.0
    opt.disable_guard()                                               # nothing to free: a no-op
    with pytest.raises(RuntimeError, match='GPU only'):
        opt.enable_guard(skip_nonfinite=True, max_grad_norm=1.0)      # valid settings: there is no CPU path
    assert optim.check_guard_settings(1, None) == (True, None) and optim.check_guard_settings(False, 2) == (False, 2.0)


def test_train_py_flags():
    train = importlib.import_module(PKG + '.train')
    base = ['--params_file', 'x.yaml', '--seed', '0']
    a = train.parse_args(base)
    assert a.skip_nonfinite_steps is False and a.gradient_clip_val is None
    a = train.parse_args(base + ['--skip_nonfinite_steps', '--gradient_clip_val', '0.5'])
    assert a.skip_nonfinite_steps is True and a.gradient_clip_val == 0.5
    a = train.parse_args(base + ['--gradient_clip_val', '2'])
    assert a.skip_nonfinite_steps is False and a.gradient_clip_val == 2.0
    with pytest.raises(SystemExit):
        train.parse_args(base + ['--gradient_clip_val', 'much'])


def test_record_keys_from_a_fake_state_block(tmp_path):
    scalarlog = importlib.import_module(PKG + '.scalarlog')
    before = optim.guard_state_dict([10.0, 1.0, 2.0, 0.0, 1.0, 9.5, 0.25, 3.0])
    now = optim.guard_state_dict([16.0, 5.0, 5.0, 1.0, 3.0, 14.0, 0.5, 7.0])
    assert now == dict(applied=16, skipped=5, clipped=5, consecutive_skipped=1, max_consecutive_skipped=3, clip_coef_sum=14.0,
                       clip_coef_min=0.5, last_norm=7.0)
    rec = optim.guard_epoch_record('autoencoder', now, before)
    assert rec == {'guard/autoencoder/applied': 6, 'guard/autoencoder/skipped': 4, 'guard/autoencoder/clipped': 3,
                   'guard/autoencoder/max_consecutive_skipped': 3, 'guard/autoencoder/clip_coef_mean': 0.75,
                   'guard/autoencoder/clip_coef_min': 0.5}
    first = optim.guard_epoch_record('discriminator', before)         # against a fresh block
    assert first['guard/discriminator/applied'] == 10 and first['guard/discriminator/clip_coef_mean'] == 0.95
    idle = optim.guard_epoch_record('discriminator', now, now)
    assert idle['guard/discriminator/applied'] == 0 and math.isnan(idle['guard/discriminator/clip_coef_mean'])
    # through the log: the keys join the train_epoch record; without them the record is what it was
    log = scalarlog.ScalarLog(str(tmp_path))
    plain = log.epoch_end('train_epoch', 0, 4)
    with_guard = log.epoch_end('train_epoch', 1, 8, {**rec, **idle})
    log.close()
    assert set(with_guard) - set(plain) == set(rec) | set(idle)
    lines = [json.loads(x) for x in open(tmp_path / 'metrics.jsonl', encoding='utf-8').read().splitlines()]
    assert list(lines[0]) == ['event', 'epoch', 'global_step', 'nonfinite_values', 'stats']
    assert lines[1]['guard/autoencoder/skipped'] == 4 and lines[1]['guard/autoencoder/clip_coef_mean'] == 0.75
    assert lines[1]['guard/discriminator/clip_coef_mean'] is None    # JSON has no NaN


def test_trainer_stops_when_an_epoch_skipped_every_step():
    trainer_mod = importlib.import_module(PKG + '.trainer')

    class FakeOpt:
        def __init__(self, rec):
            self.rec = rec

        def guard_epoch_end(self, name):
            return None if self.rec is None else {f'guard/{name}/{k}': v for k, v in self.rec.items()}

        def guard_state(self):
            return dict(last_norm=1.5)

    class Model:
        current_epoch = 3
    tr = trainer_mod.MiniTrainer()
    tr.optimizers = [FakeOpt(None), FakeOpt(None)]
    assert tr.guard_epoch_end(Model()) == {}
    tr.optimizers = [FakeOpt(dict(applied=3, skipped=1)), FakeOpt(dict(applied=0, skipped=0))]      # an idle discriminator is fine
    assert tr.guard_epoch_end(Model())['guard/autoencoder/skipped'] == 1
    tr.optimizers = [FakeOpt(dict(applied=4, skipped=0)), FakeOpt(dict(applied=0, skipped=4))]
    with pytest.raises(RuntimeError, match='every one of the 4 discriminator optimizer steps of epoch 3'):
        tr.guard_epoch_end(Model())
