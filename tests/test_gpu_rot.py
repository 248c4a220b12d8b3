"""The rotation-trick backward on the GPU (csrc/vq_rot.hip: vqk_vq_backward_rot_f32; ``ops.VQLookupFn(..., rotate=True)``;
``quantizer.params.gradient: rotation``) against the float64 reference of tests/rot_reference.py:

1. the raw entry point over N in {1, 31, 32, 33, 257} x D in {4, 6, 8, 64, 256, 260, 1024} at K = 32, four kinds of input, both dq
   dtypes, with and without the loss cotangent and the codebook gradient; every row on one code; N = 4096, K = 1024, D = 256; the
   degenerate case (z = 0, q = 0, z = -q: finite, left out of the comparison).  dz rtol 1e-5 / atol 1e-7, scaled by
   tests/test_rot_cpu.py::bound_scale where the fp32 restatement alone exceeds them on the CPU (nowhere, on these inputs: every scale
   is 1); de rtol 1e-4 / atol 1e-7 (the tolerances of tests/test_gpu_rvq.py).
2. dq == NULL and rows with dq = 0: the bits of the straight-through kernels' dz.
3. ``VQLookupFn`` with and without ``rotate``: the forward and (deterministic mode) de bit for bit, dz different and on the reference.
4. a small VQVAE per quantizer type with ``gradient: rotation`` against the same weights under ``straight_through``; graph capture.
5. the config surface on the device.
THE LOSS SCALARS.  q, idx and hist are compared bit for bit everywhere.  The lookup's loss is sum (q - z)^2 added up by one fp32 atomic
per block of the forward kernel, in arrival order, in deterministic mode too (csrc/vq_filter.hip, csrc/vq.hip::vq_gather_kernel: the
forward this estimator leaves untouched), and so is the reconstruction error of the train step (vqk_sse): with more than two blocks
two runs of the SAME call differ in the last bits, straight-through against straight-through as well.  The loss is therefore
compared bit for bit where the sum cannot depend on the order (at most two blocks: the N = 33 cases of part 3, and the quantizer
loss of part 4, whose 128 rows are two blocks) and within ``SUM_RTOL`` = 1e-6 elsewhere (a reordered fp32 sum of at most 64
non-negative partials moves by at most 63 ulp of 6e-8; the first run of this file on the GPU showed such differences).
Every figure that is asserted with a tolerance is printed first (``ROTMEASURE``)."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import rot_reference as R
from tests.test_rot_cpu import AE, TC, TOL, bf16_round, bound_scale, kept_rows, q_conf

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
BETA = 0.25
SUM_RTOL = 1e-6
_CASES: dict = {}


def case_data(case):
    """the inputs of one case on the host and on the device, built once and shared read-only"""
    if case not in _CASES:
        z, e, idx, g = R.make_case(*case)
        dev = lambda a: torch.from_numpy(a).to(DEV)
        _CASES[case] = dict(z=z, e=e, idx=idx, g=g, zd=dev(z), ed=dev(e), idxd=dev(idx), gd=dev(g), gbd=dev(g).to(torch.bfloat16))
    return _CASES[case]


def close(name, got, want, rtol, atol, scale=1.0):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    worst = float((err / (atol + rtol * np.abs(want))).max()) if err.size else 0.0
    print(f'ROTMEASURE {name}: max abs {err.max() if err.size else 0.0:.3e}, max |want| {np.abs(want).max() if err.size else 0.0:.3e}, '
          f'worst err / (atol + rtol |want|) {worst:.3g} (bound {scale:.3g})')
    assert np.isfinite(got).all(), name
    assert worst <= scale, name


def same_sum(name, a, b, exact):
    """two evaluations of one fp32 sum of block partials: bit for bit where the order cannot matter, within SUM_RTOL elsewhere"""
    a, b = float(a), float(b)
    print(f'ROTMEASURE {name}: {a!r} against {b!r}, relative difference {abs(a - b) / max(abs(b), 1e-300):.3e} ({"exact" if exact else SUM_RTOL})')
    assert a == b if exact else abs(a - b) <= SUM_RTOL * abs(b), name


def raw(fn_name, c, n, k, d, dq, gs, want_de, deterministic=False, cz=R.CZ, ce=R.CE):
    """one call of a backward entry point on the case's device tensors -> (dz, de or None) on the host; dz starts as NaN"""
    dz = torch.full((n, d), float('nan'), device=DEV)
    de = torch.zeros(k, d, device=DEV) if want_de else None
    gsd = torch.full((), gs, device=DEV) if gs is not None else None
    ops.set_deterministic(deterministic)
    try:
        st = ops._stream()                                       # (arms / disarms the library's ordered-sum workspace)
        native.check(getattr(native.lib(), fn_name)(c['zd'].data_ptr(), c['ed'].data_ptr(), c['idxd'].data_ptr(), ops._p(dq),
                                                    ops.dcode(dq.dtype) if dq is not None else ops.F32, n, k, d, cz, ce, ops._p(gsd),
                                                    dz.data_ptr(), ops._p(de), st), fn_name)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
        ops._stream()
    return dz.cpu().numpy(), (de.cpu().numpy() if want_de else None)


def check_raw(case, deterministic=False):
    n, k, d, kind = case
    c, keep = case_data(case), kept_rows(case)
    q = c['e'][c['idx']]
    for dq_name in ('fp32', 'bf16'):
        g = c['g'] if dq_name == 'fp32' else bf16_round(c['g'])
        dq = c['gd'] if dq_name == 'fp32' else c['gbd']
        for gs in (None, R.GS):
            s = 1.0 if gs is None else gs
            dz_ref, de_ref = R.dz(c['z'], q, g, R.CZ * s), R.de(c['z'], c['e'], c['idx'], R.CE * s)
            for want_de in (False, True):
                tag = f'{case} dq {dq_name} gs {gs} de {int(want_de)} det {int(deterministic)}'
                dz, de = raw('vqk_vq_backward_rot_f32', c, n, k, d, dq, gs, want_de, deterministic)
                assert np.isfinite(dz).all(), tag                                    # (the special rows included; no element left unwritten)
                close(f'{tag} dz', dz[keep], dz_ref[keep], *TOL['dz'], scale=bound_scale(kind, d))
                if want_de:
                    close(f'{tag} de', de, de_ref, *TOL['de'])


# ---------------------------------------------------------------------------------------------- 1. the raw kernel against float64
@pytest.mark.parametrize('d', R.DS)
@pytest.mark.parametrize('kind', R.KINDS)
def test_raw_kernel_against_float64(kind, d):
    for n in R.NS:
        check_raw((n, R.K_GRID, d, kind))


@pytest.mark.parametrize('case', [R.ONE_CODE, R.LARGE], ids=['one-code', 'large'])
def test_raw_kernel_one_code_and_large(case):
    check_raw(case)


@pytest.mark.parametrize('case', [(257, R.K_GRID, 256, 'noise0.1'), (257, R.K_GRID, 260, 'noise0.1'), (33, R.K_GRID, 6, 'noise0.3'), R.LARGE], ids=str)
def test_raw_kernel_in_deterministic_mode(case):
    """the ordered form: d == 256 leaves the fused kernel for the row kernel beside the ordered codebook gradient, whose de has the bits of
    the straight-through path"""
    check_raw(case, deterministic=True)
    n, k, d, _ = case
    c = case_data(case)
    for gs in (None, R.GS):
        _, de_rot = raw('vqk_vq_backward_rot_f32', c, n, k, d, c['gd'], gs, True, deterministic=True)
        _, de_st = raw('vqk_vq_backward_f32', c, n, k, d, c['gd'], gs, True, deterministic=True)
        assert np.array_equal(de_rot, de_st)


def test_degenerate_rows_are_finite():
    case = R.DEGENERATE
    assert len(R.SPECIAL_ROWS) <= 3 and int((~kept_rows(case)).sum()) == len(R.SPECIAL_ROWS)
    check_raw(case)
    check_raw(case, deterministic=True)


# ---------------------------------------------------------------------------------------------- 2. no upstream gradient
@pytest.mark.parametrize('d', R.DS)
def test_without_upstream_gradient_dz_is_the_straight_through_dz(d):
    """dq == NULL, and rows of a dq that are zero: the commitment term alone, the bits of the straight-through kernels"""
    for n in (33, 257):
        case = (n, R.K_GRID, d, 'noise0.3')
        c = case_data(case)
        others = ['vqk_vq_backward_f32'] + (['vqk_vq_backward_fused_f32'] if d == 256 else [])
        for gs in (None, R.GS):
            rot, _ = raw('vqk_vq_backward_rot_f32', c, n, R.K_GRID, d, None, gs, False)
            for name in others:
                st, _ = raw(name, c, n, R.K_GRID, d, None, gs, False)
                assert np.array_equal(rot, st), (case, gs, name)
            rows = np.arange(n) % 3 == 0
            for dq in (c['gd'].clone(), c['gbd'].clone()):
                dq[torch.from_numpy(rows).to(DEV)] = 0
                rot_z, _ = raw('vqk_vq_backward_rot_f32', c, n, R.K_GRID, d, dq, gs, False)
                assert np.array_equal(rot_z[rows], rot[rows]), (case, gs, dq.dtype)
                assert not np.array_equal(rot_z[~rows], rot[~rows])


# ---------------------------------------------------------------------------------------------- 3. the autograd function
@pytest.mark.parametrize('deterministic', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('codebook_loss', [True, False], ids=['standard', 'ema'])
@pytest.mark.parametrize('case', [(257, 32, 256, 'noise0.1'), (257, 32, 64, 'noise0.3'), (33, 32, 256, 'noise0.1'), (33, 32, 64, 'noise0.3')], ids=str)
def test_lookup_function_with_and_without_rotation(case, codebook_loss, deterministic):
    n, k, d, kind = case
    c = case_data(case)
    img = lambda t: t.view(1, n, 1, d).permute(0, 3, 1, 2)
    for out_dtype in (torch.float32, torch.bfloat16):
        dq = c['gd'] if out_dtype == torch.float32 else c['gbd']
        g = c['g'] if out_dtype == torch.float32 else bf16_round(c['g'])
        res = {}
        ops.set_deterministic(deterministic)
        try:
            for rotate in (False, True):
                z = c['zd'].clone().requires_grad_(True)
                cb = torch.nn.Parameter(c['ed'].clone(), requires_grad=codebook_loss)
                args = (img(z), cb, BETA, codebook_loss, 0, out_dtype) + ((True,) if rotate else ())      # six arguments: today's call
                q, idx, loss, hist = ops.VQLookupFn.apply(*args)
                assert q.dtype == out_dtype
                grads = torch.autograd.grad([q, loss], [z, cb] if codebook_loss else [z], [img(dq), torch.ones((), device=DEV)])
                torch.cuda.synchronize()
                res[rotate] = dict(q=q.detach(), idx=idx, loss=loss.detach(), hist=hist, dz=grads[0], de=grads[1] if codebook_loss else None)
        finally:
            ops.set_deterministic(False)
            ops._stream()
        st, rot = res[False], res[True]
        tag = f'{case} {"standard" if codebook_loss else "ema"} out {out_dtype} det {int(deterministic)}'
        for name in ('q', 'idx', 'hist'):
            assert torch.equal(st[name], rot[name]), name
        same_sum(f'{tag} loss', rot['loss'], st['loss'], exact=n <= 64)      # (one block per 32 rows at D = 256, per 64 rows otherwise)
        assert not torch.equal(st['dz'], rot['dz'])
        idx = rot['idx'].reshape(-1).cpu().numpy()
        scale = 2.0 / (n * d)
        close(f'{tag} dz', rot['dz'].cpu().numpy(), R.dz(c['z'], c['e'][idx], g, BETA * scale), *TOL['dz'], scale=bound_scale(kind, d))
        close(f'{tag} dz (straight-through)', st['dz'].cpu().numpy(), g.astype(np.float64) + BETA * scale * (c['z'].astype(np.float64) - c['e'][idx]),
              *TOL['dz'])
        if codebook_loss:
            close(f'{tag} de', rot['de'].cpu().numpy(), R.de(c['z'], c['e'], idx, scale), *TOL['de'])
            if deterministic:
                assert torch.equal(st['de'], rot['de'])


# ---------------------------------------------------------------------------------------------- 4. the module and the train step
def _pair(qtype):
    """two models on the same weights: straight-through and rotation"""
    torch.manual_seed(0)
    st = model_mod.VQVAE(32, AE, q_conf(qtype), None, TC).to(DEV).train()
    rot = model_mod.VQVAE(32, AE, q_conf(qtype, gradient='rotation'), None, TC).to(DEV).train()
    missing = rot.load_state_dict(st.state_dict(), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    with torch.no_grad():
        for m in (st, rot):
            m.quantizer.codebook.weight.mul_(32.0)              # codes among the latents: more than one code in use
    return st, rot


@pytest.mark.parametrize('qtype', ['standard', 'ema'])
def test_module_forward_is_unchanged_and_only_the_encoder_gradient_moves(qtype):
    images = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)           # 2 x 8 x 8 = 128 latent rows
    ops.set_deterministic(True)
    try:
        st, rot = _pair(qtype)
        assert rot.quantizer.rotate and not st.quantizer.rotate
        out = {}
        for name, m in (('st', st), ('rot', rot)):
            m.eval()
            with torch.no_grad():
                recon, q_loss, idx = m(m.preprocess_batch(images))
            m.train()
            tr = trainer_mod.MiniTrainer(num_training_batches=1)
            opt = tr.attach(m)[0]
            opt.zero_grad()
            loss = m.training_step(images, 0)
            loss.backward()
            torch.cuda.synchronize()
            out[name] = dict(recon=recon, q_loss=q_loss, idx=idx, loss=loss.detach(), hist=m.quantizer.last_hist,
                             grads={n_: p.grad.detach().clone() for n_, p in m.named_parameters() if p.grad is not None})
    finally:
        ops.set_deterministic(False)
        ops._stream()
    for name in ('recon', 'idx', 'hist'):
        assert torch.equal(out['st'][name], out['rot'][name]), name
    same_sum(f'{qtype} quantizer loss', out['rot']['q_loss'], out['st']['q_loss'], exact=True)
    same_sum(f'{qtype} train loss', out['rot']['loss'], out['st']['loss'], exact=False)
    assert set(out['st']['grads']) == set(out['rot']['grads'])
    moved = 0
    for name, g in out['st']['grads'].items():
        if name.startswith('encoder.'):
            moved += int(not torch.equal(g, out['rot']['grads'][name]))
        else:                                                   # the decoder, and the codebook of the standard quantizer
            assert torch.equal(g, out['rot']['grads'][name]), name
    n_enc = sum(name.startswith('encoder.') for name in out['st']['grads'])
    print(f'ROTMEASURE {qtype}: {moved} of {n_enc} encoder gradients differ between the estimators; '
          f'{int((out["st"]["hist"] > 0).sum())} codes in use')
    assert moved > n_enc // 2 and not torch.equal(out['st']['grads']['encoder.conv_out.weight'], out['rot']['grads']['encoder.conv_out.weight'])


@pytest.mark.parametrize('qtype', ['standard', 'ema'])
def test_graph_replay_matches_eager_with_rotation(qtype):
    """MiniTrainer.capture + two replays against eager steps on the same trajectory (the tolerance of
    tests/test_gpu_train_step.py::test_graph_replay_matches_eager)"""
    tc = dict(TC, lr=1e-3)
    images = torch.rand(4, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    losses, state = {}, {}
    for mode in ('eager', 'graph'):
        torch.manual_seed(0)
        m = model_mod.VQVAE(32, AE, q_conf(qtype, gradient='rotation'), None, tc).to(DEV).train()
        tr = trainer_mod.MiniTrainer(num_training_batches=100)
        tr.attach(m)
        m.on_train_start()
        if mode == 'graph':
            tr.capture(m, images, warmup=2)
            out = [tr.train_batch_graphed(m, images, 2 + i).item() for i in range(2)]
        else:
            out = [tr.train_batch(m, images, i).item() for i in range(4)][2:]
        losses[mode] = out
        state[mode] = {k: v.detach().float().cpu().clone() for k, v in m.quantizer.state_dict().items()}
    print(f'ROTMEASURE {qtype} graph {losses["graph"]} eager {losses["eager"]}')
    np.testing.assert_allclose(losses['graph'], losses['eager'], rtol=2e-3)
    if qtype == 'ema':
        for k in ('ema_count', 'ema_weight', 'codebook.weight'):
            np.testing.assert_allclose(state['graph'][k].numpy(), state['eager'][k].numpy(), rtol=2e-3, atol=1e-5)


# ---------------------------------------------------------------------------------------------- 5. config
def test_config_on_the_device():
    train = importlib.import_module(PKG + '.train')
    with pytest.raises(ValueError, match='quantizer.params.gradient'):
        model_mod.VQVAE(32, AE, q_conf('standard', gradient='rotated'), None, TC)
    with pytest.raises(ValueError, match="'standard' and 'ema' quantizers only"):
        model_mod.VQVAE(32, AE, q_conf('residual', gradient='rotation', depth=2), None, TC)
    assert model_mod.VQVAE(32, AE, q_conf('ema'), None, TC).quantizer.rotate is False
    run = train.derive_run_config(train.get_model_conf(os.path.join(ROOT, 'example_confs', 'rotation_vqvae.yaml')), 1,
                                  {'image_size': 32, 'autoencoder.channels': 32, 'autoencoder.num_res_blocks': 1,
                                   'autoencoder.channel_multipliers': [1, 2], 'quantizer.num_embeddings': 64, 'training.cumulative_bs': 4})
    m = model_mod.VQVAE(run['image_size'], run['ae_conf'], run['q_conf'], run['l_conf'], run['t_conf']).to(DEV).train()
    assert m.quantizer.rotate is True and m.quantizer.embedding_dim == 256
    tr = trainer_mod.MiniTrainer(num_training_batches=1)
    tr.attach(m)
    loss = tr.train_batch(m, torch.rand(4, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV), 0)
    assert np.isfinite(loss.item())
