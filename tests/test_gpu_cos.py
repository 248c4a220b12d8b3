"""The cosine quantizer on the GPU (csrc/vq_cos.hip, _ops_cos.py, CosineVectorQuantizer).

1. The fused kernel equals the staged formulation (ops.cos_staged: vqk_l2norm_rows_f32 + ops.vq_assign + vqk_vq_gather_f32) BIT FOR
   BIT -- indices, q as fp32 and bf16, hist, and in deterministic mode the loss -- on every case: both evaluate the same fp32
   expression sequence, any difference is a bug (normalisation in LDS, tile walk, reduction, epilogue mapping).
2. Float64 acceptance (tests/cos_reference.py::check_acceptance) on every row: within 2 eta of the float64 minimum on the
   float64-normalised rows, equal to the float64 argmin where the runner-up is more than 2 eta away; eta = rvq_reference.eta(1, 1).
   tests/test_cos_cpu.py shows that >= 99 % of the scale-1 rows are separated, so the equality branch carries it.
3. loss, dz, de against the float64 closed forms on the kernel's indices at the tolerances of tests/test_gpu_rvq.py (loss rtol 1e-5;
   dz rtol 1e-5 / atol 1e-7; de rtol 1e-4 / atol 1e-7), scaled by tests/test_cos_cpu.py::bound_scale where the fp32 restatement
   itself exceeds them on the CPU ((init, de): 5.2; (collapsed, dz): 4.52; 1 everywhere else).  Clamped rows (|x| < eps) are
   asserted finite and left out of the comparison.
The inputs (tests/cos_reference.py) are shared with the CPU tests; every figure that is asserted with a tolerance is printed first
(``COSMEASURE``)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import cos_reference as C
from tests.test_cos_cpu import RESTATEMENT, TOL, bound_scale

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
vqm = importlib.import_module(PKG + '.modules.vector_quantizers')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
BETA = 0.25
IDS = lambda c: f'N{c[0]}-K{c[1]}-D{c[2]}-{c[3]}'
_FWD: dict = {}


def dev_case(case):
    z, e = C.make_case(*case)
    return z.to(DEV), e.to(DEV)


def img(t):
    n, d = t.shape
    return t.view(1, n, 1, d).permute(0, 3, 1, 2)


def rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def lookup(case, fused_on: bool, deterministic: bool):
    """forward of one case through CosLookupFn as fp32 and bf16 output"""
    z, e = dev_case(case)
    saved = ops.COS_FUSED
    ops.COS_FUSED = fused_on
    ops.set_deterministic(deterministic)
    try:
        assert ops.cos_fused_serves(e) == fused_on
        with torch.no_grad():
            q32, idx, loss, hist = ops.CosLookupFn.apply(img(z), e, BETA, torch.float32)
            qlo, idx2, loss2, hist2 = ops.CosLookupFn.apply(img(z), e, BETA, torch.bfloat16)
        torch.cuda.synchronize()
    finally:
        ops.COS_FUSED = saved
        ops.set_deterministic(False)
    assert torch.equal(idx, idx2) and torch.equal(hist, hist2)
    if deterministic:
        assert torch.equal(loss, loss2)
    return dict(idx=idx.view(-1), q32=rows(q32), qlo=rows(qlo), loss=loss, hist=hist)


def fused(case):
    """the fused forward of one case in default mode, computed once and shared read-only"""
    if case not in _FWD:
        _FWD[case] = lookup(case, True, False)
    return _FWD[case]


def close(name, got, want, rtol, atol=0.0, scale=1.0):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return
    err = np.abs(got - want)
    allowed = scale * (atol + rtol * np.abs(want))
    print(f'COSMEASURE {name}: max abs {err.max():.3e}, max |want| {np.abs(want).max():.3e}, worst err / (atol + rtol |want|) '
          f'{(err / (atol + rtol * np.abs(want) + 1e-300)).max():.3g} (allowed {scale:.3g})')
    assert bool((err <= allowed).all()), name


# ---------------------------------------------------------------------------------------------- 1. fused == staged, bit for bit
@pytest.mark.parametrize('case', C.cases(), ids=IDS)
def test_fused_equals_staged_bit_for_bit(case):
    n, k, d, kind = case
    z, e = dev_case(case)
    f, s = lookup(case, True, True), lookup(case, False, True)
    assert torch.equal(f['idx'], s['idx'])
    assert torch.equal(f['q32'], s['q32']) and f['q32'].dtype == torch.float32
    assert torch.equal(f['qlo'], s['qlo']) and f['qlo'].dtype == torch.bfloat16
    assert torch.equal(f['hist'], s['hist']) and f['hist'].dtype == torch.int32 and int(f['hist'].sum()) == n
    assert torch.equal(f['loss'], s['loss'])                      # deterministic mode: the same block partials in the same order
    # the staged operators themselves, and the default mode (the sums arrive in another order)
    idx_s, q_s, qlo_s, sse_s, hist_s, zn, inv_z = ops.cos_staged(z, e, want_lo=True)
    d0 = fused(case)
    assert torch.equal(d0['idx'], idx_s) and torch.equal(d0['q32'], q_s) and torch.equal(d0['qlo'], qlo_s) and torch.equal(d0['hist'], hist_s)
    assert torch.equal(f['idx'], idx_s)
    assert torch.equal(ops.cos_assign(z, e), idx_s)
    assert torch.equal(hist_s, torch.bincount(idx_s, minlength=k).to(torch.int32))
    close('loss default vs deterministic', d0['loss'].item(), f['loss'].item(), rtol=1e-5)
    close('sse staged vs fused', (sse_s * ((1.0 + BETA) / (n * d))).item(), f['loss'].item(), rtol=1e-5)
    # the stand-alone normalisation: the rows the staged path ranks are unit rows (or zero), the workspace holds the same for e
    norms = zn.double().norm(dim=1)
    live = ~C.clamped(C.make_case(*case)[0]).to(DEV)
    assert float((norms[live] - 1.0).abs().max()) < 4e-7 if bool(live.any()) else True
    assert float(norms[~live].max()) == 0.0 if bool((~live).any()) else True
    assert torch.equal(ops.l2norm_rows(e)[f['idx']], f['q32'])
    if kind == 'collapsed':
        assert int(f['idx'].max()) < 4                            # exact ties: the smallest index wins


# ---------------------------------------------------------------------------------------------- 2. float64 acceptance
@pytest.mark.parametrize('case', C.cases(), ids=IDS)
def test_float64_acceptance(case):
    z, e = C.make_case(*case)
    idx = fused(case)['idx'].cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < case[1]
    separated = C.check_acceptance(z, e, idx)
    print(f'COSMEASURE {IDS(case)}: separated rows {separated:.4f}')
    if case[3] == 'scale1':
        assert separated >= 0.99
    if case[3] == 'collapsed':
        assert int(idx.max()) < 4                                 # the smallest index among bitwise-equal rows
    if case[3] == 'zero':
        assert int(idx[0]) == 3                                   # the zero latent takes the zero code (distance 0 against 1)


# ---------------------------------------------------------------------------------------------- 3. loss, dz, de
def _grads(case, dq_name, deterministic=False, arena=False):
    n, k, d, _ = case
    z, e = dev_case(case)
    x = img(z).detach().requires_grad_(True)
    cb = e.detach().clone().requires_grad_(True)
    if arena:                                                     # what FlatAdamW does to its parameters: the kernels add into .grad
        cb.grad = torch.zeros_like(cb)
        cb._vqk_direct_grad = True
    dq = None
    if dq_name != 'none':
        dq = torch.randn(n, d, generator=torch.Generator().manual_seed(11)).to(DEV)
        dq = dq.to(torch.bfloat16) if dq_name == 'bf16' else dq
    ops.set_deterministic(deterministic)
    try:
        q, idx, loss, _ = ops.CosLookupFn.apply(x, cb, BETA, torch.bfloat16 if dq_name == 'bf16' else torch.float32)
        outs, gouts = [loss], [torch.ones((), device=DEV)]
        if dq is not None:
            outs.append(q), gouts.append(img(dq))
        dz, de = torch.autograd.grad(outs, [x, cb], gouts, allow_unused=True)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
    if arena:
        assert de is None
        de = cb.grad
    return dict(idx=idx.view(n), loss=loss, dz=rows(dz), de=de, dq=None if dq is None else dq.float().cpu())


@pytest.mark.parametrize('dq_name', ['fp32', 'bf16', 'none'])
@pytest.mark.parametrize('case', C.cases(), ids=IDS)
def test_loss_and_gradients_against_float64(case, dq_name):
    kind = case[3]
    z, e = C.make_case(*case)
    kz, ke = ~C.clamped(z), ~C.clamped(e)
    ref = None
    for deterministic in (False, True):
        for arena in (False, True):
            g = _grads(case, dq_name, deterministic, arena)
            assert torch.equal(g['idx'], fused(case)['idx'])
            if ref is None:
                ref = C.gradients(z, e, g['idx'].cpu(), g['dq'], BETA)
            loss, _, dz, de = ref
            tag = f'{IDS(case)} dq {dq_name} det {int(deterministic)} arena {int(arena)}'
            got_dz, got_de = g['dz'].cpu(), g['de'].cpu()
            assert bool(torch.isfinite(got_dz).all()) and bool(torch.isfinite(got_de).all()) and bool(torch.isfinite(g['loss']))
            close(f'{tag} loss', g['loss'].item(), loss.item(), *TOL['loss'], scale=bound_scale(kind, 'loss'))
            close(f'{tag} dz', got_dz[kz], dz[kz], *TOL['dz'], scale=bound_scale(kind, 'dz'))
            close(f'{tag} de', got_de[ke], de[ke], *TOL['de'], scale=bound_scale(kind, 'de'))


def test_backward_takes_an_out_of_range_token_as_a_zero_code():
    """vqk_cos_backward_f32 on tokens the forward never writes (outside [0, K)): q = 0 for that row and no code row receives its term
    -- the float64 closed forms on a codebook extended by a zero row that stands in for such a token.  Default (LDS chains + atomics)
    and deterministic mode (per-row terms + ordered sums); a ragged last block; the tolerances of part 3."""
    case = (67, 64, 16, 'scale1')
    n, k, d, kind = case
    z, e = C.make_case(*case)
    zd, ed = dev_case(case)
    idx = fused(case)['idx'].clone()
    for row, bad in zip((0, 33, 40, n - 1), (-1, k, 2 ** 40 + 3, -2 ** 62)):
        idx[row] = bad
    ok = (idx >= 0) & (idx < k)
    assert int((~ok).sum()) == 4
    dq = torch.randn(n, d, generator=torch.Generator().manual_seed(11))
    _, _, dz_ref, de_ref = C.gradients(z, torch.cat([e, torch.zeros(1, d)]), torch.where(ok, idx, k).cpu(), dq, BETA)
    lib, s = native.lib(), torch.cuda.current_stream().cuda_stream
    dqd, gs = dq.to(DEV), torch.ones((), device=DEV)
    cz, ce = 2.0 * BETA / (n * d), 2.0 / (n * d)
    ws = ops.cos_prepared(ed)
    ws2 = torch.empty(lib.vqk_cos_backward_ws_bytes(n, d), dtype=torch.uint8, device=DEV)
    for deterministic in (False, True):
        dz, de = torch.empty(n, d, device=DEV), torch.zeros(k, d, device=DEV)
        ops.set_deterministic(deterministic)
        try:
            native.check(lib.vqk_cos_backward_f32(zd.data_ptr(), ws.data_ptr(), idx.data_ptr(), dqd.data_ptr(), ops.F32, n, k, d, cz, ce,
                                                  gs.data_ptr(), dz.data_ptr(), de.data_ptr(), ws2.data_ptr(), ws2.numel(), s),
                         'cos_backward')
            torch.cuda.synchronize()
        finally:
            ops.set_deterministic(False)
        close(f'bad token det {int(deterministic)} dz', dz.cpu(), dz_ref, *TOL['dz'], scale=bound_scale(kind, 'dz'))
        close(f'bad token det {int(deterministic)} de', de.cpu(), de_ref[:k], *TOL['de'], scale=bound_scale(kind, 'de'))


# ---------------------------------------------------------------------------------------------- 4. deterministic mode
@pytest.mark.parametrize('kind', ['scale1', 'collapsed'])
def test_deterministic_backward_is_reproducible(kind):
    case = (2051, 1024, 32, kind)
    a, b = _grads(case, 'fp32', deterministic=True), _grads(case, 'fp32', deterministic=True)
    assert torch.equal(a['dz'], b['dz']) and torch.equal(a['de'], b['de']) and torch.equal(a['idx'], b['idx'])
    assert torch.equal(a['loss'], b['loss'])
    d = _grads(case, 'fp32')
    assert torch.equal(a['idx'], d['idx']) and torch.equal(a['dz'], d['dz'])          # dz holds no sum over rows


# ---------------------------------------------------------------------------------------------- 5. decode
@pytest.mark.parametrize('case', [c for c in C.cases() if c[:3] in ((67, 64, 16), (2051, 8192, 8))], ids=IDS)
def test_decode_has_the_forwards_bits(case):
    n, k, d, _ = case
    z, e = dev_case(case)
    f = fused(case)
    for dtype, key in ((torch.float32, 'q32'), (torch.bfloat16, 'qlo')):
        dec = ops.cos_decode(f['idx'].view(1, n), e, dtype)
        assert dec.dtype == dtype and tuple(dec.shape) == (1, n, d) and torch.equal(dec[0], f[key])
    # a token outside [0, K) reads nothing and gives a zero row; the other rows are untouched
    row = n // 2
    for bad in (-1, k, 2 ** 40 + 3, -2 ** 62):
        wild = f['idx'].clone()
        wild[row] = bad
        out = ops.cos_decode(wild, e)
        assert float(out[row].abs().max()) == 0.0
        keep = torch.arange(n, device=DEV) != row
        assert torch.equal(out[keep], f['q32'][keep])
    # the module over the same codebook
    quant = vqm.CosineVectorQuantizer(k, d, BETA).to(DEV)
    with torch.no_grad():
        quant.codebook.weight.copy_(e)
        codes = quant.vec_to_codes(img(z))
        assert tuple(codes.shape) == (1, n) and torch.equal(codes[0], f['idx'])
        assert torch.equal(quant.codes_to_vec(codes)[0], f['q32'])
        q, idx, _ = quant(img(z))
        assert torch.equal(rows(q), f['q32']) and torch.equal(idx.view(-1), f['idx']) and torch.equal(quant.last_hist, f['hist'])


def test_staged_serves_the_other_shapes():
    """D = 24 (no fused instantiation), K = 40 (not a multiple of 32) and D = 256 (vq_assign's filter path) go through cos_staged and the
    torch backward; checked against float64 like the fused path"""
    for n, k, d in ((67, 40, 16), (67, 64, 24), (67, 64, 256)):
        g = torch.Generator().manual_seed(5 + d)
        z, e = torch.randn(n, d, generator=g), torch.randn(k, d, generator=g)
        dq = torch.randn(n, d, generator=g)
        cb = e.to(DEV).requires_grad_(True)
        assert not ops.cos_fused_serves(cb)
        x = img(z.to(DEV)).detach().requires_grad_(True)
        q, idx, loss, hist = ops.CosLookupFn.apply(x, cb, BETA, torch.float32)
        dz, de = torch.autograd.grad([loss, q], [x, cb], [torch.ones((), device=DEV), img(dq.to(DEV))])
        idx = idx.view(-1).cpu()
        C.check_acceptance(z, e, idx)
        assert torch.equal(ops.cos_decode(idx.to(DEV), cb), rows(q)) and int(hist.sum()) == n
        rl, _, rdz, rde = C.gradients(z, e, idx, dq, BETA)
        # this backward IS the restatement's arithmetic (fp32 torch operations): 4 x its worst recorded figure per quantity
        worst = {name: 4.0 * max(1.0, max(v for (_, q_), v in RESTATEMENT.items() if q_ == name)) for name in TOL}
        close(f'staged D{d} K{k} loss', loss.item(), rl.item(), *TOL['loss'], scale=worst['loss'])
        close(f'staged D{d} K{k} dz', rows(dz).cpu(), rdz, *TOL['dz'], scale=worst['dz'])
        close(f'staged D{d} K{k} de', de.cpu(), rde, *TOL['de'], scale=worst['de'])


# ---------------------------------------------------------------------------------------------- 6. model level
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)


def _qc(dim, init=None):
    conf = dict(num_embeddings=64, embedding_dim=dim, reinit_every_n_epochs=None, type='cosine', params=dict(commitment_cost=0.25))
    if init:
        conf['codebook_init'] = init
    return conf


def _images(seed=3, b=4):
    return torch.rand(b, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize('dtype,dim', [(torch.float32, 8), (torch.bfloat16, 8), (torch.float32, 32), (torch.bfloat16, 32)],
                         ids=['fp32-D8', 'bf16-D8', 'fp32-D32', 'bf16-D32'])
def test_model_step_tokens_roundtrip_and_checkpoint(dtype, dim, tmp_path):
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, AE, _qc(dim), None, TC, compute_dtype=dtype).to(DEV).train()
    assert ops.cos_fused_serves(m.quantizer.codebook.weight)
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    m.on_train_start()
    images = _images()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss = tr.train_batch(m, images, 0)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and float(m.logged['train/quant_loss']) > 0.0
    qz = m.quantizer
    assert qz.last_hist.numel() == 64 and int(qz.last_hist.sum()) == 4 * 64
    assert int(m.train_epoch_usage_count.sum()) == 4 * 64
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert {'quantizer.codebook.weight', 'encoder.conv_in.weight', 'decoder.conv_out.weight'} <= changed

    m.eval()
    with torch.no_grad():
        tokens = m.get_tokens(images)
        assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (4, 64)
        vec = m.quantize(images)
        assert tuple(vec.shape) == (4, 64, dim) and float((vec.double().norm(dim=-1) - 1.0).abs().max()) < 4e-7      # the normalised codes
        # (the autoencoder's GroupNorm sums are combined in arrival order by default: bits are compared in deterministic mode)
        ops.set_deterministic(True)
        try:
            tokens_det = m.get_tokens(images)
            assert torch.equal(m.reconstruct_from_tokens(tokens_det), m.reconstruct(images))
        finally:
            ops.set_deterministic(False)
        usage = qz.get_codebook_usage(m.train_epoch_usage_count.float())[0]
        dead = usage == 0
        book = qz.codebook.weight.detach().clone()
        qz.reinit_unused_codes(usage)
        assert torch.equal(qz.codebook.weight[~dead], book[~dead])
        if bool(dead.any()):
            live = book[~dead]
            assert all(bool((live == row).all(1).any()) for row in qz.codebook.weight[dead])
        ops.refresh_vq_prepared()
        tokens = m.get_tokens(images)
        assert torch.equal(qz.codes_to_vec(tokens), ops.l2norm_rows(qz.codebook.weight)[tokens])     # the refreshed workspace
    path = str(tmp_path / 'cos.ckpt')
    tr.save_checkpoint(m, path)
    torch.manual_seed(1)
    m2 = model_mod.VQVAE(32, AE, _qc(dim), None, TC, compute_dtype=dtype).to(DEV)
    t2 = trainer_mod.MiniTrainer(num_training_batches=10)
    t2.attach(m2)
    t2.load_checkpoint(m2, path)
    m2.eval()
    assert torch.equal(m2.quantizer.codebook.weight, m.quantizer.codebook.weight)
    assert torch.equal(m2.get_tokens(images), tokens)


@pytest.mark.parametrize('dim', [8, 32])
def test_codebook_init_runs(dim):
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, AE, _qc(dim, init=dict(method='kmeans', samples=256, iters=2)), None, TC).to(DEV).train()
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    before = m.quantizer.codebook.weight.detach().clone()
    info = m.init_codebook_from_batches([_images(seed=s) for s in range(2)], seed=0)
    w = m.quantizer.codebook.weight.detach()
    assert info['samples'] == 256 and bool(torch.isfinite(w).all()) and not torch.equal(w, before)
    assert float(w.double().norm(dim=1).max()) <= 1.0 + 1e-6      # centres of unit rows lie in the unit ball
    with torch.no_grad():
        tokens = m.eval().get_tokens(_images())
        assert torch.equal(m.quantizer.codes_to_vec(tokens), ops.l2norm_rows(w)[tokens])            # the workspace followed the in-place write


# ---------------------------------------------------------------------------------------------- 7. graph replay
@pytest.mark.parametrize('deterministic', [True, False], ids=['deterministic', 'default'])
def test_captured_forward_backward_replays(deterministic):
    n, k, d = 2051, 1024, 32
    z0, e0 = dev_case((n, k, d, 'scale1'))
    gen = torch.Generator().manual_seed(23)
    dq0 = torch.randn(n, d, generator=gen).to(DEV)
    step = (torch.randn(k, d, generator=gen) * 0.5).to(DEV)               # what optimizer steps do to the codebook

    def run(z, cb, dq):
        q, idx, loss, hist = ops.CosLookupFn.apply(img(z), cb, BETA, torch.float32)
        dz, de = torch.autograd.grad([q, loss], [z, cb], [img(dq), torch.ones((), device=DEV)])
        return q, idx, loss, hist, dz, de

    ops.set_deterministic(deterministic)
    try:
        cb = torch.nn.Parameter(e0.clone())
        z = z0.clone().requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(z, cb, dq0)                                               # first launches, workspaces and the prepared codebook: outside
            torch.cuda.synchronize()
            graph, update = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                got = run(z, cb, dq0)
            with torch.cuda.graph(update, stream=side):
                with torch.no_grad():
                    cb.add_(step)
        torch.cuda.current_stream().wait_stream(side)
        for round_ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            replayed = [t.detach().clone() for t in got]
            want = run(z, cb, dq0)
            torch.cuda.synchronize()
            for name, a, b in zip(('q', 'idx', 'loss', 'hist', 'dz', 'de'), replayed, want):
                if deterministic or name in ('q', 'idx', 'hist', 'dz'):
                    assert torch.equal(a, b), (round_, name)
                else:
                    close(f'replay {round_} {name}', a.cpu(), b.detach().cpu(), rtol=1e-5 if name == 'loss' else 1e-4,
                          atol=0.0 if name == 'loss' else 1e-7)
            if round_ == 0:
                first_idx = replayed[1]
                update.replay()                                           # the codebook changes under the captured step ...
                ops.refresh_vq_prepared(data_ptr=cb.data_ptr())           # ... and the prepared workspace follows, as after an optimizer step
        assert not torch.equal(first_idx, replayed[1])                    # the second replay ranked against the NEW codebook
    finally:
        ops.set_deterministic(False)


# ---------------------------------------------------------------------------------------------- 8. entry points
SMALL = ['--set', 'image_size=32', '--set', 'autoencoder.channels=32', '--set', 'autoencoder.num_res_blocks=1',
         '--set', 'autoencoder.channel_multipliers=[1, 2]', '--set', 'quantizer.num_embeddings=64', '--set', 'training.cumulative_bs=4']


def test_entry_points(tmp_path, capsys):
    train = importlib.import_module(PKG + '.train')
    ev = importlib.import_module(PKG + '.evaluate')
    conf = os.path.join(ROOT, 'example_confs', 'cosine_vqvae.yaml')
    common = ['--params_file', conf] + SMALL + ['--max_epochs', '1', '--batches_per_epoch', '2', '--seed', '0', '--dtype', 'f32']
    capsys.readouterr()
    loss = train.main(common + ['--save_path', str(tmp_path), '--run_name', 'cos'])
    out = capsys.readouterr().out
    assert loss is not None and np.isfinite(loss)
    assert 'eager launches' not in out                                                  # the graph was captured, not given up
    ckpt = str(tmp_path / 'cos' / 'epoch=00.ckpt')
    assert os.path.exists(ckpt)
    small = tmp_path / 'conf.yaml'
    small.write_text('image_size: 32\nautoencoder:\n  channels: 32\n  num_res_blocks: 1\n  channel_multipliers: [1, 2]\n'
                     'quantizer:\n  num_embeddings: 64\n  embedding_dim: 32\n  type: cosine\n  params:\n'
                     '    commitment_cost: 0.25\n  reinit_every_n_epochs:\n')
    pt = str(tmp_path / 'test.pt')
    torch.save(torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(5)), pt)
    capsys.readouterr()
    res = ev.main(['--params_file', str(small), '--batch_size', '4', '--seed', '0', '--loading_path', ckpt, '--dtype', 'f32',
                   '--dataset_path', pt])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert json.loads(lines[-1]) == res
    assert {'mse', 'psnr', 'ssim', 'used_codebook', 'perplexity'} <= set(res)
    assert 0.0 < res['used_codebook'] <= 100.0 and 1.0 <= res['perplexity'] <= 64.0
