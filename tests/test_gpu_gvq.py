"""The grouped quantizer on the GPU (csrc/gvq.hip, _ops_gvq.py, GroupedVectorQuantizer).

1. The fused forward equals the staged formulation (ops.gvq_staged: per group a contiguous slice copy, ops.vq_assign and
   vqk_vq_gather_f32) BIT FOR BIT in the indices, q as fp32 and bf16 and hist, with ``ops.GVQ_FUSED`` on against off, on every case:
   both evaluate the same fp32 expression sequence, any difference is a bug (pitch, slab, tile walk, epilogue slot).  The loss: rtol
   1e-5 against staged (the block partials are added in another order), bit-identical between two deterministic runs.
2. Float64 acceptance (tests/gvq_reference.py::check_acceptance) on every (row, group): within 2 eta of the float64 minimum, equal to
   the float64 argmin where the runner-up is more than 2 eta away.  tests/test_gvq_cpu.py shows that >= 99 % of the scale-1 pairs are
   separated, so the equality branch carries it.
3. loss, dz, de against the float64 closed forms on the kernel's indices at the tolerances of tests/test_gpu_rvq.py (loss rtol 1e-5;
   dz rtol 1e-5 / atol 1e-7; de rtol 1e-4 / atol 1e-7) times tests/test_gvq_cpu.py::bound_scale (1 everywhere: the fp32 restatement
   stays below 0.1 of them on the CPU).
4. groups = 1 against ops.VQLookupFn on the same [K, D] codebook.  5. Decode.  6. The staged product path (d = 24, K = 40).
7. Model, checkpoint, re-initialisation, k-means start, graph replay, train.py / evaluate.py.
The inputs (tests/gvq_reference.py) are shared with the CPU tests; every figure that is asserted with a tolerance is printed first
(``GVQMEASURE``)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import gvq_reference as G
from tests.test_gvq_cpu import RESTATEMENT, TOL, bound_scale

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
IDS = lambda c: f'N{c[0]}-K{c[1]}-d{c[2]}-G{c[3]}-{c[4]}'
_FWD: dict = {}


def dev_case(case):
    z, e = G.make_case(*case)
    return z.to(DEV), e.to(DEV)


def img(t):
    n, d = t.shape
    return t.view(1, n, 1, d).permute(0, 3, 1, 2)


def rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def lookup(case, fused_on: bool, deterministic: bool):
    """forward of one case through GVQLookupFn as fp32 and bf16 output"""
    groups = case[3]
    z, e = dev_case(case)
    saved = ops.GVQ_FUSED
    ops.GVQ_FUSED = fused_on
    ops.set_deterministic(deterministic)
    try:
        assert ops.gvq_fused_serves(e, groups) == fused_on
        with torch.no_grad():
            q32, idx, loss, hist = ops.GVQLookupFn.apply(img(z), e, BETA, groups, torch.float32)
            qlo, idx2, loss2, hist2 = ops.GVQLookupFn.apply(img(z), e, BETA, groups, torch.bfloat16)
        torch.cuda.synchronize()
    finally:
        ops.GVQ_FUSED = saved
        ops.set_deterministic(False)
    assert tuple(idx.shape) == (1, case[0], groups) and idx.dtype == torch.int64
    assert torch.equal(idx, idx2) and torch.equal(hist, hist2)
    if deterministic and fused_on:
        assert torch.equal(loss, loss2)
    return dict(idx=idx.view(-1, groups), q32=rows(q32), qlo=rows(qlo), loss=loss, hist=hist)


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
    print(f'GVQMEASURE {name}: max abs {err.max():.3e}, max |want| {np.abs(want).max():.3e}, worst err / (atol + rtol |want|) '
          f'{(err / (atol + rtol * np.abs(want) + 1e-300)).max():.3g} (allowed {scale:.3g})')
    assert bool((err <= allowed).all()), name


# ---------------------------------------------------------------------------------------------- 1. fused == staged, bit for bit
@pytest.mark.parametrize('case', G.cases(), ids=IDS)
def test_fused_equals_staged_bit_for_bit(case):
    n, k, d, groups, kind = case
    z, e = dev_case(case)
    f, s = lookup(case, True, True), lookup(case, False, True)
    f2 = lookup(case, True, True)
    assert torch.equal(f['idx'], s['idx'])
    assert torch.equal(f['q32'], s['q32']) and f['q32'].dtype == torch.float32 and tuple(f['q32'].shape) == (n, groups * d)
    assert torch.equal(f['qlo'], s['qlo']) and f['qlo'].dtype == torch.bfloat16
    assert torch.equal(f['hist'], s['hist']) and f['hist'].dtype == torch.int32 and tuple(f['hist'].shape) == (groups * k,)
    assert int(f['hist'].sum()) == n * groups
    assert torch.equal(f['loss'], f2['loss'])                     # deterministic mode: the same block partials in the same order
    close('loss fused vs staged', f['loss'].item(), s['loss'].item(), rtol=1e-5)
    # the staged operators themselves, and the default mode (the sums arrive in another order)
    idx_s, q_s, qlo_s, sse_s, hist_s = ops.gvq_staged(z, e, groups, want_lo=True)
    d0 = fused(case)
    assert torch.equal(d0['idx'], idx_s) and torch.equal(d0['q32'], q_s) and torch.equal(d0['qlo'], qlo_s) and torch.equal(d0['hist'], hist_s)
    assert torch.equal(ops.gvq_assign(z, e, groups), idx_s)
    assert torch.equal(hist_s.cpu(), G.hist(idx_s.cpu(), k).to(torch.int32))
    assert torch.equal(q_s.cpu(), G.decode(idx_s.cpu(), e.cpu()))
    close('loss default vs deterministic', d0['loss'].item(), f['loss'].item(), rtol=1e-5)
    close('sse staged vs fused', (sse_s * ((1.0 + BETA) / (n * groups * d))).item(), f['loss'].item(), rtol=1e-5)
    if kind == 'collapsed':
        assert int(f['idx'].max()) < 4                            # exact ties: the smallest index wins


# ---------------------------------------------------------------------------------------------- 2. float64 acceptance
@pytest.mark.parametrize('case', G.cases(), ids=IDS)
def test_float64_acceptance(case):
    n, k, d, groups, kind = case
    z, e = G.make_case(*case)
    idx = fused(case)['idx'].cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < k
    separated = G.check_acceptance(z, e, idx, groups)
    print(f'GVQMEASURE {IDS(case)}: separated (row, group) pairs {separated:.4f}')
    if kind == 'scale1':
        assert separated >= 0.99
    if kind == 'collapsed':
        assert int(idx.max()) < 4                                 # the smallest index among bitwise-equal rows


# ---------------------------------------------------------------------------------------------- 3. loss, dz, de
def _grads(case, dq_name, deterministic=False, arena=False):
    n, k, d, groups, _ = case
    z, e = dev_case(case)
    x = img(z).detach().requires_grad_(True)
    cb = e.detach().clone().requires_grad_(True)
    if arena:                                                     # what FlatAdamW does to its parameters: the kernels add into .grad
        cb.grad = torch.zeros_like(cb)
        cb._vqk_direct_grad = True
    dq = None
    if dq_name != 'none':
        dq = torch.randn(n, groups * d, generator=torch.Generator().manual_seed(11)).to(DEV)
        dq = dq.to(torch.bfloat16) if dq_name == 'bf16' else dq
    ops.set_deterministic(deterministic)
    try:
        assert ops.gvq_fused_serves(cb, groups)
        q, idx, loss, _ = ops.GVQLookupFn.apply(x, cb, BETA, groups, torch.bfloat16 if dq_name == 'bf16' else torch.float32)
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
    assert tuple(de.shape) == (groups * k, d)
    return dict(idx=idx.view(n, groups), loss=loss, dz=rows(dz), de=de, dq=None if dq is None else dq.float().cpu())


@pytest.mark.parametrize('dq_name', ['fp32', 'bf16', 'none'])
@pytest.mark.parametrize('case', G.cases(), ids=IDS)
def test_loss_and_gradients_against_float64(case, dq_name):
    kind = case[4]
    z, e = G.make_case(*case)
    ref = None
    for deterministic in (False, True):
        for arena in (False, True):
            g = _grads(case, dq_name, deterministic, arena)
            assert torch.equal(g['idx'], fused(case)['idx'])
            if ref is None:
                ref = G.gradients(z, e, g['idx'].cpu(), g['dq'], BETA)
            loss, _, dz, de = ref
            tag = f'{IDS(case)} dq {dq_name} det {int(deterministic)} arena {int(arena)}'
            got_dz, got_de = g['dz'].cpu(), g['de'].cpu()
            assert bool(torch.isfinite(got_dz).all()) and bool(torch.isfinite(got_de).all()) and bool(torch.isfinite(g['loss']))
            close(f'{tag} loss', g['loss'].item(), loss.item(), *TOL['loss'], scale=bound_scale(kind, 'loss'))
            close(f'{tag} dz', got_dz, dz, *TOL['dz'], scale=bound_scale(kind, 'dz'))
            close(f'{tag} de', got_de, de, *TOL['de'], scale=bound_scale(kind, 'de'))


def test_backward_takes_an_out_of_range_token_as_a_zero_code():
    """vqk_gvq_backward_f32 on tokens the forward never writes (outside [0, K)): q = 0 for that slice and no code row -- of this group
    or of a neighbouring one -- receives its term: the float64 closed forms on slabs extended by a zero row that stands in for such a
    token.  Default (LDS chains + atomics) and deterministic mode (per-row terms + ordered sums); a ragged last block."""
    case = (77, 32, 8, 2, 'scale1')
    n, k, d, groups, kind = case
    z, e = G.make_case(*case)
    zd, ed = dev_case(case)
    idx = fused(case)['idx'].clone()
    for (row, g), bad in zip(((0, 0), (33, 1), (40, 0), (n - 1, 1)), (-1, k, 2 ** 40 + 3, -2 ** 62)):
        idx[row, g] = bad
    ok = (idx >= 0) & (idx < k)
    assert int((~ok).sum()) == 4
    dq = torch.randn(n, groups * d, generator=torch.Generator().manual_seed(11))
    e_ext = torch.cat([e.view(groups, k, d), torch.zeros(groups, 1, d)], 1).reshape(groups * (k + 1), d)
    _, _, dz_ref, de_ref = G.gradients(z, e_ext, torch.where(ok, idx, k).cpu(), dq, BETA)
    de_ref = de_ref.view(groups, k + 1, d)[:, :k].reshape(groups * k, d)
    lib, s = native.lib(), torch.cuda.current_stream().cuda_stream
    dqd, gs = dq.to(DEV), torch.ones((), device=DEV)
    cz, ce = 2.0 * BETA / (n * groups * d), 2.0 / (n * groups * d)
    ws = torch.empty(lib.vqk_gvq_backward_ws_bytes(n, d, groups), dtype=torch.uint8, device=DEV)
    for deterministic in (False, True):
        dz, de = torch.empty(n, groups * d, device=DEV), torch.zeros(groups * k, d, device=DEV)
        ops.set_deterministic(deterministic)
        try:
            ops._stream()                                         # arms / disarms the context's deterministic state
            native.check(lib.vqk_gvq_backward_f32(zd.data_ptr(), ed.data_ptr(), idx.data_ptr(), dqd.data_ptr(), ops.F32, n, k, d, groups,
                                                  cz, ce, gs.data_ptr(), dz.data_ptr(), de.data_ptr(), ws.data_ptr(), ws.numel(), s),
                         'gvq_backward')
            torch.cuda.synchronize()
        finally:
            ops.set_deterministic(False)
        close(f'bad token det {int(deterministic)} dz', dz.cpu(), dz_ref, *TOL['dz'], scale=bound_scale(kind, 'dz'))
        close(f'bad token det {int(deterministic)} de', de.cpu(), de_ref, *TOL['de'], scale=bound_scale(kind, 'de'))


@pytest.mark.parametrize('kind', ['scale1', 'collapsed'])
def test_deterministic_backward_is_reproducible(kind):
    case = (2051, 1024, 32, 2, kind)
    a, b = _grads(case, 'fp32', deterministic=True), _grads(case, 'fp32', deterministic=True)
    assert torch.equal(a['dz'], b['dz']) and torch.equal(a['de'], b['de']) and torch.equal(a['idx'], b['idx'])
    assert torch.equal(a['loss'], b['loss'])
    d = _grads(case, 'fp32')
    assert torch.equal(a['idx'], d['idx']) and torch.equal(a['dz'], d['dz'])          # dz holds no sum over rows


# ---------------------------------------------------------------------------------------------- 4. groups = 1 is the standard quantizer
@pytest.mark.parametrize('d', [32, 64])
@pytest.mark.parametrize('kind', ['scale1', 'collapsed'])
def test_one_group_reproduces_the_standard_quantizer(d, kind):
    n, k = 77, 64
    z, e = dev_case((n, k, d, 1, kind))
    dq = torch.randn(n, d, generator=torch.Generator().manual_seed(11)).to(DEV)
    out = []
    for name in ('grouped', 'standard'):
        x = img(z).detach().requires_grad_(True)
        cb = e.detach().clone().requires_grad_(True)
        if name == 'grouped':
            q, idx, loss, hist = ops.GVQLookupFn.apply(x, cb, BETA, 1, torch.float32)
            idx = idx.view(1, n)
        else:
            q, idx, loss, hist = ops.VQLookupFn.apply(x, cb, BETA, True, 0, torch.float32)
        dz, de = torch.autograd.grad([loss, q], [x, cb], [torch.ones((), device=DEV), img(dq)])
        out.append((idx, rows(q), hist, rows(dz), loss, de))
    torch.cuda.synchronize()
    a, b = out
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])    # tokens and q: bit for bit
    assert torch.equal(a[2], b[2]) and tuple(a[2].shape) == (k,)
    assert torch.equal(a[3], b[3])                                # dz: the same fused multiply-add per element
    close(f'G1 d{d} {kind} loss', a[4].item(), b[4].item(), *TOL['loss'])
    close(f'G1 d{d} {kind} de', a[5].cpu(), b[5].cpu(), *TOL['de'])


# ---------------------------------------------------------------------------------------------- 5. decode
@pytest.mark.parametrize('case', [c for c in G.cases() if c[:4] in ((77, 32, 8, 2), (64, 96, 16, 3), (256, 4096, 8, 8))], ids=IDS)
def test_decode_has_the_forwards_bits(case):
    n, k, d, groups, _ = case
    z, e = dev_case(case)
    f = fused(case)
    for dtype, key in ((torch.float32, 'q32'), (torch.bfloat16, 'qlo')):
        dec = ops.gvq_decode(f['idx'].view(1, n, groups), e, dtype)
        assert dec.dtype == dtype and tuple(dec.shape) == (1, n, groups * d) and torch.equal(dec[0], f[key])
    # a token outside [0, K) gives a zero slice; the row's other groups and the other rows are untouched -- K itself would be row 0 of
    # the NEXT group's slab, -1 the last row of the previous one
    row, grp = n // 2, groups - 2 if groups > 2 else 0
    for bad in (-1, k, 2 ** 40 + 3, -2 ** 62):
        wild = f['idx'].clone()
        wild[row, grp] = bad
        out = ops.gvq_decode(wild, e)
        keep = torch.ones(n, groups * d, dtype=torch.bool, device=DEV)
        keep[row, grp * d:(grp + 1) * d] = False
        assert float(out[~keep].abs().max()) == 0.0
        assert torch.equal(out[keep], f['q32'][keep])
    # the module over the same codebook
    quant = vqm.GroupedVectorQuantizer(k, groups * d, BETA, groups).to(DEV)
    with torch.no_grad():
        quant.codebook.weight.copy_(e)
        codes = quant.vec_to_codes(img(z))
        assert tuple(codes.shape) == (1, n, groups) and torch.equal(codes[0], f['idx'])
        assert torch.equal(quant.codes_to_vec(codes)[0], f['q32'])
        q, idx, _ = quant(img(z))
        assert torch.equal(rows(q), f['q32']) and torch.equal(idx[0], f['idx']) and torch.equal(quant.last_hist, f['hist'])
        assert torch.equal(quant.tokens_to_hist(idx), f['hist'].to(torch.int64))


# ---------------------------------------------------------------------------------------------- 6. the staged product path
def test_staged_serves_the_other_shapes():
    """d = 24 (no fused instantiation) and K = 40 (not a multiple of 32) go through gvq_staged and the torch backward; checked
    against float64 like the fused path"""
    for n, k, d, groups in ((67, 40, 16, 2), (67, 64, 24, 3)):
        g = torch.Generator().manual_seed(5 + d)
        z, e = torch.randn(n, groups * d, generator=g), torch.randn(groups * k, d, generator=g)
        dq = torch.randn(n, groups * d, generator=g)
        cb = e.to(DEV).requires_grad_(True)
        assert not ops.gvq_fused_serves(cb, groups)
        x = img(z.to(DEV)).detach().requires_grad_(True)
        q, idx, loss, hist = ops.GVQLookupFn.apply(x, cb, BETA, groups, torch.float32)
        dz, de = torch.autograd.grad([loss, q], [x, cb], [torch.ones((), device=DEV), img(dq.to(DEV))])
        idx = idx.view(n, groups).cpu()
        G.check_acceptance(z, e, idx, groups)
        assert torch.equal(ops.gvq_decode(idx.to(DEV), cb), rows(q)) and int(hist.sum()) == n * groups
        assert torch.equal(hist.cpu(), G.hist(idx, k).to(torch.int32))
        rl, _, rdz, rde = G.gradients(z, e, idx, dq, BETA)
        close(f'staged d{d} K{k} loss', loss.item(), rl.item(), *TOL['loss'])
        close(f'staged d{d} K{k} dz', rows(dz).cpu(), rdz, *TOL['dz'])
        close(f'staged d{d} K{k} de', de.cpu(), rde, *TOL['de'])
        assert max(RESTATEMENT.values()) < 1.0                   # this backward IS the restatement's arithmetic: the stated tolerances


# ---------------------------------------------------------------------------------------------- 7. model level
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)


def _qc(dim, groups, init=None, reinit=None):
    conf = dict(num_embeddings=64, embedding_dim=dim, reinit_every_n_epochs=reinit, type='grouped',
                params=dict(commitment_cost=0.25, groups=groups))
    if init:
        conf['codebook_init'] = init
    return conf


def _images(seed=3, b=4):
    return torch.rand(b, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize('dtype,dim,groups', [(torch.float32, 32, 4), (torch.bfloat16, 32, 4), (torch.float32, 64, 2), (torch.bfloat16, 64, 8)],
                         ids=['fp32-D32-G4', 'bf16-D32-G4', 'fp32-D64-G2', 'bf16-D64-G8'])
def test_model_step_tokens_roundtrip_and_checkpoint(dtype, dim, groups, tmp_path):
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, AE, _qc(dim, groups), None, TC, compute_dtype=dtype).to(DEV).train()
    assert ops.gvq_fused_serves(m.quantizer.codebook.weight, groups)
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    m.on_train_start()
    images = _images()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss = tr.train_batch(m, images, 0)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and float(m.logged['train/quant_loss']) > 0.0
    qz = m.quantizer
    assert qz.last_hist.numel() == groups * 64 and int(qz.last_hist.sum()) == 4 * 64 * groups
    assert int(m.train_epoch_usage_count.sum()) == 4 * 64 * groups
    after = m.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert {'quantizer.codebook.weight', 'encoder.conv_in.weight', 'decoder.conv_out.weight'} <= changed

    m.eval()
    with torch.no_grad():
        tokens = m.get_tokens(images)
        assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (4, 64, groups)
        vec = m.quantize(images)
        assert tuple(vec.shape) == (4, 64, dim)
        assert torch.equal(vec.cpu(), G.decode(tokens.view(-1, groups).cpu(), qz.codebook.weight.detach().cpu()).view(4, 64, dim))
        # (the autoencoder's GroupNorm sums are combined in arrival order by default: bits are compared in deterministic mode)
        ops.set_deterministic(True)
        try:
            tokens_det = m.get_tokens(images)
            assert torch.equal(m.reconstruct_from_tokens(tokens_det), m.reconstruct(images))
        finally:
            ops.set_deterministic(False)
        # the test loop's histogram goes through tokens_to_hist: one range per group
        m.on_test_epoch_start()
        m.test_step(images, 0)
        assert tuple(m.test_usage_count.shape) == (groups * 64,) and int(m.test_usage_count.sum()) == 4 * 64 * groups
        res = m.on_test_epoch_end()
        assert 0.0 < res['used_codebook'] <= 100.0 and 1.0 <= res['perplexity'] <= 64.0
    path = str(tmp_path / 'gvq.ckpt')
    tr.save_checkpoint(m, path)
    torch.manual_seed(1)
    m2 = model_mod.VQVAE(32, AE, _qc(dim, groups), None, TC, compute_dtype=dtype).to(DEV)
    t2 = trainer_mod.MiniTrainer(num_training_batches=10)
    t2.attach(m2)
    t2.load_checkpoint(m2, path)
    m2.eval()
    assert torch.equal(m2.quantizer.codebook.weight, m.quantizer.codebook.weight)
    assert torch.equal(m2.get_tokens(images), tokens)


def test_reinit_every_n_epochs_redraws_within_groups():
    torch.manual_seed(0)
    groups, k = 4, 64
    m = model_mod.VQVAE(32, AE, _qc(32, groups, reinit=1), None, TC).to(DEV).train()
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    m.on_train_start()
    tr.train_batch(m, _images(), 0)
    torch.cuda.synchronize()
    qz = m.quantizer
    count = m.train_epoch_usage_count.float()
    dead = (count == 0).view(groups, k)
    assert bool(dead.any()) and not bool(dead.all(1).any())       # 256 positions on 64 codes per group: some dead, none empty
    book = qz.codebook.weight.detach().clone().view(groups, k, -1)
    m.current_epoch = 1
    m.on_train_epoch_end()
    new = qz.codebook.weight.detach().view(groups, k, -1)
    assert m.train_epoch_usage_count is None
    for g in range(groups):
        assert torch.equal(new[g][~dead[g]], book[g][~dead[g]])   # live codes stay
        live = book[g][~dead[g]]
        assert all(bool((live == row).all(1).any()) for row in new[g][dead[g]])        # a dead code takes a live row of ITS group
    with torch.no_grad():                                         # nothing is cached: the next lookup ranks against the new rows
        tokens = m.eval().get_tokens(_images())
        assert torch.equal(qz.codes_to_vec(tokens).cpu(), G.decode(tokens.view(-1, groups).cpu(), qz.codebook.weight.detach().cpu()).view(4, 64, 32))


def test_codebook_init_runs():
    torch.manual_seed(0)
    groups, k = 4, 64
    m = model_mod.VQVAE(32, AE, _qc(32, groups, init=dict(method='kmeans', samples=256, iters=2)), None, TC).to(DEV).train()
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    before = m.quantizer.codebook.weight.detach().clone()
    batches = [_images(seed=s) for s in range(2)]
    ops.set_deterministic(True)                                   # (the encoder's GroupNorm sums and the Lloyd sums in a fixed order: bits are compared)
    try:
        info = m.init_codebook_from_batches(batches, seed=0)
        w = m.quantizer.codebook.weight.detach()
        assert info['samples'] == 256 and bool(torch.isfinite(w).all()) and not torch.equal(w, before)
        assert 0.0 < info['used'] <= 1.0 and np.isfinite(info['inertia'])
        # slab g is the k-means fit of the contiguous slice g with the draws u[g K:(g + 1) K]
        with torch.no_grad():
            flat = vqm._flat_view(ops.nhwc(m.encoder(m._preprocess_train(batches[0], False)[0]).to(torch.float32))).clone()
            assert tuple(flat.shape) == (256, 32)
            u = torch.rand(groups * k, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
            for g in (0, groups - 1):
                fit = ops.kmeans_fit(flat[:, g * 8:(g + 1) * 8].contiguous(), k, 2, u[g * k:(g + 1) * k])
                assert torch.equal(fit['centres'], w[g * k:(g + 1) * k])
    finally:
        ops.set_deterministic(False)
    with torch.no_grad():
        tokens = m.eval().get_tokens(_images())
        assert tuple(tokens.shape) == (4, 64, groups)


# ---------------------------------------------------------------------------------------------- graph replay
@pytest.mark.parametrize('deterministic', [True, False], ids=['deterministic', 'default'])
def test_captured_forward_backward_replays(deterministic):
    n, k, d, groups = 2051, 1024, 32, 2
    z0, e0 = dev_case((n, k, d, groups, 'scale1'))
    gen = torch.Generator().manual_seed(23)
    dq0 = torch.randn(n, groups * d, generator=gen).to(DEV)
    step = (torch.randn(groups * k, d, generator=gen) * 0.5).to(DEV)      # what optimizer steps do to the codebook

    def run(z, cb, dq):
        q, idx, loss, hist = ops.GVQLookupFn.apply(img(z), cb, BETA, groups, torch.float32)
        dz, de = torch.autograd.grad([q, loss], [z, cb], [img(dq), torch.ones((), device=DEV)])
        return q, idx, loss, hist, dz, de

    ops.set_deterministic(deterministic)
    try:
        cb = torch.nn.Parameter(e0.clone())
        z = z0.clone().requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(z, cb, dq0)                                               # first launches and workspaces: outside the capture
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
                update.replay()                                           # the codebook changes under the captured step: |e|^2 is taken
                #                                                           inside the capture, there is no workspace to refresh
        assert not torch.equal(first_idx, replayed[1])                    # the second replay ranked against the NEW codebook
    finally:
        ops.set_deterministic(False)


# ---------------------------------------------------------------------------------------------- entry points
SMALL = ['--set', 'image_size=32', '--set', 'autoencoder.channels=32', '--set', 'autoencoder.num_res_blocks=1',
         '--set', 'autoencoder.channel_multipliers=[1, 2]', '--set', 'quantizer.num_embeddings=64', '--set', 'training.cumulative_bs=4']


def test_entry_points(tmp_path, capsys):
    train = importlib.import_module(PKG + '.train')
    ev = importlib.import_module(PKG + '.evaluate')
    conf = os.path.join(ROOT, 'example_confs', 'grouped_vqvae.yaml')
    common = ['--params_file', conf] + SMALL + ['--max_epochs', '1', '--batches_per_epoch', '2', '--seed', '0', '--dtype', 'f32']
    capsys.readouterr()
    loss = train.main(common + ['--save_path', str(tmp_path), '--run_name', 'gvq'])
    out = capsys.readouterr().out
    assert loss is not None and np.isfinite(loss)
    assert 'eager launches' not in out                                                  # the graph was captured, not given up
    ckpt = str(tmp_path / 'gvq' / 'epoch=00.ckpt')
    assert os.path.exists(ckpt)
    small = tmp_path / 'conf.yaml'
    small.write_text('image_size: 32\nautoencoder:\n  channels: 32\n  num_res_blocks: 1\n  channel_multipliers: [1, 2]\n'
                     'quantizer:\n  num_embeddings: 64\n  embedding_dim: 64\n  type: grouped\n  params:\n'
                     '    commitment_cost: 0.25\n    groups: 8\n  reinit_every_n_epochs:\n')
    pt = str(tmp_path / 'test.pt')
    torch.save(torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(5)), pt)
    capsys.readouterr()
    res = ev.main(['--params_file', str(small), '--batch_size', '4', '--seed', '0', '--loading_path', ckpt, '--dtype', 'f32',
                   '--dataset_path', pt])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert json.loads(lines[-1]) == res
    assert {'mse', 'psnr', 'ssim', 'used_codebook', 'perplexity'} <= set(res)
    assert 0.0 < res['used_codebook'] <= 100.0 and 1.0 <= res['perplexity'] <= 64.0
