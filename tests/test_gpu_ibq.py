"""The index-backpropagation (IBQ) quantizer on the GPU (csrc/ibq.hip, _ops_ibq.py, IBQuantizer).

1. Tokens: every token is accepted by float64 (2 eta rule of tests/ibq_reference.py), on separated rows it IS the float64 argmax, on
   'collapsed' it is the smallest index of the winning group; hist.sum() == N, hist == bincount(idx); q == E[idx] bit for bit in fp32
   and bf16; the argmax-only call gives the training forward's tokens bit for bit.
2. lse, ebar, the loss against float64; dz and dE teacher-forced on the device's tokens: 4 x the TABLE entry of the restatement
   (max|got - want| / max|want|), the loss rtol 1e-5; dq fp32 / bf16 / absent, s present / absent; dE into a fresh buffer and into a
   pre-filled one (old + sum: one rounding of |old + sum| is added to the bound).
3. Two runs give bit-identical dz, dE, loss and ebar, with and without deterministic mode.  4. Fused vs staged, and the staged route
   at D = 48, and the routing of small shapes (N K <= IBQ_STAGED_BWD_MAX_NK) to the torch backward.  5. Out-of-range tokens.  6. Capture and replay around an in-place codebook step.  7. Model: train step, EVERY codebook
   row moves (with ``type: standard`` only the used rows do), token round trip, histogram, checkpoint, re-initialisation.
8. train.py / evaluate.py.
Cases: every kind at the five small shapes and both temperatures; 'normal' at (2051, 1024, 256) T = 1 and (4096, 4096, 256) T = 0.5
(float64 references are evaluated on the device).  Every figure that is asserted with a tolerance is printed first (``IBQMEASURE``).

Measured on an MI355X: the worst figure / bound of the file is 0.78 (ebar at (4096, 4096, 256), T = 0.5), the next 0.54 ('peaked' ebar
at (64, 64, 256)) and 0.52 ('peaked' dz at (1, 64, 64)); the loss is within 1.7e-7."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import ibq_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
ibq = importlib.import_module(PKG + '._ops_ibq')
native = importlib.import_module(PKG + '._native')
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
BETA, SCALE = R.BETA, R.SCALE

CASES = [(s, kind, t) for s in R.SMALL_SHAPES for kind in R.KINDS for t in R.TEMPS] + \
        [((2051, 1024, 256), 'normal', 1.0), ((4096, 4096, 256), 'normal', 0.5)]
CID = lambda c: f'{R.shape_id(c[0])}-{c[1]}-T{c[2]}'            # noqa: E731
VARIANT_CASES = [((65, 96, 64), 'normal', 1.0), ((130, 200, 256), 'peaked', 1.0), ((100, 40, 128), 'scaled', 0.5)]
_IN: dict = {}
_FWD: dict = {}
_REF: dict = {}


def inputs(shape, kind):
    """(z, e, g) of one case on the device in fp32, made once and shared read-only"""
    key = (shape, kind)
    if key not in _IN:
        _IN[key] = tuple(t.to(torch.float32).to(DEV) for t in R.make_case(*shape, kind))
    return _IN[key]


def forward(case):
    """the training forward of one case, run once and shared read-only"""
    if case not in _FWD:
        shape, kind, t = case
        z, e, _ = inputs(shape, kind)
        idx, q32, qlo, sse, hist, lse, ebar = ibq._ibq_forward(z, e, 1.0 / t, True, True, True, True)
        torch.cuda.synchronize()
        _FWD[case] = dict(idx=idx, q32=q32, qlo=qlo, sse=sse, hist=hist, lse=lse, ebar=ebar)
    return _FWD[case]


def reference(case, g, s, idx=None):
    """the float64 closed forms on the device, teacher-forced on the device's tokens"""
    shape, kind, t = case
    z, e, _ = inputs(shape, kind)
    idx = forward(case)['idx'] if idx is None else idx
    return R.closed_form(z, e, idx, g, s, BETA, t)


def backward(case, dq, s, de=None, idx=None, want_de=True):
    """vqk_ibq_backward_f32 on the shared forward of one case: (dz, de); de is accumulated into when given"""
    shape, kind, t = case
    z, e, _ = inputs(shape, kind)
    f = forward(case)
    n, d = z.shape
    gs = torch.tensor(s, dtype=torch.float32, device=DEV) if s is not None else None
    ce = 2.0 / (n * d) if s is not None else 0.0
    dz = torch.empty_like(z)
    if want_de and de is None:
        de = torch.zeros_like(e)
    ops.ibq_backward_rows(z, e, f['idx'] if idx is None else idx, f['lse'], f['ebar'], dq, 1.0 / t, BETA * ce, ce, gs, dz, de)
    torch.cuda.synchronize()
    return dz, de


def held(name, got, want, bound, norm=None, extra=None):
    """max|got - want| <= bound max|want| (+ extra, elementwise), printed first"""
    got, want = got.double(), want.double()
    norm = float(want.abs().max()) if norm is None else norm
    err = (got - want).abs()
    allow = bound * norm + (extra if extra is not None else 0.0)
    ratio = float((err / allow).max()) if norm > 0 else float(err.max())
    print(f'IBQMEASURE {name}: max abs err {float(err.max()):.3e}, bound {bound:.2g} x {norm:.3e}, worst err / bound {ratio:.3g}')
    assert bool((err <= allow).all()), name


def dq_of(case, mode):
    g = inputs(case[0], case[1])[2]
    return None if mode == 'none' else (g.to(torch.bfloat16) if mode == 'bf16' else g)


# ---------------------------------------------------------------------------------------------- 1. tokens
@pytest.mark.parametrize('case', CASES, ids=CID)
def test_tokens(case):
    shape, kind, t = case
    n, k, d = shape
    z, e, _ = inputs(shape, kind)
    f = forward(case)
    idx = f['idx']
    assert int(idx.min()) >= 0 and int(idx.max()) < k
    sep = R.check_acceptance(z, e, idx, t)
    print(f'IBQMEASURE {CID(case)}: separated rows {sep:.4f}')
    if kind == 'collapsed':
        assert int(idx.max()) < 4                                 # the smallest index of the winning group
        s64, best, first, _, _ = R.margins(z, e, t)
        exact = s64.gather(1, idx.view(-1, 1))[:, 0] == best      # where fp32 and float64 agree on the winning group: its first member
        assert torch.equal(idx[exact], first[exact])
    assert int(f['hist'].sum()) == n and torch.equal(f['hist'].cpu(), R.hist(idx, k).to(torch.int32))
    assert torch.equal(f['q32'], e[idx]) and torch.equal(f['qlo'], e[idx].to(torch.bfloat16))
    assert torch.equal(ops.ibq_assign(z, e, t), idx)              # the argmax-only mode: the same tokens, bit for bit
    only = ibq._ibq_forward(z, e, 1.0 / t, False, True, False, True)
    assert torch.equal(only[0], idx) and torch.equal(only[1], f['q32']) and torch.equal(only[4], f['hist'])
    assert torch.equal(only[3], f['sse']) and only[5] is None and only[6] is None


# ---------------------------------------------------------------------------------------------- 2. quantities against float64
@pytest.mark.parametrize('case', CASES, ids=CID)
def test_quantities_against_float64(case):
    shape, kind, t = case
    n, d = shape[0], shape[2]
    f = forward(case)
    g = dq_of(case, 'f32')
    ref = reference(case, g, SCALE)
    held(f'{CID(case)} lse', f['lse'], ref['lse'], 4 * R.bound(kind, 'lse'))
    held(f'{CID(case)} ebar', f['ebar'], ref['ebar'], 4 * R.bound(kind, 'ebar'))
    loss = float(f['sse']) * (2.0 + BETA) / (n * d)
    print(f'IBQMEASURE {CID(case)} loss: rel err {abs(loss - float(ref["loss"])) / float(ref["loss"]):.3e} (bound 1e-5)')
    assert abs(loss - float(ref['loss'])) <= 1e-5 * float(ref['loss'])
    dz, de = backward(case, g, SCALE)
    held(f'{CID(case)} dz', dz, ref['dz'], 4 * R.bound(kind, 'dz'))
    held(f'{CID(case)} de', de, ref['de'], 4 * R.bound(kind, 'de'))


@pytest.mark.parametrize('case', VARIANT_CASES, ids=CID)
@pytest.mark.parametrize('mode,s', [('bf16', SCALE), ('none', SCALE), ('f32', None), ('bf16', None)])
def test_gradient_variants_and_prefilled_target(case, mode, s):
    kind = case[1]
    dq = dq_of(case, mode)
    ref = reference(case, dq.float() if dq is not None else None, s)
    dz, de = backward(case, dq, s)
    held(f'{CID(case)} dq {mode} s {s} dz', dz, ref['dz'], 4 * R.bound(kind, 'dz'))
    held(f'{CID(case)} dq {mode} s {s} de', de, ref['de'], 4 * R.bound(kind, 'de'))
    old = torch.randn(de.shape, generator=torch.Generator().manual_seed(31)).to(DEV) * float(ref['de'].abs().max())
    _, into = backward(case, dq, s, de=old.clone())
    want = old.double() + ref['de']
    held(f'{CID(case)} dq {mode} s {s} de into a pre-filled target', into, want, 4 * R.bound(kind, 'de'), norm=float(ref['de'].abs().max()),
         extra=2.0 ** -24 * want.abs())
    assert torch.equal(into, old + de)                            # one read-modify-write of the ordered sum
    dz_only, none = backward(case, dq, s, want_de=False)          # de = NULL: the code-owning pass is skipped
    assert none is None and torch.equal(dz_only, dz)


def test_absent_cotangents_give_zero():
    z, e, _ = inputs((65, 96, 64), 'normal')
    x = z.view(1, 65, 1, 64).permute(0, 3, 1, 2).detach().requires_grad_(True)
    cb = e.clone().requires_grad_(True)
    q, idx, loss, hist = ops.IBQLookupFn.apply(x, cb, BETA, 1.0, torch.float32)
    dz, de = torch.autograd.grad([q.sum() * 0.0 + 0.0 * loss], [x, cb], allow_unused=True)
    assert float(dz.abs().max()) == 0.0 and (de is None or float(de.abs().max()) == 0.0)


# ---------------------------------------------------------------------------------------------- 3. reproducibility
@pytest.mark.parametrize('case', [((130, 200, 256), 'normal', 1.0), ((2051, 1024, 256), 'normal', 1.0)], ids=CID)
def test_runs_are_bit_identical_in_every_mode(case):
    shape, kind, t = case
    z, e, g = inputs(shape, kind)
    f = forward(case)
    dz0, de0 = backward(case, g, SCALE)
    try:
        for det in (False, True):
            ops.set_deterministic(det)
            again = ibq._ibq_forward(z, e, 1.0 / t, True, True, False, True)
            dz, de = backward(case, g, SCALE)
            for name, a, b in (('idx', again[0], f['idx']), ('sse', again[3], f['sse']), ('lse', again[5], f['lse']),
                               ('ebar', again[6], f['ebar']), ('dz', dz, dz0), ('de', de, de0)):
                assert torch.equal(a, b), (det, name)
    finally:
        ops.set_deterministic(False)


# ---------------------------------------------------------------------------------------------- 4. fused against staged
def _through_fn(shape, kind, t, fused, dtype=torch.float32, force_kernels=True):
    z, e, g = inputs(shape, kind)
    n, d = z.shape
    prev, prev_nk = ops.IBQ_FUSED, ibq.IBQ_STAGED_BWD_MAX_NK
    ops.IBQ_FUSED = fused
    ibq.IBQ_STAGED_BWD_MAX_NK = 0 if force_kernels else prev_nk   # (small shapes are routed to the torch backward: see the constant)
    try:
        x = z.view(1, n, 1, d).permute(0, 3, 1, 2).detach().requires_grad_(True)
        cb = e.clone().requires_grad_(True)
        assert ops.ibq_fused_serves(cb) == (fused and d in (64, 128, 256))
        q, idx, loss, hist = ops.IBQLookupFn.apply(x, cb, BETA, t, dtype)
        dz, de = torch.autograd.grad([q, loss], [x, cb], [g.view(1, n, 1, d).permute(0, 3, 1, 2).to(dtype), torch.tensor(SCALE, device=DEV)])
        torch.cuda.synchronize()
    finally:
        ops.IBQ_FUSED, ibq.IBQ_STAGED_BWD_MAX_NK = prev, prev_nk
    rows = lambda v: v.permute(0, 2, 3, 1).reshape(n, d)          # noqa: E731
    return dict(q=rows(q), idx=idx.view(-1), loss=loss, hist=hist, dz=rows(dz), de=de)


@pytest.mark.parametrize('case', [((130, 200, 256), 'normal', 1.0), ((65, 96, 64), 'scaled', 0.5), ((100, 40, 128), 'peaked', 1.0)], ids=CID)
def test_fused_against_staged(case):
    shape, kind, t = case
    z, e, g = inputs(shape, kind)
    f, s = _through_fn(shape, kind, t, True), _through_fn(shape, kind, t, False)
    _, _, first, gap, eta2 = R.margins(z, e, t)
    sep = gap > eta2
    assert torch.equal(f['idx'][sep], s['idx'][sep]) and torch.equal(f['idx'][sep], first[sep])
    assert torch.equal(f['idx'], forward(case)['idx'])            # the Function runs the kernels of the raw calls
    for name, got in (('fused', f), ('staged', s)):
        ref = R.closed_form(z, e, got['idx'], g, SCALE, BETA, t)
        assert abs(float(got['loss']) - float(ref['loss'])) <= 1e-5 * float(ref['loss'])
        assert torch.equal(got['q'], e[got['idx']])
        held(f'{CID(case)} {name} dz', got['dz'], ref['dz'], 4 * R.bound(kind, 'dz'))
        held(f'{CID(case)} {name} de', got['de'], ref['de'], 4 * R.bound(kind, 'de'))


def test_small_shapes_take_the_torch_backward_and_large_ones_the_kernels():
    """the routing constant: at N K <= IBQ_STAGED_BWD_MAX_NK the Function's backward is ops.ibq_backward_staged on the fused forward's
    lse / ebar, beyond it the three launches -- each compared bit for bit with the direct call"""
    assert ibq.IBQ_STAGED_BWD_MAX_NK == 1 << 23
    for case in (((2051, 1024, 256), 'normal', 1.0), ((4096, 4096, 256), 'normal', 0.5)):
        shape, kind, t = case
        n, k, d = shape
        z, e, g = inputs(shape, kind)
        f = forward(case)
        got = _through_fn(shape, kind, t, True, force_kernels=False)
        assert torch.equal(got['idx'], f['idx'])
        if n * k > ibq.IBQ_STAGED_BWD_MAX_NK:
            dz, de = backward(case, g, SCALE)
        else:
            ce = SCALE * 2.0 / (n * d)
            dz, de = ops.ibq_backward_staged(z, e, f['idx'], f['lse'], f['ebar'], g, 1.0 / t, torch.tensor(BETA * ce, device=DEV),
                                             torch.tensor(ce, device=DEV))
            ref = reference(case, g, SCALE)
            held(f'{CID(case)} routed staged dz', got['dz'], ref['dz'], 4 * R.bound(kind, 'dz'))
            held(f'{CID(case)} routed staged de', got['de'], ref['de'], 4 * R.bound(kind, 'de'))
        print(f'IBQMEASURE {CID(case)} routed backward vs the direct call: dz {R.distance(got["dz"], dz):.3e}, de {R.distance(got["de"], de):.3e}')
        if n * k > ibq.IBQ_STAGED_BWD_MAX_NK:
            assert torch.equal(got['dz'], dz) and torch.equal(got['de'], de)
        else:                                                     # (the Function scales by the cotangent tensor s * c: one rounding apart)
            assert R.distance(got['dz'], dz) <= 1e-6 and R.distance(got['de'], de) <= 1e-6


def test_staged_route_serves_other_shapes():
    shape = R.STAGED_SHAPE
    n, k, d = shape
    for t in R.TEMPS:
        z, e, g = inputs(shape, 'normal')
        assert not ops.ibq_fused_serves(e)
        got = _through_fn(shape, 'normal', t, True)               # the switch is on: the shape decides the route
        R.check_acceptance(z, e, got['idx'], t)
        assert torch.equal(got['q'], e[got['idx']]) and int(got['hist'].sum()) == n
        assert torch.equal(got['hist'].cpu(), R.hist(got['idx'], k).to(torch.int32))
        assert torch.equal(ops.ibq_assign(z, e, t), got['idx'])
        ref = R.closed_form(z, e, got['idx'], g, SCALE, BETA, t)
        assert abs(float(got['loss']) - float(ref['loss'])) <= 1e-5 * float(ref['loss'])
        held(f'staged {R.shape_id(shape)} T{t} dz', got['dz'], ref['dz'], 4 * R.bound('normal', 'dz'))
        held(f'staged {R.shape_id(shape)} T{t} de', got['de'], ref['de'], 4 * R.bound('normal', 'de'))


# ---------------------------------------------------------------------------------------------- 5. out-of-range tokens
@pytest.mark.parametrize('case', [((130, 200, 256), 'normal', 1.0), ((65, 96, 64), 'normal', 0.5)], ids=CID)
def test_out_of_range_tokens_skip_their_hard_terms(case):
    shape, kind, t = case
    n, k, d = shape
    g = dq_of(case, 'f32')
    idx = forward(case)['idx'].clone()
    rows = torch.tensor([0, 7, n // 2, n - 1], device=DEV)
    idx[rows] = torch.tensor([-1, k, k + 20, 1 << 40], device=DEV)            # k, k + 20: codes of the tail tile
    ref = reference(case, g, SCALE, idx)
    dz, de = backward(case, g, SCALE, idx=idx)
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(de).all())
    held(f'{CID(case)} out-of-range dz', dz, ref['dz'], 4 * R.bound(kind, 'dz'))
    held(f'{CID(case)} out-of-range de', de, ref['de'], 4 * R.bound(kind, 'de'))
    dz0, _ = backward(case, g, SCALE)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[rows] = False
    assert torch.equal(dz[keep], dz0[keep])                                   # every other row: the same bits


# ---------------------------------------------------------------------------------------------- 6. graph replay
@pytest.mark.parametrize('shape', [(2051, 1024, 256), (130, 200, 64), (8200, 1030, 64)], ids=R.shape_id)      # (the last: N K above the routing constant)
def test_captured_forward_backward_replays(shape):
    n, k, d = shape
    z0, e0, g0 = (t.to(torch.float32).to(DEV) for t in R.make_case(n, k, d, 'normal'))
    step = (torch.randn(k, d, generator=torch.Generator().manual_seed(23)) * 0.5 * d ** -0.5).to(DEV)     # what optimizer steps do to E
    img = lambda v: v.view(1, n, 1, d).permute(0, 3, 1, 2)        # noqa: E731

    def run(z, cb):
        q, idx, loss, hist = ops.IBQLookupFn.apply(img(z), cb, BETA, 1.0, torch.float32)
        dz, de = torch.autograd.grad([q, loss], [z, cb], [img(g0), torch.ones((), device=DEV)])
        return q, idx, loss, hist, dz, de

    cb = torch.nn.Parameter(e0.clone())
    z = z0.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(z, cb)                                                # first launches and workspaces: outside the capture
        torch.cuda.synchronize()
        graph, update = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = run(z, cb)
        with torch.cuda.graph(update, stream=side):
            with torch.no_grad():
                cb.add_(step)
    torch.cuda.current_stream().wait_stream(side)
    for round_ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.detach().clone() for t in got]
        want = run(z, cb)
        torch.cuda.synchronize()
        for name, a, b in zip(('q', 'idx', 'loss', 'hist', 'dz', 'de'), replayed, want):
            assert torch.equal(a, b), (round_, name)              # every sum is ordered: the loss too
        if round_ == 0:
            first_idx = replayed[1]
            update.replay()                                       # the codebook changes under the captured step
    assert not torch.equal(first_idx, replayed[1])                # the second replay ranked against the NEW codebook


# ---------------------------------------------------------------------------------------------- 7. model level
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)


def _qc(dim, qtype='ibq', k=64, reinit=None):
    params = dict(commitment_cost=0.25, temperature=1.0) if qtype == 'ibq' else dict(commitment_cost=0.25)
    return dict(num_embeddings=k, embedding_dim=dim, reinit_every_n_epochs=reinit, type=qtype, params=params)


def _images(seed=3, b=4):
    return torch.rand(b, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _one_step(qtype, dim=64, dtype=torch.float32):
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, AE, _qc(dim, qtype), None, TC, compute_dtype=dtype).to(DEV).train()
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    m.on_train_start()
    before = m.quantizer.codebook.weight.detach().clone()
    loss = tr.train_batch(m, _images(), 0)
    torch.cuda.synchronize()
    moved = (m.quantizer.codebook.weight.detach() != before).any(dim=1)
    return m, tr, loss, moved


def test_one_step_moves_every_code_where_standard_moves_only_the_used_ones():
    m, _, loss, moved = _one_step('ibq')
    used = m.quantizer.last_hist > 0
    assert np.isfinite(loss.item()) and int(used.sum()) < 64      # some codes were not selected ...
    assert bool(moved.all())                                      # ... and every row has moved all the same
    m, _, loss, moved = _one_step('standard')
    used = m.quantizer.last_hist > 0
    assert np.isfinite(loss.item()) and torch.equal(moved, used)  # the standard quantizer: exactly the used rows


@pytest.mark.parametrize('dtype,dim', [(torch.float32, 64), (torch.bfloat16, 64), (torch.bfloat16, 256)], ids=['fp32-D64', 'bf16-D64', 'bf16-D256'])
def test_model_step_tokens_roundtrip_and_checkpoint(dtype, dim, tmp_path):
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, AE, _qc(dim, reinit=1), None, TC, compute_dtype=dtype).to(DEV).train()
    qz = m.quantizer
    assert ops.ibq_fused_serves(qz.codebook.weight)
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    m.on_train_start()
    images = _images()
    for step in range(3):
        loss = tr.train_batch(m, images, step)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and float(m.logged['train/quant_loss']) > 0.0
    assert qz.last_hist.numel() == 64 and int(qz.last_hist.sum()) == 4 * 64

    m.eval()
    with torch.no_grad():
        tokens = m.get_tokens(images)
        assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (4, 64)
        e = qz.get_codebook()
        assert torch.equal(m.quantize(images), e[tokens]) and torch.equal(qz.codes_to_vec(tokens), e[tokens])
        z = m.encoder(m.preprocess_batch(images))
        q, idx, _ = qz(z)                                         # no_grad: the argmax-only mode
        assert torch.equal(qz.vec_to_codes(z), idx)
    zg = z.detach().float().requires_grad_(True)                  # the training forward on the same latents: the same tokens, bit for bit
    assert torch.equal(qz(zg)[1], idx)
    with torch.no_grad():
        ops.set_deterministic(True)     # (the autoencoder's GroupNorm sums are combined in arrival order by default: bits are compared)
        try:
            tokens_det = m.get_tokens(images)
            assert torch.equal(m.reconstruct_from_tokens(tokens_det), m.reconstruct(images))
        finally:
            ops.set_deterministic(False)
        m.on_test_epoch_start()
        m.test_step(images, 0)
        assert tuple(m.test_usage_count.shape) == (64,) and int(m.test_usage_count.sum()) == 4 * 64
        res = m.on_test_epoch_end()
        assert 0.0 < res['used_codebook'] <= 100.0 and 1.0 <= res['perplexity'] <= 64.0
        usage = qz.get_codebook_usage(m.train_epoch_usage_count.float())[0]       # reinit_every_n_epochs is allowed: the base class's
        dead = usage == 0
        book = qz.codebook.weight.detach().clone()
        qz.reinit_unused_codes(usage)
        assert torch.equal(qz.codebook.weight[~dead], book[~dead])
        if bool(dead.any()):
            live = book[~dead]
            assert all(bool((live == row).all(1).any()) for row in qz.codebook.weight[dead])
        tokens = m.get_tokens(images)
    path = str(tmp_path / 'ibq.ckpt')
    tr.save_checkpoint(m, path)
    torch.manual_seed(1)
    m2 = model_mod.VQVAE(32, AE, _qc(dim, reinit=1), None, TC, compute_dtype=dtype).to(DEV)
    t2 = trainer_mod.MiniTrainer(num_training_batches=10)
    t2.attach(m2)
    t2.load_checkpoint(m2, path)
    m2.eval()
    assert torch.equal(m2.quantizer.codebook.weight, qz.codebook.weight)
    assert torch.equal(m2.get_tokens(images), tokens)


# ---------------------------------------------------------------------------------------------- 8. entry points
SMALL = ['--set', 'image_size=32', '--set', 'autoencoder.channels=32', '--set', 'autoencoder.num_res_blocks=1',
         '--set', 'autoencoder.channel_multipliers=[1, 2]', '--set', 'quantizer.num_embeddings=64', '--set', 'training.cumulative_bs=4']


def test_entry_points(tmp_path, capsys):
    train = importlib.import_module(PKG + '.train')
    ev = importlib.import_module(PKG + '.evaluate')
    conf = os.path.join(ROOT, 'example_confs', 'ibq_vqvae.yaml')
    common = ['--params_file', conf] + SMALL + ['--max_epochs', '1', '--batches_per_epoch', '2', '--seed', '0', '--dtype', 'f32']
    capsys.readouterr()
    loss = train.main(common + ['--save_path', str(tmp_path), '--run_name', 'ibq'])
    out = capsys.readouterr().out
    assert loss is not None and np.isfinite(loss)
    assert 'eager launches' not in out                                                  # the graph was captured, not given up
    ckpt = str(tmp_path / 'ibq' / 'epoch=00.ckpt')
    assert os.path.exists(ckpt)
    small = tmp_path / 'conf.yaml'
    small.write_text('image_size: 32\nautoencoder:\n  channels: 32\n  num_res_blocks: 1\n  channel_multipliers: [1, 2]\n'
                     'quantizer:\n  num_embeddings: 64\n  embedding_dim: 256\n  type: ibq\n  params:\n'
                     '    commitment_cost: 0.25\n    temperature: 1.0\n  reinit_every_n_epochs:\n')
    pt = str(tmp_path / 'test.pt')
    torch.save(torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(5)), pt)
    capsys.readouterr()
    res = ev.main(['--params_file', str(small), '--batch_size', '4', '--seed', '0', '--loading_path', ckpt, '--dtype', 'f32',
                   '--dataset_path', pt])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert json.loads(lines[-1]) == res
    assert {'mse', 'psnr', 'ssim', 'used_codebook', 'perplexity'} <= set(res)
    assert 0.0 < res['used_codebook'] <= 100.0 and 1.0 <= res['perplexity'] <= 64.0
