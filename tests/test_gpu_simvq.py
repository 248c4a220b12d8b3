"""The SimVQ quantizer on the GPU (csrc/simvq.hip, _ops_simvq.py, SimVectorQuantizer).

1. Projection, identity: E == C as numbers.  2. Projection, other kinds: |E - E64| within the derived fp32 summation bound
   (tests/simvq_reference.py::projection_bound: any order of D products and the bias).
3. Lookup on the device's E read back: idx, q fp32 / bf16 and hist equal ops.vq_assign + vqk_vq_gather_f32 on that E BIT FOR BIT;
   float64 acceptance on every row (2 eta rule of tests/gvq_reference.py at one group); hist.sum() == N; loss rtol 1e-5.
4. Backward dz == vqk_vq_backward_f32(z, E, idx, dq, de = NULL) bit for bit, dq fp32 / bf16 / absent.
5. Backward dW / db against the float64 terms teacher-forced on the device's E and idx: (N + 8) 2^-24 term_sum per element
   (tests/simvq_reference.py::gradient_bounds), into a fresh buffer and into a pre-filled one (old + sum: one more rounding of the
   result, 2^-24 |old + sum|, is added to the bound).
6. Two runs give bit-identical dW / db, with and without deterministic mode.  7. Out-of-range tokens.  8. Fused vs staged.
9. The staged product path at (40, 40, 48).  10. Capture and replay around an in-place step of W.  11. Model step, tokens,
   histogram, checkpoint.  12. train.py / evaluate.py.
The inputs (tests/simvq_reference.py) are shared with the CPU tests; every figure that is asserted with a tolerance is printed first
(``SIMVQMEASURE``)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import simvq_reference as S

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
BETA = 0.25
SCALE = 0.7                          # the loss cotangent s of the raw backward calls
IDS = lambda c: f'N{c[0]}-K{c[1]}-D{c[2]}' + (f'-{c[3]}' if len(c) > 3 else '')
_E: dict = {}


def on_dev(case):
    return tuple(t.to(DEV) if t is not None else None for t in S.make_case(*case))


def device_e(case):
    """the device's E of one case, projected once and shared read-only"""
    if case not in _E:
        z, c, w, b = on_dev(case)
        _E[case] = ops.simvq_project(c, w, b)
        torch.cuda.synchronize()
    return _E[case]


def img(t):
    n, d = t.shape
    return t.view(1, n, 1, d).permute(0, 3, 1, 2)


def rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def within(name, got, want, bound):
    got, want, bound = (np.asarray(t, dtype=np.float64) for t in (got, want, bound))
    err = np.abs(got - want)
    frac = err / np.maximum(bound, 1e-300)
    print(f'SIMVQMEASURE {name}: max abs err {err.max():.3e}, worst err / bound {np.where(err > 0, frac, 0.0).max():.3g}')
    assert bool((err <= bound).all()), name


def standard_lookup(z, e):
    """ops.vq_assign + vqk_vq_gather_f32 on (z, E): (idx, q fp32, q bf16, sse, hist)"""
    n, d = z.shape
    k = e.shape[0]
    idx = ops.vq_assign(z, e, 0)
    q32 = torch.empty((n, d), dtype=torch.float32, device=DEV)
    qlo = torch.empty((n, d), dtype=torch.bfloat16, device=DEV)
    hist, sse = ops.hist_sse(k, z.device)
    native.check(native.lib().vqk_vq_gather_f32(z.data_ptr(), e.data_ptr(), idx.data_ptr(), n, k, d, q32.data_ptr(), qlo.data_ptr(),
                                                sse.data_ptr(), hist.data_ptr(), ops._stream()), 'vq_gather')
    return idx, q32, qlo, sse, hist


def raw_backward(z, e, c, idx, dq, dw=None, db=None, want_db=True):
    """vqk_simvq_backward_f32 with s = SCALE on the device: (dz, dw, db); dw / db are accumulated into when given"""
    n, d = z.shape
    k = e.shape[0]
    lib = native.lib()
    ws = torch.empty(lib.vqk_simvq_backward_ws_bytes(n, d), dtype=torch.uint8, device=DEV)
    gs = torch.tensor(SCALE, dtype=torch.float32, device=DEV)
    dz = torch.empty_like(z)
    dw = torch.zeros((d, d), dtype=torch.float32, device=DEV) if dw is None else dw
    db = (torch.zeros(d, dtype=torch.float32, device=DEV) if db is None else db) if want_db else None
    native.check(lib.vqk_simvq_backward_f32(z.data_ptr(), e.data_ptr(), c.data_ptr(), idx.data_ptr(), ops._p(dq),
                                            ops.dcode(dq.dtype) if dq is not None else ops.F32, n, k, d, 2.0 * BETA / (n * d), 2.0 / (n * d),
                                            gs.data_ptr(), dz.data_ptr(), dw.data_ptr(), ops._p(db), ws.data_ptr(), ws.numel(), ops._stream()),
                 'simvq_backward')
    torch.cuda.synchronize()
    return dz, dw, db


def make_dq(n, d, mode, seed=11):
    if mode == 'none':
        return None
    dq = torch.randn(n, d, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return dq.to(torch.bfloat16) if mode == 'bf16' else dq


# ---------------------------------------------------------------------------------------------- 1. / 2. projection
@pytest.mark.parametrize('shape', S.SHAPES, ids=IDS)
def test_projection_identity_returns_the_table(shape):
    case = shape + ('identity',)
    z, c, w, b = on_dev(case)
    e = device_e(case)
    assert e.dtype == torch.float32 and tuple(e.shape) == tuple(c.shape)
    assert bool((e == c).all())
    assert bool((ops.simvq_project(c, w, None) == c).all())        # and without the bias addition


@pytest.mark.parametrize('case', S.cases(['random', 'collapsed', 'nobias']), ids=IDS)
def test_projection_within_the_summation_bound(case):
    z, c, w, b = S.make_case(*case)
    e = device_e(case).cpu()
    within(f'{IDS(case)} E', e, S.effective(c, w, b), S.projection_bound(c, w, b))
    assert torch.equal(ops.simvq_project(*on_dev(case)[1:]).cpu(), e)      # the order of the sum is fixed: the same bits again
    if case[3] == 'collapsed':
        assert torch.equal(e, e[:4][torch.arange(case[1]) % 4])            # equal rows of C give bitwise-equal rows of E
    if case[3] == 'random':                                                # a transposed W cannot pass
        wrong = (S.effective(c, w.T.contiguous(), b) - e.double()).abs()
        assert bool((wrong > S.projection_bound(c, w, b)).any())


# ---------------------------------------------------------------------------------------------- 3. lookup on the device's E
@pytest.mark.parametrize('project', [False, True], ids=['addmm', 'hip-projection'])
@pytest.mark.parametrize('case', S.cases(), ids=IDS)
def test_lookup_equals_the_standard_operators_on_the_device_e(case, project):
    """both routes of the projection (ops.SIMVQ_PROJECT off, the default, and on): E is read back through ops.simvq_effective, the call
    the forward makes"""
    n, k, d, kind = case
    z, c, w, b = on_dev(case)
    saved = ops.SIMVQ_PROJECT
    ops.SIMVQ_PROJECT = project
    try:
        assert ops.simvq_project_serves(c) == project
        e = ops.simvq_effective(c, w, b)
        with torch.no_grad():
            q32, idx, loss, hist = ops.SimVQLookupFn.apply(img(z), c, w, b, BETA, torch.float32)
            qlo, idx2, loss2, hist2 = ops.SimVQLookupFn.apply(img(z), c, w, b, BETA, torch.bfloat16)
            assert torch.equal(ops.simvq_assign(z, c, w, b), idx.view(-1))
            assert torch.equal(ops.simvq_effective(c, w, b), e)
        torch.cuda.synchronize()
    finally:
        ops.SIMVQ_PROJECT = saved
    if project:
        assert torch.equal(e, device_e(case))                     # the kernel's bits, again
    within(f'{IDS(case)} E through simvq_effective', e.cpu(), S.effective(*S.make_case(*case)[1:]), S.projection_bound(*S.make_case(*case)[1:]))
    assert ops.simvq_fused_serves(c)
    assert tuple(idx.shape) == (1, n) and idx.dtype == torch.int64 and torch.equal(idx, idx2) and torch.equal(hist, hist2)
    idx_s, q_s, qlo_s, sse_s, hist_s = standard_lookup(z, e)
    idx = idx.view(-1)
    assert torch.equal(idx, idx_s)
    assert torch.equal(rows(q32), q_s) and q32.dtype == torch.float32
    assert torch.equal(rows(qlo), qlo_s) and qlo.dtype == torch.bfloat16
    assert torch.equal(hist, hist_s) and hist.dtype == torch.int32 and tuple(hist.shape) == (k,)
    assert int(hist.sum()) == n
    zc, ec, ic = z.cpu(), e.cpu(), idx.cpu()
    assert int(ic.min()) >= 0 and int(ic.max()) < k
    separated = S.check_acceptance(zc, ec, ic)
    print(f'SIMVQMEASURE {IDS(case)}: separated rows {separated:.4f}')
    if kind == 'random':
        assert separated >= 0.99
    if kind == 'collapsed':
        assert int(ic.max()) < 4                                  # exact ties: the smallest index wins
    assert torch.equal(hist.cpu(), S.hist(ic, k).to(torch.int32))
    assert torch.equal(q_s.cpu(), ec[ic])
    want = S.gradients(zc, ec, c.cpu(), ic, None, BETA)['loss'].item()
    for name, got in (('fp32', loss.item()), ('bf16', loss2.item())):
        print(f'SIMVQMEASURE {IDS(case)} loss {name}: rel err {abs(got - want) / want:.3e}')
        assert abs(got - want) <= 1e-5 * want


@pytest.mark.parametrize('shape', [(300, 32768, 64), (64, 32768, 256)], ids=IDS)
def test_lookup_beyond_the_gather_histogram_and_the_one_kernel_range(shape):
    """K > 16384: the tokens are counted by vqk_simvq_hist_i32 (the gather kernel's LDS histogram ends there) and D = 256 takes the
    staged launches (ops.SIMVQ_ONE_KERNEL_MAX_K); same checks as above, the histogram against a host count"""
    n, k, d = shape
    assert k > ops.SIMVQ_ONE_KERNEL_MAX_K
    z, c, w, b = on_dev(shape + ('random',))
    with torch.no_grad():
        e = ops.simvq_effective(c, w, b)
        q32, idx, loss, hist = ops.SimVQLookupFn.apply(img(z), c, w, b, BETA, torch.float32)
        qlo, idx2, loss2, hist2 = ops.SimVQLookupFn.apply(img(z), c, w, b, BETA, torch.bfloat16)
    torch.cuda.synchronize()
    idx = idx.view(-1)
    assert torch.equal(idx, ops.vq_assign(z, e, 0)) and torch.equal(idx, idx2.view(-1)) and torch.equal(hist, hist2)
    assert torch.equal(rows(q32), e[idx]) and torch.equal(rows(qlo), e[idx].to(torch.bfloat16))
    assert hist.dtype == torch.int32 and int(hist.sum()) == n and torch.equal(hist.cpu(), S.hist(idx.cpu(), k).to(torch.int32))
    S.check_acceptance(z.cpu(), e.cpu(), idx.cpu())
    want = S.gradients(z.cpu(), e.cpu(), c.cpu(), idx.cpu(), None, BETA)['loss'].item()
    assert abs(loss.item() - want) <= 1e-5 * want and abs(loss2.item() - want) <= 1e-5 * want


# ---------------------------------------------------------------------------------------------- 4. backward: dz
@pytest.mark.parametrize('mode', ['f32', 'bf16', 'none'])
@pytest.mark.parametrize('shape', S.SHAPES, ids=IDS)
def test_backward_dz_is_the_standard_backward(shape, mode):
    case = shape + ('random',)
    n, k, d, _ = case
    z, c, w, b = on_dev(case)
    e = device_e(case)
    idx = ops.vq_assign(z, e, 0)
    dq = make_dq(n, d, mode)
    dz, _, _ = raw_backward(z, e, c, idx, dq)
    want = torch.empty_like(z)
    gs = torch.tensor(SCALE, dtype=torch.float32, device=DEV)
    native.check(native.lib().vqk_vq_backward_f32(z.data_ptr(), e.data_ptr(), idx.data_ptr(), ops._p(dq),
                                                  ops.dcode(dq.dtype) if dq is not None else ops.F32, n, k, d, 2.0 * BETA / (n * d),
                                                  2.0 / (n * d), gs.data_ptr(), want.data_ptr(), 0, ops._stream()), 'vq_backward')
    torch.cuda.synchronize()
    assert torch.equal(dz, want)
    ref = S.gradients(z.cpu(), e.cpu(), c.cpu(), idx.cpu(), dq.float().cpu() if dq is not None else None, BETA, SCALE)
    np.testing.assert_allclose(dz.cpu().double().numpy(), ref['dz'].numpy(), rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------------------------------------- 5. backward: dW, db
@pytest.mark.parametrize('target', ['fresh', 'arena'])
@pytest.mark.parametrize('case', S.cases(['random', 'collapsed']), ids=IDS)
def test_backward_dw_db_within_the_summation_bound(case, target):
    n, k, d, kind = case
    z, c, w, b = on_dev(case)
    e = device_e(case)
    idx = ops.vq_assign(z, e, 0)
    dq = make_dq(n, d, 'f32')
    old_w = old_b = None
    if target == 'arena':                                         # a view of a larger buffer that already holds values
        arena = torch.randn(5 + d * d + d, generator=torch.Generator().manual_seed(3)).to(DEV)
        dw0, db0 = arena[4:4 + d * d].view(d, d), arena[4 + d * d:4 + d * d + d]
        old_w, old_b = dw0.clone(), db0.clone()
        dz, dw, db = raw_backward(z, e, c, idx, dq, dw0, db0)
        assert float(arena[:4].abs().min()) > 0.0 and dw.data_ptr() == dw0.data_ptr()
    else:
        dz, dw, db = raw_backward(z, e, c, idx, dq)
    ref = S.gradients(z.cpu(), e.cpu(), c.cpu(), idx.cpu(), dq.cpu(), BETA, SCALE)
    bw, bb = S.gradient_bounds(ref, n)
    want_w, want_b = ref['dw'], ref['db']
    if target == 'arena':
        want_w, want_b = want_w + old_w.cpu().double(), want_b + old_b.cpu().double()
        bw, bb = bw + S.U * want_w.abs(), bb + S.U * want_b.abs()
    within(f'{IDS(case)} {target} dW', dw.cpu(), want_w, bw)
    within(f'{IDS(case)} {target} db', db.cpu(), want_b, bb)
    if target == 'fresh':                                         # db is optional: dW is the same without it
        _, dw2, none = raw_backward(z, e, c, idx, dq, want_db=False)
        assert none is None and torch.equal(dw2, dw)


# ---------------------------------------------------------------------------------------------- 6. reproducibility
def _grads(case, dtype=torch.float32):
    n, k, d, _ = case
    z, c, w, b = on_dev(case)
    x = img(z).detach().requires_grad_(True)
    wp, bp = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    q, idx, loss, hist = ops.SimVQLookupFn.apply(x, c, wp, bp, BETA, dtype)
    dq = img(make_dq(n, d, 'bf16' if dtype == torch.bfloat16 else 'f32'))
    dz, dw, db = torch.autograd.grad([loss, q], [x, wp, bp], [torch.ones((), device=DEV), dq])
    torch.cuda.synchronize()
    return dict(idx=idx.view(-1), q=rows(q), loss=loss.detach(), hist=hist, dz=rows(dz), dw=dw, db=db)


@pytest.mark.parametrize('deterministic', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('shape', [(77, 96, 64), (2051, 1024, 256)], ids=IDS)
def test_two_runs_give_the_same_bits(shape, deterministic):
    ops.set_deterministic(deterministic)
    try:
        a, b = _grads(shape + ('random',)), _grads(shape + ('random',))
    finally:
        ops.set_deterministic(False)
    for name in ('idx', 'q', 'hist', 'dz', 'dw', 'db'):
        assert torch.equal(a[name], b[name]), name
    assert float(a['dw'].abs().max()) > 0.0 and float(a['db'].abs().max()) > 0.0


def test_default_and_deterministic_mode_give_the_same_gradient_bits():
    case = (2051, 1024, 256, 'random')
    a = _grads(case)
    ops.set_deterministic(True)
    try:
        b = _grads(case)
    finally:
        ops.set_deterministic(False)
    assert torch.equal(a['dw'], b['dw']) and torch.equal(a['db'], b['db']) and torch.equal(a['dz'], b['dz'])


# ---------------------------------------------------------------------------------------------- 7. out-of-range tokens
@pytest.mark.parametrize('shape', [(77, 96, 64), (64, 32, 256)], ids=IDS)
def test_out_of_range_tokens_are_zero_codes(shape):
    case = shape + ('random',)
    n, k, d, _ = case
    z, c, w, b = on_dev(case)
    e = device_e(case)
    good = ops.vq_assign(z, e, 0)
    idx = good.clone()
    bad = torch.tensor([0, 5, 31, 32, n - 1])
    idx[bad.to(DEV)] = torch.tensor([-1, k, k + 5, -7, 1 << 40], dtype=torch.int64, device=DEV)
    dq = make_dq(n, d, 'f32')
    dz, dw, db = raw_backward(z, e, c, idx, dq)
    dz_good, _, _ = raw_backward(z, e, c, good, dq)
    keep = torch.ones(n, dtype=torch.bool)
    keep[bad] = False
    assert torch.equal(dz[keep.to(DEV)], dz_good[keep.to(DEV)])
    ref = S.gradients(z.cpu(), e.cpu(), c.cpu(), idx.cpu(), dq.cpu(), BETA, SCALE)
    np.testing.assert_allclose(dz.cpu().double().numpy(), ref['dz'].numpy(), rtol=1e-5, atol=1e-7)
    bw, bb = S.gradient_bounds(ref, n)
    within(f'{IDS(case)} out-of-range dW', dw.cpu(), ref['dw'], bw)
    within(f'{IDS(case)} out-of-range db', db.cpu(), ref['db'], bb)


# ---------------------------------------------------------------------------------------------- 8. fused vs staged
def _switch(case, fused_on, dtype=torch.float32):
    saved = ops.SIMVQ_FUSED
    ops.SIMVQ_FUSED = fused_on
    try:
        assert ops.simvq_fused_serves(on_dev(case)[1]) == fused_on
        return _grads(case, dtype)
    finally:
        ops.SIMVQ_FUSED = saved


@pytest.mark.parametrize('shape', S.SHAPES, ids=IDS)
def test_fused_equals_staged_on_the_same_e(shape):
    """identity: the staged E (torch.addmm with W = I, b = 0) and the projected E are both C as numbers, so both paths rank the same
    codebook: idx, q and hist are identical; each path's gradients lie within the bounds of the float64 terms"""
    case = shape + ('identity',)
    n, k, d, _ = case
    z, c, w, b = S.make_case(*case)
    for dtype in (torch.float32, torch.bfloat16):
        f, s = _switch(case, True, dtype), _switch(case, False, dtype)
        for name in ('idx', 'q', 'hist'):
            assert torch.equal(f[name], s[name]), name
        assert abs(f['loss'].item() - s['loss'].item()) <= 1e-5 * s['loss'].item()
    dq = make_dq(n, d, 'bf16').float().cpu()
    ref = S.gradients(z, c, c, f['idx'].cpu(), dq, BETA)
    bw, bb = S.gradient_bounds(ref, n)
    for name, got in (('fused', f), ('staged', s)):
        within(f'{IDS(case)} {name} dW', got['dw'].cpu(), ref['dw'], bw)
        within(f'{IDS(case)} {name} db', got['db'].cpu(), ref['db'], bb)
        np.testing.assert_allclose(got['dz'].cpu().double().numpy(), ref['dz'].numpy(), rtol=1e-5, atol=1e-7)


def test_fused_and_staged_agree_on_a_random_layer():
    """two evaluations of E in different summation orders: the rows they rank apart are near-ties; loss and gradients agree closely"""
    case = (2051, 1024, 256, 'random')
    f, s = _switch(case, True), _switch(case, False)
    same = float((f['idx'] == s['idx']).double().mean())
    print(f'SIMVQMEASURE fused vs staged {IDS(case)}: equal tokens {same:.4f}')
    assert same >= 0.99
    assert abs(f['loss'].item() - s['loss'].item()) <= 1e-5 * s['loss'].item()


# ---------------------------------------------------------------------------------------------- 9. the staged path alone
def test_staged_path_serves_other_shapes():
    n, k, d = S.STAGED_SHAPE
    for kind in ('random', 'nobias'):
        z, c, w, b = S.make_case(n, k, d, kind)
        dq = torch.randn(n, d, generator=torch.Generator().manual_seed(11))
        cd, x = c.to(DEV), img(z.to(DEV)).detach().requires_grad_(True)
        assert not ops.simvq_fused_serves(cd)
        wp = w.to(DEV).requires_grad_(True)
        bp = b.to(DEV).requires_grad_(True) if b is not None else None
        q, idx, loss, hist = ops.SimVQLookupFn.apply(x, cd, wp, bp, BETA, torch.float32)
        grads = torch.autograd.grad([loss, q], [x, wp] + ([bp] if bp is not None else []), [torch.ones((), device=DEV), img(dq.to(DEV))])
        e = ops.simvq_effective(cd, wp, bp).cpu()
        within(f'staged {kind} E', e, S.effective(c, w, b), S.projection_bound(c, w, b))
        idx = idx.view(-1).cpu()
        S.check_acceptance(z, e, idx)
        assert torch.equal(rows(q).cpu(), e[idx]) and int(hist.sum()) == n and torch.equal(hist.cpu(), S.hist(idx, k).to(torch.int32))
        ref = S.gradients(z, e, c, idx, dq, BETA)
        assert abs(loss.item() - ref['loss'].item()) <= 1e-5 * ref['loss'].item()
        np.testing.assert_allclose(rows(grads[0]).cpu().double().numpy(), ref['dz'].numpy(), rtol=1e-5, atol=1e-7)
        bw, bb = S.gradient_bounds(ref, n)
        within(f'staged {kind} dW', grads[1].cpu(), ref['dw'], bw)
        if bp is not None:
            within(f'staged {kind} db', grads[2].cpu(), ref['db'], bb)


# ---------------------------------------------------------------------------------------------- 10. graph replay
@pytest.mark.parametrize('shape', [(2051, 1024, 256), (256, 4096, 128)], ids=IDS)
def test_captured_forward_backward_replays(shape):
    n, k, d = shape
    z0, c, w0, b0 = on_dev(shape + ('random',))
    gen = torch.Generator().manual_seed(23)
    dq0 = torch.randn(n, d, generator=gen).to(DEV)
    step = (torch.randn(d, d, generator=gen) * 0.5 * d ** -0.5).to(DEV)        # what optimizer steps do to W

    def run(z, wp, bp, dq):
        q, idx, loss, hist = ops.SimVQLookupFn.apply(img(z), c, wp, bp, BETA, torch.float32)
        dz, dw, db = torch.autograd.grad([q, loss], [z, wp, bp], [img(dq), torch.ones((), device=DEV)])
        return q, idx, loss, hist, dz, dw, db

    wp, bp = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
    z = z0.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(z, wp, bp, dq0)                                               # first launches and workspaces: outside the capture
        torch.cuda.synchronize()
        graph, update = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = run(z, wp, bp, dq0)
        with torch.cuda.graph(update, stream=side):
            with torch.no_grad():
                wp.add_(step)
    torch.cuda.current_stream().wait_stream(side)
    for round_ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.detach().clone() for t in got]
        want = run(z, wp, bp, dq0)
        torch.cuda.synchronize()
        for name, a, b in zip(('q', 'idx', 'loss', 'hist', 'dz', 'dw', 'db'), replayed, want):
            if name == 'loss':                                            # the one sum that arrives in arrival order
                assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item())
            else:
                assert torch.equal(a, b), (round_, name)
        if round_ == 0:
            first_idx = replayed[1]
            update.replay()                 # W changes under the captured step: the projection and the prepare launch are INSIDE it
    assert not torch.equal(first_idx, replayed[1])                        # the second replay ranked against the NEW E


# ---------------------------------------------------------------------------------------------- 11. model level
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)


def _qc(dim, k=64, bias=True):
    return dict(num_embeddings=k, embedding_dim=dim, reinit_every_n_epochs=None, type='simvq',
                params=dict(commitment_cost=0.25, proj_bias=bias))


def _images(seed=3, b=4):
    return torch.rand(b, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize('dtype,dim,bias', [(torch.float32, 64, True), (torch.bfloat16, 64, False), (torch.bfloat16, 256, True)],
                         ids=['fp32-D64', 'bf16-D64-nobias', 'bf16-D256'])
def test_model_step_tokens_roundtrip_and_checkpoint(dtype, dim, bias, tmp_path):
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, AE, _qc(dim, bias=bias), None, TC, compute_dtype=dtype).to(DEV).train()
    qz = m.quantizer
    assert ops.simvq_fused_serves(qz.codebook.weight)
    tr = trainer_mod.MiniTrainer(num_training_batches=10)
    tr.attach(m)
    m.on_train_start()
    images = _images()
    table = qz.codebook.weight.detach().clone()
    w_before = qz.codebook_proj.weight.detach().clone()
    assert torch.equal(w_before, torch.eye(dim, device=DEV))
    for step in range(3):
        loss = tr.train_batch(m, images, step)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and float(m.logged['train/quant_loss']) > 0.0
    assert torch.equal(qz.codebook.weight.detach(), table)                 # the frozen table: bit-identical after three steps
    assert not torch.equal(qz.codebook_proj.weight.detach(), w_before)     # the layer has moved
    assert (qz.codebook_proj.bias is not None) == bias
    if bias:
        assert float(qz.codebook_proj.bias.detach().abs().max()) > 0.0
    assert qz.last_hist.numel() == 64 and int(qz.last_hist.sum()) == 4 * 64

    m.eval()
    with torch.no_grad():
        tokens = m.get_tokens(images)
        assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (4, 64)
        e = qz.get_codebook()
        assert tuple(e.shape) == (64, dim) and not torch.equal(e, table)
        vec = m.quantize(images)
        assert torch.equal(vec, e[tokens])
        assert torch.equal(qz.codes_to_vec(tokens), e[tokens])
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
    with pytest.raises(RuntimeError):
        qz.reinit_unused_codes(torch.ones(64, device=DEV))
    path = str(tmp_path / 'simvq.ckpt')
    tr.save_checkpoint(m, path)
    torch.manual_seed(1)
    m2 = model_mod.VQVAE(32, AE, _qc(dim, bias=bias), None, TC, compute_dtype=dtype).to(DEV)
    t2 = trainer_mod.MiniTrainer(num_training_batches=10)
    t2.attach(m2)
    t2.load_checkpoint(m2, path)
    m2.eval()
    assert torch.equal(m2.quantizer.codebook.weight, qz.codebook.weight)
    assert torch.equal(m2.quantizer.codebook_proj.weight, qz.codebook_proj.weight)
    assert torch.equal(m2.get_tokens(images), tokens)


# ---------------------------------------------------------------------------------------------- 12. entry points
SMALL = ['--set', 'image_size=32', '--set', 'autoencoder.channels=32', '--set', 'autoencoder.num_res_blocks=1',
         '--set', 'autoencoder.channel_multipliers=[1, 2]', '--set', 'quantizer.num_embeddings=64', '--set', 'training.cumulative_bs=4']


def test_entry_points(tmp_path, capsys):
    train = importlib.import_module(PKG + '.train')
    ev = importlib.import_module(PKG + '.evaluate')
    conf = os.path.join(ROOT, 'example_confs', 'simvq_vqvae.yaml')
    common = ['--params_file', conf] + SMALL + ['--max_epochs', '1', '--batches_per_epoch', '2', '--seed', '0', '--dtype', 'f32']
    capsys.readouterr()
    loss = train.main(common + ['--save_path', str(tmp_path), '--run_name', 'simvq'])
    out = capsys.readouterr().out
    assert loss is not None and np.isfinite(loss)
    assert 'eager launches' not in out                                                  # the graph was captured, not given up
    ckpt = str(tmp_path / 'simvq' / 'epoch=00.ckpt')
    assert os.path.exists(ckpt)
    small = tmp_path / 'conf.yaml'
    small.write_text('image_size: 32\nautoencoder:\n  channels: 32\n  num_res_blocks: 1\n  channel_multipliers: [1, 2]\n'
                     'quantizer:\n  num_embeddings: 64\n  embedding_dim: 256\n  type: simvq\n  params:\n'
                     '    commitment_cost: 0.25\n    proj_bias: true\n  reinit_every_n_epochs:\n')
    pt = str(tmp_path / 'test.pt')
    torch.save(torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(5)), pt)
    capsys.readouterr()
    res = ev.main(['--params_file', str(small), '--batch_size', '4', '--seed', '0', '--loading_path', ckpt, '--dtype', 'f32',
                   '--dataset_path', pt])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert json.loads(lines[-1]) == res
    assert {'mse', 'psnr', 'ssim', 'used_codebook', 'perplexity'} <= set(res)
    assert 0.0 < res['used_codebook'] <= 100.0 and 1.0 <= res['perplexity'] <= 64.0
