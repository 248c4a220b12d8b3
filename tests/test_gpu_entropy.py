"""The Entropy quantizer on the GPU (csrc/entropy.hip, the statistics epilogues of the two distance kernels of csrc/vq.hip, EntropyVQFn
in _ops_vq.py) against the float64 reference of tests/entropy_reference.py; cases, shared references and bounds are in
tests/entropy_cases.py.

(a) the row / column kernels through the C ABI on a matrix built on the host: that fp32 matrix is the exact input of the device and of
    the reference, so the distance kernels' rounding does not enter.  The backward kernels get the REFERENCE's lse / hrow / u (rounded
    to fp32), so a forward defect cannot hide a backward one or the other way round.  The split kernel's hi must be bf16(dd) of the
    device's own fp32 dd bit for bit and hi + lo reproduce it to 2^-16 |dd| elementwise.
(b) the statistics epilogues of the distance kernels, register and LDS form: lse / hrow / hsum against the float64 rows of the matrix
    THAT CALL wrote, idx against that matrix's first minimum.
(c) EntropyVQFn end to end against ``entropy_vq``: q, idx on every row, loss, hist, dz, dE, with dq alone, the loss alone and both; a
    spy on the C ABI asserts which kernels each case ran, so that a changed dispatch rule cannot silently move a case.

Tokens are integers: the device must return the reference's on every row (the makers redraw rows until the float64 margin between the
nearest and the second-nearest code is 1e-4 max(1, max d), and plant one exact tie whose lower index must win).  Real-valued results are
compared in max|got - want| / max|want|, against max(16 e32, floor) (tests/entropy_cases.py).  Every figure is printed (``ENTMEASURE``)
before it is asserted.

Where max(16 e32, floor) >= 1 it says nothing -- with ONE row the 'softmax' loss is zero up to the 1e-5 inside the logarithm (a row's
entropy is the entropy of its mean) and its cotangent ~1e-8 of its terms -- so there the device's value is held, as well, to 16 times
the larger of the two evaluations' magnitudes (``check``, as in tests/test_gpu_lfq.py).

Invariants these tests hold beyond the values: log p = -d / T - lse is ONE fma at every site of csrc/entropy.hip (``ent_logp``), so the
fp32 and the split form of the cotangent see the same p and hi is bf16(dd) bit for bit; the VQ_LDS slot changes the kernel exactly where
the LDS form applies.

Measured on an MI355X, largest e32 / largest device distance over the cases.  (a) lse 8.4e-8 / 7.5e-8, hrow 2.8e-5 / 3.5e-6, hsum
2.8e-5 / 2.3e-6, psum 1.9e-6 / 6.5e-7, u 1.9e-6 / 4.8e-7, avg_term 4.1e-6 / 2.1e-7; argmax forward ssum 2.3e-6 / 6.8e-7, u 1.2e-7 /
3.5e-7, avg_term 1.4e-3 / 1.4e-3 (one row: log(1 + 1e-5) in float32); dd softmax 3.2e-5 / 9.2e-6, dd argmax 2.9e-6 / 3.4e-6; the one-row
softmax dd (vacuous bound): distance 45 against 56 and max|device| 1.2e-6 against 1.5e-6 at T = 0.01, 419 against 758 and 1.7e-8
against 3.2e-8 at T = 1; hi + lo against dd 7.4e-6 of an element (bound 1.5e-5), hi bit-equal at all sixteen cases; row_scale_add
8.8e-8 / 5.0e-8.  (b) lse 7.7e-8 / 7.6e-8, hrow 9.1e-6 / 2.3e-6 (largest bound 1.5e-4), hsum 5.8e-7 / 2.4e-7; the LDS slot changes
lse / hrow bits at the four LDS shapes and none at (96, 104).  (c) q exact, loss over its largest term 2.5e-6 / 4.3e-7, relative to
itself at most 7.2e-7 (bounds 1.1e-5 to 8.9e-5); dz 2.1e-5 / 3.1e-5 and dE 5.0e-6 / 1.0e-5 (N = 259, K = 128, D = 256, loss alone);
split-product route max(e32, e_split) 1.8e-5 / dz 2.3e-5, 5.7e-6 / dE 6.4e-6.  Every case is inside its bound; the closest are the two
figures of the one-row softmax dd at T = 0.01 (0.80 of their bounds, a deterministic kernel), then the argmax u at N = 4115, K = 8,
T = 1: 3.5e-7 against 1.6e-6."""
import importlib

import numpy as np
import pytest
import torch

from tests import entropy_cases as C
from tests import entropy_reference as R
from tests import test_gpu_vq_lds as L

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
DEV = 'cuda:0'


def t32(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float32, device=DEV)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def check(name, case, got, want64, want32, floor=1e-6, extra=''):
    e32, dist = R.distance(want32, want64), R.distance(got, want64)
    b = C.bound(e32, floor)
    print(f'ENTMEASURE {name} {case} {extra} e32 {e32:.3e} device {dist:.3e} bound {b:.3e}')
    assert dist <= b, (name, case, extra, dist, b)
    if b >= 1.0:
        # the bound says nothing: the float64 value is what cancellation left of terms many orders larger (one row: its entropy IS the
        # entropy of its mean, the 'softmax' loss and its gradient are what the 1e-5 inside the logarithm leaves) and float32 keeps none
        # of its digits.  What can still be asked: the device's value is as small as the two evaluations', not of the terms' order
        small = 16.0 * max(np.abs(np.asarray(want64, dtype=np.float64)).max(), np.abs(np.asarray(want32, dtype=np.float64)).max())
        got_max = float(np.abs(np.asarray(got, dtype=np.float64)).max())
        print(f'ENTMEASURE {name} {case} {extra} vacuous relative bound: max|device| {got_max:.3e} against {small:.3e}')
        assert got_max <= small, (name, case, got_max, small)


# ----------------------------------------------------------------------------------------------------------------------------------
# (a)
# ----------------------------------------------------------------------------------------------------------------------------------
ROWCOL = [pytest.mark.parametrize('temp', C.ROWCOL_TEMPS, ids=lambda t: f'T{t[0]}'),
          pytest.mark.parametrize('shape', C.ROWCOL_SHAPES, ids=C.rowcol_id)]
F = dict(dtype=torch.float32, device=DEV)


def rowcol(f):
    for mark in ROWCOL:
        f = mark(f)
    return f


def rowcol_cmp(shape, temp):
    """(reference of the case, compare(name, device tensor, key of the reference, extra))"""
    ref = C.rowcol_reference(shape, temp)
    case = f'{C.rowcol_id(shape)}-T{temp[0]}'

    def cmp(name, got, key=None, extra=''):
        key = key or name
        check(name, case, host(got), ref['f64'][key], ref['f32'][key], ref['floor'].get(key, 1e-6), extra)
    return ref, cmp


@rowcol
def test_row_and_column_kernels_forward(shape, temp):
    (n, k), t = shape, temp[0]
    ref, cmp = rowcol_cmp(shape, temp)
    lib, st = native.lib(), ops._stream()
    d = t32(ref['d'])
    # 'softmax'
    lse, hrow, psum, u, scal = torch.empty(n, **F), torch.empty(n, **F), torch.zeros(k, **F), torch.empty(k, **F), torch.zeros(2, **F)
    native.check(lib.vqk_entropy_forward_f32(d.data_ptr(), n, k, t, lse.data_ptr(), hrow.data_ptr(), scal[0:1].data_ptr(), psum.data_ptr(),
                                             u.data_ptr(), scal[1:2].data_ptr(), st), 'entropy_forward')
    torch.cuda.synchronize()
    assert torch.equal(d, t32(ref['d']))                                # the forward leaves the matrix alone
    for name, got in (('lse', lse), ('hrow', hrow), ('hsum', scal[0]), ('psum', psum), ('u', u), ('avg', scal[1])):
        cmp(name, got)
    # 'argmax' (idx and hist are inputs)
    idx = torch.tensor(ref['idx'], dtype=torch.int64, device=DEV)
    hist = torch.tensor(ref['hist'], dtype=torch.int32, device=DEV)
    lse2, hrow2, mbuf, u2, scal2 = torch.empty(n, **F), torch.empty(n, **F), torch.empty(k, **F), torch.empty(k, **F), torch.zeros(3, **F)
    native.check(lib.vqk_entropy_argmax_forward_f32(d.data_ptr(), idx.data_ptr(), hist.data_ptr(), n, k, t, lse2.data_ptr(), hrow2.data_ptr(),
                                                    scal2[0:1].data_ptr(), scal2[1:2].data_ptr(), mbuf.data_ptr(), u2.data_ptr(),
                                                    scal2[2:3].data_ptr(), st), 'entropy_argmax_forward')
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(mbuf), ref['f64']['m'])
    for name, got in (('lse', lse2), ('hrow', hrow2), ('hsum', scal2[0]), ('ssum', scal2[1]), ('u_am', u2), ('avg_am', scal2[2])):
        cmp(name, got, extra='argmax-forward')


def reference_stats(ref):
    f64 = ref['f64']
    return t32(f64['lse']), t32(f64['hrow']), t32(f64['u']), t32(f64['u_am'])


@rowcol
def test_row_kernels_backward(shape, temp):
    """both forms; gs = 1 is passed as NO device scalar, gs = 1.7 as one"""
    (n, k), t = shape, temp[0]
    ref, cmp = rowcol_cmp(shape, temp)
    lib, st = native.lib(), ops._stream()
    d = t32(ref['d'])
    idx = torch.tensor(ref['idx'], dtype=torch.int64, device=DEV)
    lse_r, hrow_r, u_r, u_am_r = reference_stats(ref)
    for gs in C.GS_VALUES:
        g = t32([gs]) if gs != 1.0 else None
        dm, da = d.clone(), d.clone()
        native.check(lib.vqk_entropy_backward_f32(dm.data_ptr(), lse_r.data_ptr(), hrow_r.data_ptr(), u_r.data_ptr(), n, k, t, C.RATIO,
                                                  ops._p(g), st), 'entropy_backward')
        native.check(lib.vqk_entropy_argmax_backward_f32(da.data_ptr(), idx.data_ptr(), lse_r.data_ptr(), hrow_r.data_ptr(), u_am_r.data_ptr(),
                                                         n, k, t, C.RATIO, ops._p(g), st), 'entropy_argmax_backward')
        torch.cuda.synchronize()
        cmp('dd-softmax', dm, f'dd-softmax-{gs}', extra=f'gs={gs}')
        cmp('dd-argmax', da, f'dd-argmax-{gs}', extra=f'gs={gs}')


@rowcol
def test_split_kernel_splits_the_fp32_cotangent(shape, temp):
    """hi = bf16(dd) of the device's own fp32 dd (vqk_entropy_backward_f32 on the same inputs) bit for bit; hi + lo reproduces it to
    2^-16 |dd| elementwise (2^-133 more: the spacing of bf16 below the smallest normal, where lo of a vanishing dd lives)"""
    (n, k), t = shape, temp[0]
    ref = C.rowcol_reference(shape, temp)
    lib, st = native.lib(), ops._stream()
    d, g = t32(ref['d']), t32([C.GLOSS])
    lse_r, hrow_r, u_r, _ = reference_stats(ref)
    dd = d.clone()
    native.check(lib.vqk_entropy_backward_f32(dd.data_ptr(), lse_r.data_ptr(), hrow_r.data_ptr(), u_r.data_ptr(), n, k, t, C.RATIO,
                                              g.data_ptr(), st), 'entropy_backward')
    hi, lo = torch.empty((n, k), dtype=torch.bfloat16, device=DEV), torch.empty((n, k), dtype=torch.bfloat16, device=DEV)
    native.check(lib.vqk_entropy_backward_split_f32(d.data_ptr(), lse_r.data_ptr(), hrow_r.data_ptr(), u_r.data_ptr(), n, k, t, C.RATIO,
                                                    g.data_ptr(), hi.data_ptr(), lo.data_ptr(), st), 'entropy_backward_split')
    torch.cuda.synchronize()
    assert torch.equal(d, t32(ref['d']))                                # the split form leaves the matrix alone
    assert torch.equal(hi, dd.to(torch.bfloat16))
    dd64 = host(dd)
    err = np.abs(host(hi) + host(lo) - dd64)
    worst = float((err / np.maximum(np.abs(dd64), 1e-300)).max()) if dd64.any() else 0.0
    print(f'ENTMEASURE split-hi+lo {C.rowcol_id(shape)}-T{t} max |hi + lo - dd| / |dd| {worst:.3e} bound {2.0 ** -16:.3e}')
    assert (err <= 2.0 ** -16 * np.abs(dd64) + 2.0 ** -133).all()


@pytest.mark.parametrize('shape', C.RSA_SHAPES, ids=lambda s: f'rows{s[0]}-c{s[1]}')
def test_row_scale_add(shape):
    rows, c = shape
    ref = C.rsa_reference(shape)
    o, mm, sc = t32(ref['out']), t32(ref['m']), t32(ref['scale'])
    native.check(native.lib().vqk_row_scale_add_f32(o.data_ptr(), mm.data_ptr(), sc.data_ptr(), rows, c, 2.0, ops._stream()), 'row_scale_add')
    torch.cuda.synchronize()
    check('row_scale_add', f'rows{rows}-c{c}', host(o), ref['f64'], ref['f32'])


# ----------------------------------------------------------------------------------------------------------------------------------
# (b)
# ----------------------------------------------------------------------------------------------------------------------------------
def stats_run(shape, t, slot):
    inp = C.stats_inputs(shape, t)
    return L._run(t32(inp['z']), t32(inp['e']), t, True, slot)


@pytest.mark.parametrize('slot', [0, 1], ids=['slot0', 'slot1'])
@pytest.mark.parametrize('t', list(C.STATS_TEMPS))
@pytest.mark.parametrize('shape', C.STATS_SHAPES, ids=C.rowcol_id)
def test_statistics_epilogue_of_the_distance_kernels(shape, t, slot):
    n, k = shape
    idx, dm, lse, hrow, hsum = stats_run(shape, t, slot)
    case = f'N{n}-K{k}-T{t}-{"lds" if C.stats_lds_form(n, k, slot) else "register"}'
    dmat = host(dm)
    np.testing.assert_array_equal(idx.cpu().numpy(), dmat.argmin(-1))   # first minimum of the matrix this call wrote, every row
    assert int(idx[3]) == 3 and dmat[3, 3] == dmat[3, 5]
    w64, w32, bounds = C.stats_reference(dmat, t)
    floor = R.atomic_bound(w64[1], n)
    assert max(bounds) <= 1e-3, bounds                                  # as tests/test_entropy_cpu.py found for the host's matrix
    check('stats-lse', case, host(lse), w64[0], w32[0])
    check('stats-hrow', case, host(hrow), w64[1], w32[1])
    check('stats-hsum', case, host(hsum)[0], w64[2], w32[2], floor)


@pytest.mark.parametrize('shape', C.STATS_SHAPES, ids=C.rowcol_id)
def test_the_lds_slot_changes_the_kernel_exactly_where_the_lds_form_applies(shape):
    """A witness of which form ran.  Both forms write the same matrix and indices bit for bit (tests/test_gpu_vq_lds.py) but reduce the
    row statistics over another partition of the codes, so lse / hrow differ in their last bits in some row; where the LDS form does
    not apply (96 rows, 104 codes) slot 1 runs the register kernel and every bit agrees.  A changed dispatch guard that moved the
    LDS cases of the test above onto one kernel would fail here."""
    n, k = shape
    a, b = stats_run(shape, 0.01, 0), stats_run(shape, 0.01, 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    same = torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert same != C.stats_lds_form(n, k, 1), (shape, same)


# ----------------------------------------------------------------------------------------------------------------------------------
# (c)
# ----------------------------------------------------------------------------------------------------------------------------------
SPIED = ('vqk_vq_distances_stats_f32', 'vqk_vq_distances_f32', 'vqk_entropy_forward_presummed_f32', 'vqk_entropy_forward_f32',
         'vqk_entropy_argmax_forward_f32', 'vqk_vq_backward_fused_f32', 'vqk_vq_backward_f32', 'vqk_entropy_backward_split_f32',
         'vqk_entropy_backward_f32', 'vqk_entropy_argmax_backward_f32')


def spy(monkeypatch):
    """record which of the quantizer's C ABI entries are called (each call is forwarded)"""
    lib, calls = native.lib(), []
    for name in SPIED:
        def wrapper(*a, _f=getattr(lib, name), _n=name):
            calls.append(_n)
            return _f(*a)
        monkeypatch.setattr(lib, name, wrapper)
    return calls


def expected_calls(case, with_loss):
    n, k, dim, _, _, lt, _ = case
    fused_rows = lt == 'softmax' and dim == 256
    fwd = ['vqk_vq_distances_stats_f32' if fused_rows else 'vqk_vq_distances_f32',
           'vqk_entropy_forward_presummed_f32' if fused_rows else
           'vqk_entropy_forward_f32' if lt == 'softmax' else 'vqk_entropy_argmax_forward_f32']
    bwd = ['vqk_vq_backward_fused_f32' if dim == 256 else 'vqk_vq_backward_f32']
    if with_loss:
        bwd += ['vqk_vq_distances_f32', 'vqk_entropy_backward_split_f32' if C.vq_split_route(case) else
                'vqk_entropy_backward_f32' if lt == 'softmax' else 'vqk_entropy_argmax_backward_f32']
    return fwd, bwd


@pytest.mark.parametrize('setting', list(C.VQ_SETTINGS))
@pytest.mark.parametrize('case', C.VQ_CASES, ids=C.vq_id)
def test_entropy_vq_function(case, setting, monkeypatch):
    n, k, dim, t, dt, lt, split_on = case
    ref = C.vq_reference(case)
    ent, inp = ref[setting], ref['inp']
    f64, f32 = ent['f64'], ent['f32']
    use_dq, gloss = C.VQ_SETTINGS[setting]
    tdt = torch.bfloat16 if dt == 'bf16' else torch.float32
    cid = C.vq_id(case)
    assert ops.ENTROPY_SPLIT_GEMM and ops.ENTROPY_FUSED_ROWS and ops.VQ_FUSED and not ops.DETERMINISTIC      # the shipped defaults
    monkeypatch.setattr(ops, 'ENTROPY_SPLIT_GEMM', split_on)
    calls = spy(monkeypatch)
    rows = lambda a: t32(a).view(1, n, 1, dim).permute(0, 3, 1, 2)
    z, e = rows(inp['z']).requires_grad_(True), t32(inp['E']).requires_grad_(True)
    q, idx, loss, hist = ops.EntropyVQFn.apply(z, e, C.BETA, C.RATIO, t, tdt, lt)
    torch.cuda.synchronize()
    fwd, bwd = expected_calls(case, True)                               # (autograd materialises an absent cotangent as zeros)
    assert calls == fwd, calls
    assert q.grad_fn.split_gemm == C.vq_split_route(case)
    assert q.dtype == tdt and tuple(q.shape) == (1, dim, n, 1) and tuple(idx.shape) == (1, n) and loss.dtype == torch.float32

    np.testing.assert_array_equal(idx.reshape(-1).cpu().numpy(), f64['idx'])          # every row, the planted tie's row 0 included
    a, b = inp['tie']
    assert f64['idx'][0] == a and np.array_equal(inp['E'][a], inp['E'][b])
    assert hist.dtype == torch.int32
    np.testing.assert_array_equal(hist.cpu().numpy(), f64['hist'])
    qrows = host(q.permute(0, 2, 3, 1).reshape(n, dim))
    if dt == 'bf16':
        np.testing.assert_array_equal(qrows, R.bf16(f64['q']))
    else:
        check('q', cid, qrows, f64['q'], f32['q'])
    scale, e32, lb, plain = C.vq_loss_bound(case, ref)
    dist = abs(float(loss.detach()) - float(ref['both']['f64']['loss'])) / scale
    print(f'ENTMEASURE loss {cid} e32 {e32:.3e} device {dist:.3e} bound {lb:.3e} (over the largest term {scale:.3e})')
    assert dist <= lb
    pdist = R.distance(float(loss.detach()), float(ref['both']['f64']['loss']))
    print(f'ENTMEASURE loss-plain {cid} device {pdist:.3e} bound {plain:.3e} (relative to the loss itself)')
    assert pdist <= plain                                               # the same inequality; it discriminates where plain <= 1e-3

    del calls[:]
    outs, cots = [], []
    if use_dq:
        outs.append(q)
        cots.append(rows(ref['dq_in']).to(tdt))
    if gloss is not None:
        outs.append(loss)
        cots.append(t32(gloss))
    dz, de = torch.autograd.grad(outs, [z, e], cots, retain_graph=True)
    torch.cuda.synchronize()
    assert calls == bwd, calls
    results = [('autograd', dz, de)]
    if gloss is None:                                                   # the same with the loss cotangent truly ABSENT (None)
        del calls[:]
        dz2, de2 = ops.EntropyVQFn.backward(q.grad_fn, cots[0], None, None, None)[:2]
        torch.cuda.synchronize()
        assert calls == expected_calls(case, False)[1], calls
        results.append(('dloss=None', dz2, de2))
    for how, gz, ge in results:
        assert gz.dtype == torch.float32 and ge.dtype == torch.float32
        for key, got in (('dz', host(gz.permute(0, 2, 3, 1).reshape(n, dim))), ('dE', host(ge))):
            if not np.any(f64[key]):
                assert not got.any(), (key, how)                        # no loss cotangent: the codebook gradient is exactly zero
                continue
            e32, es, b = C.vq_grad_bound(ent, key)
            dist = R.distance(got, f64[key])
            print(f'ENTMEASURE {key} {cid} {setting} {how} e32 {e32:.3e} e_split {es if es is None else format(es, ".3e")} '
                  f'device {dist:.3e} bound {b:.3e}')
            assert dist <= b, (key, cid, setting, how, dist, b)


def test_a_codebook_size_that_is_no_multiple_of_four_is_refused():
    z = torch.zeros(1, 16, 8, 1, device=DEV)
    with pytest.raises(RuntimeError, match='num_embeddings % 4 == 0'):
        ops.EntropyVQFn.apply(z, torch.zeros(66, 16, device=DEV), C.BETA, C.RATIO, 1.0, torch.float32, 'softmax')
