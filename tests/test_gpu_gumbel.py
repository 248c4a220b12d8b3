"""The Gumbel-softmax quantizer on the GPU (gumbel_rows_fwd_kernel / gumbel_rows_bwd_kernel of csrc/entropy.hip, GumbelVQFn in
_ops_vq.py, GumbelVectorQuantizer) against the float64 reference of tests/entropy_reference.py; cases, shared references and bounds are
in tests/entropy_cases.py.

(d) the row kernels through the C ABI, fp32 and bf16 y / dy, soft and hard, with and without the device schedule tensor
    ``sched = [tau, kl_cost]``.  With a schedule tensor the host arguments carry 2 tau and another kl_cost: the reference uses the
    tensor's values, and sched[1] / n for the KL coefficient.  Two exact ties are planted: columns 0 and 64 of row 0 (the same lane
    meets both, in two trips) and columns 3 and 40 of row 1 (two lanes); the lower index must win.  One case has a row whose noise
    spans 1e-30 .. 1e4.  The backward runs with dy alone, dy and the KL cotangent, and the KL cotangent ALONE (dy = 0: the KL term
    is 1 / N of the other and would vanish beside it).
(e) GumbelVQFn and GumbelVectorQuantizer against ``gumbel_vq``: q, idx on every row, kl, hist, dlogits, dE; fp32 and bf16, soft and
    hard, with and without a schedule tensor; the backward with the KL cotangent absent must use the forward's temperature; the module
    in train() with straight_through, after ``set_consts``, and ``vec_to_codes`` with injected noise.

Tokens must match on every row (the maker redraws a noise row until the float64 margin between the best and the second-best
t = (logit - log noise) / tau is 1e-4 max(1, max|t|)).  Real-valued fp32 results are compared in max|got - want| / max|want| against
max(16 e32, floor) (tests/entropy_cases.py; tests/test_entropy_cpu.py holds every such bound to <= 1e-3); a bf16 y with bf16(float32
evaluation) within one bf16 ulp of the value; the other results of a bf16 model as ``compare_fn`` says.  Every figure is printed
(``GUMMEASURE``) before it is asserted.

Invariant held beyond the values: the backward recomputes y at the temperature the forward used -- sched[0] whenever a schedule tensor
was given, whether the KL output has a cotangent (autograd always supplies one, zeros if need be) or none at all (``dkl=None``) -- and
the KL term is zero without a KL cotangent.

Measured on an MI355X, largest e32 / largest device distance over the cases.  (d) y 7.6e-6 / 4.7e-6 (N = 2051, K = 32, tau = 0.05), the
bf16 y at most 1.00 ulp from bf16(float32 evaluation) (and 2^-126 where the float32 value is subnormal: the device's exp flushes),
klsum 5.5e-7 / 1.1e-6, dlogits 2.3e-5 / 5.7e-6 (N = 515, K = 1000, tau = 0.05); K = 1: klsum = 0 against 1.6e-9 (vacuous relative
bound).  (e) fp32: q 1.2e-6 / 6.2e-7, dE 7.7e-7 / 3.9e-7, kl 3.8e-7 / 2.9e-7, dlogits inside (d)'s figures.  bf16: the stored y is at
most 1.00 ulp from the reference's; hard y equals it, soft y differs by one ulp somewhere at all three shapes, dy at the two larger
ones.  Where the operands are equal: q = bf16(reference q) exactly, dE and dlogits within the fp32 bound (dlogits 4.5e-7 against
1.3e-5); elsewhere q at most 2.8e-3 (format bound 1.6e-2), dE 7.5e-6, dlogits 1.2e-6.  Every case is inside its bound; the closest is
y at N = 3, K = 5, tau = 0.05: 1.4e-6 against 8.3e-6.  Before ``GumbelVQFn.backward`` passed the schedule tensor unconditionally, the
``dkl=None`` call was at a distance of 0.59 (N = 67, K = 64) and 0.72 (N = 515, K = 128) where autograd's path is at 4.6e-7 and 7.2e-7.

Not tested, on purpose: a row whose perturbed logits are all -inf or NaN (noise inf or 0) leaves gumbel_rows_fwd_kernel's argmax at
its initial 0x7fffffff, which then indexes the histogram -- a host-side guard is still to be written."""
import importlib

import numpy as np
import pytest
import torch

from tests import entropy_cases as C
from tests import entropy_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
vqm = importlib.import_module(PKG + '.modules.vector_quantizers')
DEV = 'cuda:0'
TDT = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def t32(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float32, device=DEV)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def check(name, case, got, want64, want32, floor=1e-6, extra=''):
    e32, dist = R.distance(want32, want64), R.distance(got, want64)
    b = C.bound(e32, floor)
    print(f'GUMMEASURE {name} {case} {extra} e32 {e32:.3e} device {dist:.3e} bound {b:.3e}')
    assert dist <= b, (name, case, extra, dist, b)
    if b >= 1.0:
        # the bound says nothing (K = 1: kl = log(1 + 1e-10), 1e-10 in float64 and 0 in float32): the device's value must be as small
        small = 16.0 * max(np.abs(np.asarray(want64, dtype=np.float64)).max(), np.abs(np.asarray(want32, dtype=np.float64)).max())
        got_max = float(np.abs(np.asarray(got, dtype=np.float64)).max())
        print(f'GUMMEASURE {name} {case} {extra} vacuous relative bound: max|device| {got_max:.3e} against {small:.3e}')
        assert got_max <= small, (name, case, got_max, small)


def check_bf16(name, case, got, want32, extra=''):
    """a bf16 result against bf16(float32 evaluation): within one bf16 ulp of the value, elementwise.  Below the smallest normal
    (2^-126) the device's exp flushes to zero where numpy keeps a subnormal: there the allowance is 2^-126 itself."""
    want = R.bf16(want32)
    sub = np.abs(np.asarray(want32, dtype=np.float64)) < 2.0 ** -126          # (a float32 subnormal may still round UP to bf16's 2^-126)
    ulps = float((np.abs(got - want) / np.where(sub, 2.0 ** -126, R.bf16_ulp(want))).max())
    print(f'GUMMEASURE {name} {case} {extra} bf16: max |device - bf16(f32)| {ulps:.2f} ulp, bound 1')
    assert ulps <= 1.0, (name, case, extra, ulps)


# ----------------------------------------------------------------------------------------------------------------------------------
# (d)
# ----------------------------------------------------------------------------------------------------------------------------------
def run_forward(ref, n, k, tau, dt, hard, sched):
    lib, st = native.lib(), ops._stream()
    logits, noise = t32(ref['inp']['logits']), t32(ref['inp']['noise'])
    y = torch.empty((n, k), dtype=TDT[dt], device=DEV)
    idx = torch.empty(n, dtype=torch.int64, device=DEV)
    klsum, hist = torch.zeros(1, dtype=torch.float32, device=DEV), torch.zeros(k, dtype=torch.int32, device=DEV)
    sc = t32([tau, C.KL_SCHED]) if sched else None
    native.check(lib.vqk_gumbel_forward(ops.dcode(TDT[dt]), logits.data_ptr(), noise.data_ptr(), n, k, 2.0 * tau if sched else tau, int(hard),
                                        y.data_ptr(), idx.data_ptr(), klsum.data_ptr(), hist.data_ptr(), ops._p(sc), st), 'gumbel_forward')
    torch.cuda.synchronize()
    return y, idx, klsum, hist


@pytest.mark.parametrize('tau', C.GUM_TAUS, ids=lambda t: f'tau{t}')
@pytest.mark.parametrize('shape', C.GUM_SHAPES, ids=C.gum_id)
def test_row_forward(shape, tau):
    n, k = shape
    ref = C.gumbel_reference(shape, tau)
    f64, f32 = ref['f64'], ref['f32']
    for r, (a, b) in enumerate(ref['inp']['ties']):
        assert f64['idx'][r] == a and ref['inp']['logits'][r, a] == ref['inp']['logits'][r, b]
    one_hot = np.zeros((n, k))
    one_hot[np.arange(n), f64['idx']] = 1
    for dt in ('fp32', 'bf16'):
        for hard in (0, 1):
            for sched in (False, True):
                case, extra = f'{C.gum_id(shape)}-tau{tau}', f'{dt} hard={hard} sched={int(sched)}'
                y, idx, klsum, hist = run_forward(ref, n, k, tau, dt, hard, sched)
                np.testing.assert_array_equal(idx.cpu().numpy(), f64['idx'])                # every row
                np.testing.assert_array_equal(hist.cpu().numpy(), f64['hist'])
                check('klsum', case, host(klsum)[0], f64['klsum'], f32['klsum'], ref['floor']['klsum'], extra)
                if hard:
                    np.testing.assert_array_equal(host(y), one_hot)
                elif dt == 'fp32':
                    check('y', case, host(y), f64['y'], f32['y'], extra=extra)
                else:
                    check_bf16('y', case, host(y), f32['y'], extra)


@pytest.mark.parametrize('tau', C.GUM_TAUS, ids=lambda t: f'tau{t}')
@pytest.mark.parametrize('shape', C.GUM_SHAPES, ids=C.gum_id)
def test_row_backward(shape, tau):
    n, k = shape
    ref = C.gumbel_reference(shape, tau)
    lib, st = native.lib(), ops._stream()
    logits, noise = t32(ref['inp']['logits']), t32(ref['inp']['noise'])
    for setting, (use_dy, gs, sched) in C.GUM_SETTINGS.items():
        for dt in ('fp32', 'bf16'):
            dyn = dt if use_dy else 'zero'
            dy = t32(ref['dy'][dyn]).to(TDT[dt])
            g = t32([gs]) if gs is not None else None
            sc = t32([tau, C.KL_SCHED]) if sched else None
            dl = torch.empty((n, k), dtype=torch.float32, device=DEV)
            native.check(lib.vqk_gumbel_backward(ops.dcode(TDT[dt]), logits.data_ptr(), noise.data_ptr(), dy.data_ptr(), n, k,
                                                 2.0 * tau if sched else tau, 0.0 if setting == 'dy' else C.KL_HOST, ops._p(g), dl.data_ptr(),
                                                 ops._p(sc), st), 'gumbel_backward')
            torch.cuda.synchronize()
            key = f'dl|{setting}|{dyn}'
            if not np.any(ref['f64'][key]):
                assert not host(dl).any(), (setting, dt)                # one column: the gradient of a constant
                continue
            check('dlogits', f'{C.gum_id(shape)}-tau{tau}', host(dl), ref['f64'][key], ref['f32'][key], extra=f'{setting} {dt}')


# ----------------------------------------------------------------------------------------------------------------------------------
# (e)
# ----------------------------------------------------------------------------------------------------------------------------------
FN_SHAPES, FN_TAU, FN_KL, fn_id, fn_inputs, fn_reference, kl_floor_of = (C.FN_SHAPES, C.FN_TAU, C.FN_KL, C.fn_id, C.fn_inputs, C.fn_reference,
                                                                         C.fn_kl_floor)


def format_bound(name, case, extra, got, want, a, b, factor, why):
    """the fallback of a bf16 model's result when the device's bf16 y (or dy) is NOT the reference's rounding everywhere: each may be
    one bf16 ulp off (<= 2^-7 of the value) and a bf16 output one more; carried through the product that forms the result this is at
    most ``factor`` 2^-7 max(|A| |B|) -- a bound from the number format alone, in ``distance``"""
    tol = factor * 2.0 ** -7 * float((np.abs(a) @ np.abs(b)).max()) / max(float(np.abs(want).max()), 1e-300)
    dist = R.distance(got, want)
    print(f'GUMMEASURE {name} {case} {extra} bf16: device {dist:.3e} bound {tol:.3e} ({why})')
    assert dist <= tol, (name, case, extra, dist, tol)


def device_dy(shape):
    """dy = dq E^T of a bf16 model as GumbelVQFn.backward forms it (the same 1x1 GEMM on the same operands): [N, K], bf16 values"""
    n, k, dim = shape
    inp = fn_inputs(shape)
    dq = t32(inp['dq']).view(1, n, 1, dim).permute(0, 3, 1, 2).to(torch.bfloat16)
    e_w = ops.pack_weights(t32(inp['E']).reshape(-1), torch.bfloat16, k, dim, 1, False, 0)
    dy = ops.raw_conv_fprop(dq, e_w, None, None, 1, False, 0, torch.bfloat16, k, 0)
    torch.cuda.synchronize()
    return host(dy.permute(0, 2, 3, 1).reshape(n, k))


def run_fn(shape, dt, hard, sched, cot_q, cot_kl):
    """one forward and backward of GumbelVQFn on the [1, K, N, 1] map whose pixels are the rows; with a schedule tensor the host
    scalars are 2 tau and 3 kl_cost, to be ignored in both directions.  ``node`` is the backward node (the ctx); ``keep`` holds the
    outputs, without which the node's saved tensors are released."""
    n, k, dim = shape
    inp = fn_inputs(shape)
    rows = lambda a, c: t32(a).view(1, n, 1, c).permute(0, 3, 1, 2)
    logits, e = rows(inp['logits'], k).requires_grad_(True), t32(inp['E']).requires_grad_(True)
    sc = t32([FN_TAU, FN_KL]) if sched else None
    q, idx, kl, hist = ops.GumbelVQFn.apply(logits, e, rows(inp['noise'], k), 2.0 * FN_TAU if sched else FN_TAU,
                                            3.0 * FN_KL if sched else FN_KL, bool(hard), TDT[dt], sc)
    outs = [o for o, c in ((q, cot_q), (kl, cot_kl)) if c]
    cots = [c for c in (rows(inp['dq'], dim).to(TDT[dt]) if cot_q else None, t32(C.GLOSS) if cot_kl else None) if c is not None]
    dl, de = torch.autograd.grad(outs, [logits, e], cots, retain_graph=True)
    torch.cuda.synchronize()
    return dict(q=host(q.permute(0, 2, 3, 1).reshape(n, dim)), idx=idx.reshape(-1).cpu().numpy(), kl=float(kl.detach()), hist=hist.cpu().numpy(),
                dlogits=host(dl.permute(0, 2, 3, 1).reshape(n, k)), dE=host(de), node=q.grad_fn, keep=(q, kl), cot_q=cots[0] if cot_q else None,
                y=host(q.grad_fn.saved_tensors[3].permute(0, 2, 3, 1).reshape(n, k)),
                q_dtype=q.dtype, idx_shape=tuple(idx.shape))


def compare_fn(shape, dt, hard, got, w64, w32, extra):
    """fp32: every real result within max(16 e32, floor).  bf16: the stored y within one bf16 ulp of the reference's rounding (the
    issue's rule for a bf16 output).  Where it IS that rounding everywhere, dE = y^T dq has the reference's operands and takes the
    fp32 bound, and q must be bf16(reference q) within one bf16 ulp of the value plus the rounding of the fp32 accumulation (16 * 2^-24
    |y| |E|); the same for dlogits where the device's dy = dq E^T is the reference's rounding.  Otherwise ``format_bound``."""
    case = fn_id(shape)
    np.testing.assert_array_equal(got['idx'], w64['idx'])                                   # every row
    np.testing.assert_array_equal(got['hist'], w64['hist'])
    check('kl', case, got['kl'], w64['kl'], w32['kl'], C.fn_kl_floor(shape), extra)
    if dt == 'fp32':
        for key in ('q', 'dE', 'dlogits'):
            check(key, case, got[key], w64[key], w32[key], extra=extra)
        return
    inp = fn_inputs(shape)
    e_abs, dq_abs = np.abs(inp['E']), np.abs(inp['dq'])
    if 'y' in got:                                                      # (the module test has no node to read y from)
        if hard:
            np.testing.assert_array_equal(got['y'], w64['y'])
        else:
            check_bf16('y-stored', case, got['y'], w32['y'], extra)
    y_same = 'y' in got and np.array_equal(got['y'], w64['y'])
    dy_dev = device_dy(shape)
    dy_same = np.array_equal(dy_dev, w64['dy'])
    ulps = float((np.abs(dy_dev - w64['dy']) / R.bf16_ulp(w64['dy'])).max())
    print(f'GUMMEASURE operands {case} {extra} bf16: y is the reference rounding: {y_same}; dy: {dy_same} (max {ulps:.2f} ulp)')
    assert ulps <= 1.0
    if y_same:
        want = R.bf16(w64['q'])
        excess = float(((np.abs(got['q'] - want) - 16.0 * 2.0 ** -24 * (w64['y'] @ e_abs)) / R.bf16_ulp(want)).max())
        print(f'GUMMEASURE q {case} {extra} bf16: max (|device - bf16(f64)| - accumulation allowance) {excess:.2f} ulp, bound 1')
        assert excess <= 1.0, ('q', case, extra, excess)
        check('dE', case, got['dE'], w64['dE'], w32['dE'], extra=extra + ' bf16')
    else:
        format_bound('q', case, extra, got['q'], w64['q'], w64['y'], e_abs, 2.0, 'y one ulp off somewhere')
        format_bound('dE', case, extra, got['dE'], w64['dE'], w64['y'].T, dq_abs, 1.0, 'y one ulp off somewhere')
    if dy_same:
        check('dlogits', case, got['dlogits'], w64['dlogits'], w32['dlogits'], extra=extra + ' bf16')
    else:
        # dlogits = y (dy - sum y dy) / tau + KL part: |y| (|dy| + sum |y| |dy|) / tau carries dy's ulp
        _, ysoft, _ = R._softmax_parts(R.gumbel_t(inp['logits'], inp['noise'], FN_TAU))
        amp = ysoft * (np.abs(w64['dy']) + (ysoft * np.abs(w64['dy'])).sum(-1, keepdims=True)) / FN_TAU
        format_bound('dlogits', case, extra, got['dlogits'], w64['dlogits'], amp.max(-1, keepdims=True), np.ones((1, 1)), 1.0,
                     'dy one ulp off somewhere')


@pytest.mark.parametrize('sched', [False, True], ids=['host-scalars', 'sched'])
@pytest.mark.parametrize('hard', [False, True], ids=['soft', 'hard'])
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', FN_SHAPES, ids=fn_id)
def test_gumbel_vq_function(shape, dt, hard, sched):
    w64, w32 = fn_reference(shape, dt, hard, C.GLOSS)
    got = run_fn(shape, dt, hard, sched, True, True)
    assert got['q_dtype'] == TDT[dt] and got['idx_shape'] == (1, shape[0], 1)
    compare_fn(shape, dt, hard, got, w64, w32, f'{dt} hard={int(hard)} sched={int(sched)} dq+kl')


@pytest.mark.parametrize('sched', [False, True], ids=['host-scalars', 'sched'])
@pytest.mark.parametrize('shape', FN_SHAPES[:2], ids=fn_id)
def test_backward_without_a_kl_cotangent_uses_the_forward_temperature(shape, sched):
    """dq alone: through autograd (which hands the kernel a ZERO cotangent for kl) and with the cotangent truly absent (None).  Either
    way y must be recomputed at the temperature the forward used -- sched[0] when a schedule tensor was given, not the host scalar --
    and the KL term must be zero."""
    w64, w32 = fn_reference(shape, 'fp32', False, None)
    got = run_fn(shape, 'fp32', False, sched, True, False)
    case = fn_id(shape)
    check('dlogits', case, got['dlogits'], w64['dlogits'], w32['dlogits'], extra=f'sched={int(sched)} dq alone, autograd')
    check('dE', case, got['dE'], w64['dE'], w32['dE'], extra=f'sched={int(sched)} dq alone, autograd')
    dl = ops.GumbelVQFn.backward(got['node'], got['cot_q'], None, None, None)[0]
    torch.cuda.synchronize()
    check('dlogits', case, host(dl.permute(0, 2, 3, 1).reshape(shape[0], shape[1])), w64['dlogits'], w32['dlogits'],
          extra=f'sched={int(sched)} dq alone, dkl=None')
    # and the KL cotangent alone, dq absent
    w64, w32 = fn_reference(shape, 'fp32', False, C.GLOSS, use_dq=False)
    got = run_fn(shape, 'fp32', False, sched, False, True)
    check('dlogits', case, got['dlogits'], w64['dlogits'], w32['dlogits'], extra=f'sched={int(sched)} kl alone')
    assert not got['dE'].any()


def _module(shape, noise_rows=None):
    n, k, dim = shape
    inp = fn_inputs(shape)
    m = vqm.GumbelVectorQuantizer(k, dim, True, 2.0 * FN_TAU, 3.0 * FN_KL).to(DEV)
    with torch.no_grad():
        m.codebook.weight.copy_(t32(inp['E']))
        m.x_to_logits.weight.copy_(torch.eye(k, device=DEV).view(k, k, 1, 1))          # logits = x, exactly
        m.x_to_logits.bias.zero_()
    return m, inp


def test_module_in_training_follows_set_consts_through_the_schedule_tensor():
    shape = FN_SHAPES[0]
    n, k, dim = shape
    m, inp = _module(shape)
    m.train()
    sc = m.enable_device_schedule(DEV)
    m.set_consts(temp=FN_TAU, kl_cost=FN_KL)                           # after the tensor exists: it must follow
    np.testing.assert_array_equal(sc.cpu().numpy(), np.array([FN_TAU, FN_KL], dtype=np.float32))
    rows = lambda a, c: t32(a).view(1, n, 1, c).permute(0, 3, 1, 2)
    x = rows(inp['logits'], k).requires_grad_(True)
    q, idx, kl = m(x, exp_noise=rows(inp['noise'], k))
    dx, de = torch.autograd.grad([q, kl], [x, m.codebook.weight], [rows(inp['dq'], dim), t32(C.GLOSS)])
    torch.cuda.synchronize()
    w64, w32 = fn_reference(shape, 'fp32', True, C.GLOSS)              # train() with straight_through: hard
    got = dict(q=host(q.permute(0, 2, 3, 1).reshape(n, dim)), idx=idx.reshape(-1).cpu().numpy(), kl=float(kl.detach()),
               hist=m.last_hist.cpu().numpy(),
               dlogits=host(dx.permute(0, 2, 3, 1).reshape(n, k)), dE=host(de))
    assert tuple(idx.shape) == (1, n, 1)
    compare_fn(shape, 'fp32', True, got, w64, w32, 'module train() straight_through after set_consts')


def test_vec_to_codes_returns_the_reference_tokens_for_injected_noise(monkeypatch):
    shape = FN_SHAPES[1]
    n, k, dim = shape
    m, _ = _module(shape)
    m.eval()
    inp = R.make_gumbel_inputs(7100, n, k, 1.0, ties=[(3, 40)])        # vec_to_codes samples x itself at tau = 1
    assert inp['rounds'] < R.ROUNDS
    rows = lambda a, c: t32(a).view(1, n, 1, c).permute(0, 3, 1, 2)
    noise = rows(inp['noise'], k)
    monkeypatch.setattr(torch.Tensor, 'exponential_', lambda self, *a, **kw: self.copy_(noise))
    idx = m.vec_to_codes(rows(inp['logits'], k))
    monkeypatch.undo()
    np.testing.assert_array_equal(idx.reshape(-1).cpu().numpy(), R.gumbel_rows(inp['logits'], inp['noise'], 1.0, True)[1])
