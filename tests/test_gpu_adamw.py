"""The AdamW arena kernel (csrc/optim.hip: adamw_kernel behind vqk_adamw / vqk_adamw_guarded) and FlatAdamW.step against float64.

Teacher-forced tests take ONE step from a given state and ask every element of p, v and m to lie within the rounding bound of
tests/adamw_reference.py (an operation count, reachable by a plain float32 evaluation: tests/test_adamw_cpu.py) of the float64
step taken from the device's own pre-step state; tests/test_adamw_cpu.py shows that a decay taken from the neighbouring
segment, a step count off by one, a dropped gradient scale and a wrong moment each leave 10 x that bound on these cases.  Every
buffer lies between 64 guard elements on both sides; the shadow must have the bits of p.to(bfloat16), the gradient and the guards
must be untouched, padding segments must keep their bits.  Free-running tests (20 kernel steps, FlatAdamW against
torch.optim.AdamW on CPU float64) take their tolerance from the distance a float32 evaluation in the kernel's operation order
(step32, numpy) keeps from float64 on the same inputs, x 4.  Writing a NaN / Inf into a gradient is data; nothing here provokes
a device fault.

Measured on an MI355X (ADAMWMEASURE lines; worst error / bound over the parametrised cases of a test, p / v / m):
  segment tables x alignments x moment forms   0.321 / 0.347 / 0.461        lengths as a single segment   0.268 / 0.386 / 0.455
  step counts 1 .. 100000                      0.292 / 0.402 / 0.448        gradient scales               0.299 / 0.394 / 0.379
  magnitudes 1e-12 .. 1e12 and g = v = 0       0.358 / 0.427 / 0.469        containment (other elements)  0.290 / 0.373 / 0.465
  guarded kernel                               0.341 / 0.323 / 0.424 (and bit-equal to vqk_adamw in all 22 cases)
  real table (2 567 296 elements, 176 segments, groups of 52 and 92 tensors, 1069 padding elements)   0.293 / 0.324 / 0.424
  (the plain float32 numpy evaluation reaches 0.60 / 0.44 / 0.47 on the same cases: the kernel's fused multiply-adds round less)
  20 free-running steps, max |dp| / (|p| + lr) and max rel dv: betas (0, 0.99)     float32 numpy 6.93e-7 / 4.68e-7, kernel 5.54e-7 / 2.89e-7
                                                               betas (0.9, 0.999)  float32 numpy 1.71e-6 / 4.19e-7, kernel 1.09e-6 / 2.78e-7
  FlatAdamW against torch.optim.AdamW, dp / dv / dm after 10 and 13 steps (the same with and without arena_front / arena_back):
    betas (0, 0.99)     float32 numpy 4.66e-7 / 2.75e-7 / - and 6.71e-7 / 3.37e-7 / -,   FlatAdamW 3.17e-7 / 2.20e-7 / - and 3.67e-7 / 2.26e-7 / -
    betas (0.9, 0.999)  float32 numpy 4.72e-7 / 2.86e-7 / 1.06e-7 and 5.49e-7 / 3.45e-7 / 9.89e-8,
                        FlatAdamW 3.54e-7 / 2.20e-7 / 7.96e-8 and 4.20e-7 / 2.32e-7 / 9.80e-8; after the states changed sides at step 10:
                        torch from FlatAdamW's state 3.50e-7 / 1.67e-7 / 6.97e-8, FlatAdamW from torch's state 4.20e-7 / 1.62e-7 / 7.44e-8
"""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import adamw_reference as A

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
optim = importlib.import_module(PKG + '.optim')
native = importlib.import_module(PKG + '._native')
DEV = 'cuda:0'
GUARD = 64
PATTERN = 0x5A5A5A5A                                                   # every guard element, as bits (float32: 1.5e16)
FLOATS = ('p', 'g', 'v', 'm')
ALIGNS = ('aligned', 'p+1', 'g+1', 'v+1', 'm+1', 'shadow+1', 'noshadow')


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Arena:
    """p / g / v / m / shadow of one launch, each between two guards; ``align`` 'x+1': buffer x starts one element behind a
    16-byte boundary (vec_ok = 0; the shadow is then 2-byte aligned only), 'noshadow': no shadow"""

    def __init__(self, case, align='aligned', x=None):
        x = case.inputs() if x is None else x
        self.case, self.n = case, case.n
        self.raw, self.view = {}, {}
        for name in FLOATS + ('shadow',):
            if (name == 'm' and not case.store_m) or (name == 'shadow' and align == 'noshadow'):
                self.view[name] = None
                continue
            dtype = torch.bfloat16 if name == 'shadow' else torch.float32
            raw = torch.empty(self.n + 2 * GUARD + 8, dtype=dtype, device=DEV)
            _bits_inplace(raw).fill_(PATTERN & 0xFFFF if name == 'shadow' else PATTERN)
            start = GUARD + (1 if align == name + '+1' else 0)
            assert raw.data_ptr() % 16 == 0
            view = raw[start:start + self.n]
            src = x['p'] if name == 'shadow' else x[name]
            view.copy_(torch.as_tensor(src).to(dtype))
            self.raw[name], self.view[name] = (raw, start), view
        self.seg_end = torch.tensor(case.ends, dtype=torch.int64, device=DEV)
        self.seg_wd = torch.tensor(case.seg_wd, dtype=torch.float32, device=DEV)
        assert int(case.ends[-1]) == self.n and self.seg_end.numel() == self.seg_wd.numel()
        for name in FLOATS:                                            # the form the kernel will take
            if self.view[name] is not None:
                assert (self.view[name].data_ptr() % 16 == 0) == (align != name + '+1')

    def _ptr(self, name):
        return 0 if self.view[name] is None else self.view[name].data_ptr()

    def _args(self, lr):
        c = self.case
        return (self._ptr('p'), self._ptr('g'), self._ptr('m'), self._ptr('v'), self.n, self.seg_end.data_ptr(), self.seg_wd.data_ptr(),
                self.seg_end.numel(), float(lr), float(c.betas[0]), float(c.betas[1]), float(c.eps))

    def step(self, lr=None, t=None):
        c = self.case
        native.check(native.lib().vqk_adamw(*self._args(c.lr if lr is None else lr), int(c.t if t is None else t),
                                            float(c.grad_scale), self._ptr('shadow'), torch.cuda.current_stream().cuda_stream), 'adamw')

    def guarded_step(self):
        """vqk_step_guard on a hand-made statistics row (finite, no clipping: apply = 1, eff_scale = grad_scale) with the applied
        count at t - 1, then vqk_adamw_guarded"""
        c = self.case
        stream = torch.cuda.current_stream().cuda_stream
        lib = native.lib()
        row = torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64, device=DEV)
        state = torch.tensor(optim.GUARD_STATE_INIT, dtype=torch.float64, device=DEV)
        state[optim.GUARD_APPLIED] = float(c.t - 1)
        self.ctrl = torch.zeros(4, dtype=torch.int32, device=DEV)
        bias = optim.bias_table(*c.betas).to(DEV)
        native.check(lib.vqk_step_guard(row.data_ptr(), 1, 0.0, float(c.lr), float(c.grad_scale), bias.data_ptr(), bias.shape[0],
                                        state.data_ptr(), self.ctrl.data_ptr(), stream), 'step_guard')
        native.check(lib.vqk_adamw_guarded(*self._args(c.lr), self.ctrl.data_ptr(), self._ptr('shadow'), stream), 'adamw_guarded')
        torch.cuda.synchronize()
        assert self.ctrl[0].item() == 1 and state[optim.GUARD_APPLIED].item() == float(c.t)

    def set_grad(self, g):
        self.view['g'].copy_(torch.as_tensor(g, dtype=torch.float32))

    def read(self):
        """the device's state as numpy (shadow: its bits)"""
        torch.cuda.synchronize()
        out = {k: (None if self.view[k] is None else self.view[k].cpu().numpy().copy()) for k in FLOATS}
        out['shadow'] = None if self.view['shadow'] is None else _bits(self.view['shadow']).cpu().numpy().copy()
        return out

    def guards_intact(self):
        bad = []
        for name, (raw, start) in self.raw.items():
            b = _bits(raw).cpu().numpy()
            want = np.int64(PATTERN & 0xFFFF if name == 'shadow' else PATTERN).astype(b.dtype)
            if not ((b[:start] == want).all() and (b[start + self.n:] == want).all()):
                bad.append(name)
        return bad


def _bits_inplace(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return (a is None and b is None) or np.array_equal(a.view(np.int32 if a.dtype == np.float32 else a.dtype),
                                                       b.view(np.int32 if b.dtype == np.float32 else b.dtype))


def teacher_forced(case, align='aligned', x=None, poisoned=None, launch='step'):
    """one launch of ``case`` with every check of the module docstring; ``poisoned``: indices whose gradient is non-finite.
    Returns (ratios, arena)."""
    a = Arena(case, align, x)
    pre = a.read()                                                     # the device's own pre-step state
    getattr(a, launch)()
    post = a.read()
    bad = np.zeros(case.n, dtype=bool)
    if poisoned is not None:
        bad[list(poisoned)] = True
    ok, ratios = A.check(case, pre, post['p'], post['v'], post['m'], skip=bad)
    assert ok, (case.name, align, ratios)
    for k in ('p', 'v') + (('m',) if case.store_m else ()):
        assert not np.isfinite(post[k][bad]).any() and np.isfinite(post[k][~bad]).all(), (case.name, align, k)
    assert _same(post['g'], pre['g']), 'the gradient was written'
    assert a.guards_intact() == [], a.guards_intact()
    if post['shadow'] is not None:
        want = _bits(torch.as_tensor(post['p']).to(torch.bfloat16)).numpy()
        assert np.array_equal(post['shadow'][~bad], want[~bad]), 'shadow != p.to(bfloat16)'
        s = torch.as_tensor(post['shadow']).view(torch.bfloat16).float().numpy()
        assert not np.isfinite(s[bad]).any()
    pad = case.pad
    for k in ('p', 'v', 'm'):
        if post[k] is not None:
            assert _same(post[k][pad], pre[k][pad]), (case.name, align, k, 'padding changed')
    return ratios, a


def _fmt(r):
    return ' '.join(f'{k} {v:.3f}' for k, v in r.items() if v is not None)


def _worst(*rs):
    return {k: (None if all(r[k] is None for r in rs) else max(r[k] for r in rs if r[k] is not None)) for k in ('p', 'v', 'm')}


# ---------------------------------------------------------------------------------------------- 1. tables x alignment x m form
TABLE_CASES = A.table_cases()
TABLE_PARAMS = [(c, al) for c in TABLE_CASES for al in ALIGNS if c.store_m or al != 'm+1']


@pytest.mark.parametrize('case,align', TABLE_PARAMS, ids=[f'{c.name}-{al}' for c, al in TABLE_PARAMS])
def test_segment_tables_alignments_and_moment_forms(case, align):
    ratios, _ = teacher_forced(case, align)
    print(f'ADAMWMEASURE table {case.name} {align}: error / bound {_fmt(ratios)}')


# ---------------------------------------------------------------------------------------------- 2. the other axes
@pytest.mark.parametrize('align', ['aligned', 'p+1'])
@pytest.mark.parametrize('case', A.length_cases(), ids=repr)
def test_lengths_as_a_single_segment(case, align):
    ratios, _ = teacher_forced(case, align)
    print(f'ADAMWMEASURE length {case.name} {align}: error / bound {_fmt(ratios)}')


@pytest.mark.parametrize('case', A.t_cases(), ids=repr)
def test_step_counts(case):
    ratios, _ = teacher_forced(case)
    print(f'ADAMWMEASURE steps {case.name}: error / bound {_fmt(ratios)}')


@pytest.mark.parametrize('case', A.scale_cases(), ids=repr)
def test_gradient_scales(case):
    ratios, _ = teacher_forced(case)
    print(f'ADAMWMEASURE scale {case.name}: error / bound {_fmt(ratios)}')


@pytest.mark.parametrize('align', ['aligned', 'g+1'])
@pytest.mark.parametrize('case', A.magnitude_cases(), ids=repr)
def test_magnitudes(case, align):
    ratios, a = teacher_forced(case, align)
    print(f'ADAMWMEASURE magnitude {case.name} {align}: error / bound {_fmt(ratios)}')
    if case.kind == 'zero':                                            # exactly the decay, nothing else
        x = case.inputs()
        post = a.read()
        assert np.array_equal(post['p'], x['p'] * (np.float32(1.0) - np.float32(case.lr) * case.wd)) and not post['v'].any()


# ---------------------------------------------------------------------------------------------- 3. containment
@pytest.mark.parametrize('align', ['aligned', 'v+1'])
@pytest.mark.parametrize('m_form', ['b1=0,m=null', 'b1=0.9'])
@pytest.mark.parametrize('rotation', [0, 1, 2])
def test_a_nonfinite_gradient_stays_in_its_element(rotation, m_form, align):
    """NaN, +Inf and -Inf inside a vector, on a segment's last element and in the scalar tail (each value in each place over the
    three rotations): p / v / m of those three elements are non-finite, every other element meets the bound"""
    case = A.Case(f'contain-{m_form}', A.table_residues(), m_form=m_form, seed=400 + rotation)
    places = [101, int(case.ends[0]) - 1, case.n - 1]
    assert places[0] % 4 == 1 and places[0] + 8 < case.ends[0] and case.n % 4 != 0 and places[2] >= case.n - case.n % 4
    values = [math.nan, math.inf, -math.inf]
    x = case.inputs()
    for k, idx in enumerate(places):
        x['g'][idx] = values[(k + rotation) % 3]
    ratios, _ = teacher_forced(case, align, x=x, poisoned=places)
    print(f'ADAMWMEASURE containment {m_form} {align} rotation {rotation}: error / bound of the other elements {_fmt(ratios)}')


# ---------------------------------------------------------------------------------------------- 4. guarded == unguarded, bitwise
GUARDED_PARAMS = [(A.Case(f'{tn}-{mf}', A.TABLES[tn](), m_form=mf, seed=500 + i), al)
                  for i, tn in enumerate(('ones', 'many')) for mf in ('b1=0,m=null', 'b1=0.9')
                  for al in ALIGNS if al != 'noshadow' and (mf == 'b1=0.9' or al != 'm+1')]


@pytest.mark.parametrize('case,align', GUARDED_PARAMS, ids=[f'{c.name}-{al}' for c, al in GUARDED_PARAMS])
def test_guarded_kernel_is_the_unguarded_one_bit_for_bit(case, align):
    ratios, g = teacher_forced(case, align, launch='guarded_step')
    u = Arena(case, align)
    u.step()
    got, want = g.read(), u.read()
    differ = [k for k in got if not _same(got[k], want[k])]
    print(f'ADAMWMEASURE guarded {case.name} {align}: error / bound {_fmt(ratios)}; differs from vqk_adamw in {differ}')
    assert not differ


# ---------------------------------------------------------------------------------------------- 5. free-running
def _distance(p, v, ref_p, ref_v, lr):
    p, v = np.asarray(p, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return float((np.abs(p - ref_p) / (np.abs(ref_p) + lr)).max()), float((np.abs(v - ref_v) / ref_v).max())


@pytest.mark.parametrize('m_form', ['b1=0,m=null', 'b1=0.9'])
def test_twenty_free_running_steps(m_form):
    """one arena, per-step lr, a fresh gradient every step; the kernel against free-running float64, measured by the distance
    free-running float32 numpy keeps (figures in the module docstring)"""
    case = A.Case(f'run-{m_form}', A.table_residues(), m_form=m_form, t=1, seed=600)
    x = case.inputs()
    a = Arena(case, 'aligned', x)
    s32 = {k: (None if x[k] is None else x[k].copy()) for k in FLOATS}
    s64 = {k: (None if x[k] is None else x[k].astype(np.float64)) for k in FLOATS}
    rng = np.random.default_rng(601)
    for t in range(1, 21):
        lr = case.lr * (1.0 - 0.03 * t)
        g = (rng.choice([-1.0, 1.0], case.n) * 1e-3 * rng.uniform(0.5, 2.0, case.n) / case.grad_scale).astype(np.float32)
        hyper = dict(case.hyper(lr), t=t)
        a.set_grad(g)
        a.step(lr=lr, t=t)
        p, m, v = A.step32(s32['p'], g, s32['m'], s32['v'], case.wd, **hyper)
        s32.update(p=p, v=v, m=m if case.store_m else None)
        res = A.step64(s64['p'], g, s64['m'], s64['v'], case.wd, **hyper)
        s64.update(p=res['p'], v=res['v'], m=res['m'] if case.store_m else None)
    got = a.read()
    base_p, base_v = _distance(s32['p'], s32['v'], s64['p'], s64['v'], case.lr)
    got_p, got_v = _distance(got['p'], got['v'], s64['p'], s64['v'], case.lr)
    print(f'ADAMWMEASURE trajectory {m_form}: float32 numpy vs float64 max |dp| / (|p| + lr) {base_p:.3e} max rel dv {base_v:.3e}; '
          f'kernel {got_p:.3e} / {got_v:.3e} (bound: 4 x)')
    assert base_p > 0.0 and base_v > 0.0 and a.guards_intact() == []
    assert got_p <= 4.0 * base_p and got_v <= 4.0 * base_v


# ---------------------------------------------------------------------------------------------- 6. FlatAdamW vs torch.optim.AdamW
def _flat_params(seed):
    g = torch.Generator().manual_seed(seed)

    def sgn(shape):
        return (torch.randint(0, 2, shape, generator=g) * 2 - 1) * (0.5 + 1.5 * torch.rand(shape, generator=g))
    values = [sgn((64, 32, 3, 3)).contiguous(memory_format=torch.channels_last), sgn((3, 64, 3, 3)), sgn((3,)), sgn(()),
              sgn((64,)), sgn((65,))]
    assert not values[0].is_contiguous() and values[1].is_contiguous()
    return values


def _logical(ts):
    return np.concatenate([t.detach().cpu().contiguous().reshape(-1).double().numpy() for t in ts])


class _Pair:
    """the same parameters under FlatAdamW on the GPU and torch.optim.AdamW on CPU float64"""
    GROUPS = ((0, 1), (2, 3, 4, 5))                                    # conv weights decay 0.1, the rest 0
    WDS = (0.1, 0.0)

    def __init__(self, values, betas, reorder, lr0):
        self.betas = betas
        self.flat_params = [torch.nn.Parameter(v.clone().to(DEV)) for v in values]
        assert optim._is_channels_last_param(self.flat_params[0]) and not optim._is_channels_last_param(self.flat_params[1])
        fp = self.flat_params
        kw = dict(arena_front={id(fp[5]), id(fp[3])}, arena_back={id(fp[0])}) if reorder else {}
        self.flat = optim.FlatAdamW([dict(params=[fp[i] for i in idx], weight_decay=wd) for idx, wd in zip(self.GROUPS, self.WDS)],
                                    lr=lr0, betas=betas, eps=1e-8, **kw)
        self.flat.grad_scale = 0.5
        self.flat.enable_bf16_shadow()
        self.ref_params = [torch.nn.Parameter(v.detach().clone().double().contiguous()) for v in values]
        rp = self.ref_params
        self.ref = torch.optim.AdamW([dict(params=[rp[i] for i in idx], weight_decay=A.f32(wd)) for idx, wd in zip(self.GROUPS, self.WDS)],
                                     lr=A.f32(lr0), betas=(A.f32(betas[0]), A.f32(betas[1])), eps=A.f32(1e-8))
        self.order = [i for idx in self.GROUPS for i in idx]          # state_dict order

    def step(self, grads, lr):
        for grp in self.flat.param_groups:
            grp['lr'] = lr
        for grp in self.ref.param_groups:
            grp['lr'] = A.f32(lr)
        for p, q, g in zip(self.flat_params, self.ref_params, grads):
            p.grad.copy_(g.to(DEV))                                    # logical layout into the arena view
            q.grad = 0.5 * g.double()
        self.flat.step()
        self.ref.step()

    def state(self, which):
        """(p, v, m) in logical layout, parameters in construction order, float64"""
        if which == 'flat':
            sd = self.flat.state_dict()['state']
            params = self.flat_params
        else:
            sd = self.ref.state_dict()['state']
            params = self.ref_params
        pos = {i: k for k, i in enumerate(self.order)}
        return (_logical(params), _logical([sd[pos[i]]['exp_avg_sq'] for i in range(len(params))]),
                _logical([sd[pos[i]]['exp_avg'] for i in range(len(params))]))

    def check_arena(self):
        opt = self.flat
        pad = np.ones(opt.flat_p.numel(), dtype=bool)
        for p in self.flat_params:
            off = opt.offsets[id(p)]
            pad[off:off + p.numel()] = False
        assert pad.sum() == opt.flat_p.numel() - sum(p.numel() for p in self.flat_params) and pad.sum() >= 61 + 63 + 63
        for buf in (opt.flat_p, opt.flat_v, opt.flat_m, opt.flat_g):
            if buf is not None:
                assert not _bits(buf).cpu().numpy()[pad].any(), 'a padding element is no longer +0'
        assert torch.equal(_bits(opt.shadow), _bits(opt.flat_p.to(torch.bfloat16))), 'shadow != flat_p.to(bfloat16)'


def _metrics(state, ref, lr, c=1e-3):
    (p, v, m), (rp, rv, rm) = state, ref
    return (float((np.abs(p - rp) / (np.abs(rp) + lr)).max()), float((np.abs(v - rv) / rv).max()),
            float((np.abs(m - rm) / (np.abs(rm) + c)).max()))


@pytest.mark.parametrize('reorder', [False, True], ids=['plain', 'front_back'])
@pytest.mark.parametrize('betas', [(0.0, 0.99), (0.9, 0.999)], ids=['b1=0', 'b1=0.9'])
def test_flat_adamw_follows_torch_adamw(betas, reorder):
    """10 steps, then the optimizer states change sides (FlatAdamW's into a torch.optim.AdamW, torch's into a FlatAdamW) and all
    four take 3 more.  The yardstick is the free-running float32 numpy evaluation against float64 on the same gradients."""
    lr0 = 0.05
    values = _flat_params(700)
    pair = _Pair(values, betas, reorder, lr0)
    opt = pair.flat
    if reorder:                                                        # arena order != group order
        offs = [opt.offsets[id(p)] for p in pair.flat_params]
        assert offs[5] < offs[1] < offs[0] and offs[3] < offs[1] and opt.front_numel == 128 + 64 and opt.back_start == offs[0]
    else:
        assert [opt.offsets[id(pair.flat_params[i])] for i in pair.order] == sorted(opt.offsets.values())
    assert (opt.flat_m is None) == (betas[0] == 0.0) and opt.flat_p.numel() < 40000
    sizes = [v.numel() for v in values]
    wd = np.repeat(np.asarray([0.1, 0.1, 0.0, 0.0, 0.0, 0.0], dtype=np.float32), sizes)
    store_m = betas[0] != 0.0
    p0 = _logical(values).astype(np.float32)
    n = p0.size
    s32 = dict(p=p0, v=np.zeros(n, np.float32), m=np.zeros(n, np.float32) if store_m else None)
    s64 = dict(p=p0.astype(np.float64), v=np.zeros(n), m=np.zeros(n) if store_m else None)
    gen = torch.Generator().manual_seed(701)

    def one_step(t, pairs):
        lr = lr0 * (1.0 - 0.05 * t)
        grads = [((torch.randint(0, 2, v.shape, generator=gen) * 2 - 1) * 2e-3 * (0.5 + 1.5 * torch.rand(v.shape, generator=gen))).float()
                 for v in values]
        for q in pairs:
            q.step(grads, lr)
        g = _logical(grads).astype(np.float32)
        hyper = dict(lr=lr, beta1=betas[0], beta2=betas[1], eps=1e-8, t=t, grad_scale=0.5)
        p, m, v = A.step32(s32['p'], g, s32['m'], s32['v'], wd, **hyper)
        s32.update(p=p, v=v, m=m if store_m else None)
        res = A.step64(s64['p'], g, s64['m'], s64['v'], wd, **hyper)
        s64.update(p=res['p'], v=res['v'], m=res['m'] if store_m else None)

    def yardstick():
        zeros = np.zeros(n)
        return _metrics((s32['p'].astype(np.float64), s32['v'].astype(np.float64), s32['m'].astype(np.float64) if store_m else zeros),
                        (s64['p'], s64['v'], s64['m'] if store_m else zeros), lr0)

    def compare(label, flat_state, ref_state):
        base, got = yardstick(), _metrics(flat_state, ref_state, lr0)
        if not store_m:
            got = got[:2] + (math.nan,)                                # (torch keeps the gradient in exp_avg, FlatAdamW zeros)
        print(f'ADAMWMEASURE flat betas={betas} reorder={reorder} {label}: float32 numpy vs float64 dp {base[0]:.3e} dv {base[1]:.3e} '
              f'dm {base[2]:.3e}; FlatAdamW vs torch.optim.AdamW {got[0]:.3e} / {got[1]:.3e} / {got[2]:.3e} (bound: 4 x)')
        assert got[0] <= 4.0 * base[0] and got[1] <= 4.0 * base[1]
        if store_m:
            assert got[2] <= 4.0 * base[2]
        elif label.endswith('steps'):                                  # FlatAdamW's exp_avg at beta1 = 0: all zeros (torch keeps the gradient)
            assert not flat_state[2].any()

    for t in range(1, 11):
        one_step(t, [pair])
    torch.cuda.synchronize()
    # torch's own float64 run is the float64 reference of this file
    np.testing.assert_allclose(pair.state('ref')[0], s64['p'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(pair.state('ref')[1], s64['v'], rtol=1e-12, atol=0)
    compare('10 steps', pair.state('flat'), pair.state('ref'))
    pair.check_arena()
    assert opt.step_count == 10 and all(float(e['step']) == 10.0 for e in opt.state_dict()['state'].values())

    # the states change sides: a torch.optim.AdamW continues from FlatAdamW's state, a FlatAdamW from torch's
    a = _Pair([p.detach().cpu() for p in pair.flat_params], betas, reorder, lr0)       # FlatAdamW's parameters on both sides
    assert optim._is_channels_last_param(a.flat_params[0])
    sd = opt.state_dict()
    own = a.ref.state_dict()['param_groups']
    a.ref.load_state_dict({'state': sd['state'], 'param_groups': [{**o, **{k: v for k, v in g.items() if k != 'betas' and k != 'lr'}}
                                                                  for o, g in zip(own, sd['param_groups'])]})
    a.flat.load_state_dict(pair.ref.state_dict())
    assert a.flat.step_count == 10
    for t in range(11, 14):
        one_step(t, [pair, a])
    torch.cuda.synchronize()
    ref = pair.state('ref')
    compare('13 steps', pair.state('flat'), ref)
    compare('13 steps, torch from FlatAdamW state', a.state('ref'), ref)
    compare('13 steps, FlatAdamW from torch state', a.state('flat'), ref)
    pair.check_arena()
    a.check_arena()


# ---------------------------------------------------------------------------------------------- 7. the real segment table
def test_real_model_segment_table():
    """the headline architecture's tensors (two ResBlocks per level, four levels) at a quarter of its width: FlatAdamW's own
    arena order and table, decays 0.1 (conv weights) and 0.3 (everything else), one teacher-forced step at t = 7 over the whole
    arena -- a segment that took the other group's decay fails the bound on every element"""
    model_mod = importlib.import_module(PKG + '.model')
    from tests.golden import seeded
    ae = dict(seeded.AE_FULL, channels=32)
    qc = dict(num_embeddings=64, embedding_dim=16, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
    tc = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1, warmup_epochs=None, decay_epochs=None)
    torch.manual_seed(0)
    m = model_mod.VQVAE(64, ae, qc, None, tc).to(DEV).train()
    full = model_mod.VQVAE(64, seeded.AE_FULL, qc, None, tc)
    assert len(list(m.parameters())) == len(list(full.parameters()))
    del full
    first = m.configure_optimizers()                                   # the model's own layout: which tensors go first and last
    front = {id(p) for p in first._params_in_order() if first.offsets[id(p)] < first.front_numel}
    back = {id(p) for p in first._params_in_order() if first.offsets[id(p)] >= first.back_start}
    groups = [dict(params=list(g['params']), weight_decay=wd) for g, wd in zip(first.param_groups, (0.1, 0.3))]
    opt = optim.FlatAdamW(groups, lr=0.05, betas=(0.9, 0.999), eps=1e-8, arena_front=front, arena_back=back)
    assert torch.equal(opt.seg_end, first.seg_end) and front and opt.flat_p.numel() < 4_000_000
    del first
    opt.enable_bf16_shadow()
    n = opt.flat_p.numel()
    wd = np.zeros(n, dtype=np.float32)
    pad = np.ones(n, dtype=bool)
    for g, w in zip(opt.param_groups, (0.1, 0.3)):
        for p in g['params']:
            off = opt.offsets[id(p)]
            wd[off:off + p.numel()] = w
            pad[off:off + p.numel()] = False
    case = A.Case('real', dict(ends=np.array([n]), wd=np.array([0.0], np.float32), pad=np.array([False])), m_form='b1=0.9', t=7, seed=800)
    x = case.inputs()
    for k in FLOATS:
        x[k][pad] = 0.0
    for buf, k in ((opt.flat_p, 'p'), (opt.flat_g, 'g'), (opt.flat_v, 'v'), (opt.flat_m, 'm')):
        buf.copy_(torch.as_tensor(x[k]))
    opt.grad_scale = case.grad_scale
    opt.step_count = 6
    opt.step()
    torch.cuda.synchronize()
    got = {k: buf.cpu().numpy() for buf, k in ((opt.flat_p, 'p'), (opt.flat_v, 'v'), (opt.flat_m, 'm'))}
    case.wd = wd
    ok, ratios = A.check(case, x, got['p'], got['v'], got['m'])
    nseg, ngroup = opt.seg_end.numel(), [len(g['params']) for g in opt.param_groups]
    print(f'ADAMWMEASURE real table: {n} elements, {nseg} segments, groups {ngroup}, {int(pad.sum())} padding; error / bound {_fmt(ratios)}')
    assert ok, ratios
    assert opt.step_count == 7 and nseg > sum(ngroup) and min(ngroup) > 40
    for k in ('p', 'v', 'm'):
        assert not got[k][pad].view(np.int32).any()
    assert torch.equal(_bits(opt.shadow), _bits(opt.flat_p.to(torch.bfloat16)))
