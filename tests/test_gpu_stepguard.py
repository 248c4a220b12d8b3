"""The guarded optimizer step on the GPU (csrc/optim.hip: vqk_step_guard, vqk_adamw_guarded; optim.py: FlatAdamW.enable_guard).

The yardstick is the existing vqk_adamw kernel, BITWISE: an applied guarded step must leave p / m / v / shadow with the bits of
vqk_adamw(step = applied + 1, grad_scale = eff_scale), a skipped one must leave every byte alone.  Only the clip test needs a
tolerance, and takes it from the unguarded kernel's own distance to the float64 reference (tests/stepguard_reference.py) on the
same inputs, measured in the same test.  Writing a NaN / Inf into a gradient buffer is data; nothing here provokes a device fault.
"""
import importlib
import json
import math
import os
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import stepguard_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
optim = importlib.import_module(PKG + '.optim')
native = importlib.import_module(PKG + '._native')
ops = importlib.import_module(PKG + '.ops')
DEV = 'cuda:0'
LR, EPS = 2e-3, 1e-8

# (elements, weight decay, group): group -1 = alignment padding (never counted by the statistics).  Ragged segment ends, vectors
# that straddle a segment end, 14 622 elements in all: two blocks, and a tail that is not a multiple of 4
SEGMENTS = [(5, 1e-2, 0), (59, 0.0, -1), (130, 0.0, 0), (62, 0.0, -1), (1, 1e-2, 0), (1000, 0.0, 0), (259, 1e-2, 0), (4099, 1e-2, 0),
            (9000, 0.0, 0), (7, 0.0, 0)]


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.set_deterministic(False)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class Arena:
    """p / g / m / v / shadow of one optimizer plus the guard's blocks, driven through the C entry points"""

    def __init__(self, betas, shadow, offset=0, seed=0, segments=SEGMENTS):
        rng = np.random.default_rng(seed)
        self.betas = betas
        self.n = n = sum(s[0] for s in segments)
        ends = np.cumsum([s[0] for s in segments])
        self.group = np.repeat([s[2] for s in segments], [s[0] for s in segments])
        self.wd = np.repeat([s[1] for s in segments], [s[0] for s in segments])

        def buf(values, dtype=torch.float32):                        # offset 1: 4-byte aligned only, the kernels' scalar path
            t = torch.zeros(n + 8, dtype=dtype, device=DEV)
            v = t[offset:offset + n]
            v.copy_(torch.as_tensor(values, dtype=dtype))
            return v
        self.p = buf(rng.standard_normal(n))
        self.g = buf(np.zeros(n))
        self.v = buf(np.zeros(n))
        self.m = buf(np.zeros(n)) if betas[0] != 0.0 else None
        self.shadow = buf(self.p.cpu().float().numpy(), torch.bfloat16) if shadow else None
        self.seg_end = torch.tensor(ends, dtype=torch.int64, device=DEV)
        self.seg_wd = torch.tensor([s[1] for s in segments], dtype=torch.float32, device=DEV)
        self.seg_group = torch.tensor([s[2] for s in segments], dtype=torch.int32, device=DEV)
        self.ws = torch.empty(ops.arena_stats_ws_doubles(n, 1), dtype=torch.float64, device=DEV)
        self.out = torch.zeros(6, dtype=torch.float64, device=DEV)
        self.state = torch.tensor(optim.GUARD_STATE_INIT, dtype=torch.float64, device=DEV)
        self.ctrl = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.bias = optim.bias_table(*betas).to(DEV)

    def set_grad(self, g):
        self.g.copy_(torch.as_tensor(g, dtype=torch.float32))

    def _ptr(self, t):
        return 0 if t is None else t.data_ptr()

    def guarded(self, skip=True, max_norm=None, lr=LR, scale=1.0):
        """arena_stats -> step_guard -> adamw_guarded on the current stream"""
        stream = torch.cuda.current_stream().cuda_stream
        lib = native.lib()
        ops.arena_stats(self.g, self.seg_end, self.seg_group, 1, scale, self.ws, self.out)
        native.check(lib.vqk_step_guard(self.out[3:6].data_ptr(), int(skip), 0.0 if max_norm is None else max_norm, lr, scale,
                                        self.bias.data_ptr(), self.bias.shape[0], self.state.data_ptr(), self.ctrl.data_ptr(), stream),
                     'step_guard')
        native.check(lib.vqk_adamw_guarded(self.p.data_ptr(), self.g.data_ptr(), self._ptr(self.m), self.v.data_ptr(), self.n,
                                           self.seg_end.data_ptr(), self.seg_wd.data_ptr(), self.seg_end.numel(), lr, self.betas[0],
                                           self.betas[1], EPS, self.ctrl.data_ptr(), self._ptr(self.shadow), stream), 'adamw_guarded')

    def unguarded(self, step, lr=LR, scale=1.0):
        native.check(native.lib().vqk_adamw(self.p.data_ptr(), self.g.data_ptr(), self._ptr(self.m), self.v.data_ptr(), self.n,
                                            self.seg_end.data_ptr(), self.seg_wd.data_ptr(), self.seg_end.numel(), lr, self.betas[0],
                                            self.betas[1], EPS, step, float(scale), self._ptr(self.shadow),
                                            torch.cuda.current_stream().cuda_stream), 'adamw')

    def tensors(self):
        return {k: t for k, t in (('p', self.p), ('v', self.v), ('m', self.m), ('shadow', self.shadow)) if t is not None}

    def copies(self):
        return {k: t.clone() for k, t in self.tensors().items()}

    def differs_from(self, other):
        mine, theirs = self.tensors(), other if isinstance(other, dict) else other.tensors()
        return [k for k in mine if not _same_bits(mine[k], theirs[k])]

    def eff_scale(self):
        return float(self.ctrl[1:2].view(torch.float32).item())

    def state_list(self):
        return self.state.tolist()


def _grad(rng, n, scale=1.0):
    return (rng.standard_normal(n) * scale * 10.0 ** rng.uniform(-3, 0, n)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1. applied steps, coef = 1
@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('shadow', [False, True], ids=['noshadow', 'shadow'])
@pytest.mark.parametrize('betas', [(0.0, 0.99), (0.9, 0.999)], ids=['b1=0', 'b1=0.9'])
def test_applied_steps_are_vqk_adamw_bit_for_bit(betas, shadow, offset):
    """32 consecutive steps on one arena, compared after every step"""
    a, b = Arena(betas, shadow, offset, seed=1), Arena(betas, shadow, offset, seed=1)
    assert not a.differs_from(b)
    rng = np.random.default_rng(2)
    for t in range(1, 33):
        g = _grad(rng, a.n)
        a.set_grad(g)
        b.set_grad(g)
        lr = LR * (1.0 - 0.01 * t)                                    # a schedule: lr is a host scalar of every launch
        a.guarded(skip=True, max_norm=None, lr=lr, scale=0.5)
        b.unguarded(t, lr=lr, scale=0.5)
        assert not a.differs_from(b), (t, a.differs_from(b))
        assert a.ctrl[0].item() == 1 and a.eff_scale() == 0.5
    st = a.state_list()
    assert st[:5] == [32.0, 0.0, 0.0, 0.0, 0.0] and st[5] == 32.0 and st[6] == 1.0 and st[7] > 0.0
    assert torch.isfinite(a.p).all() and (a.v[torch.as_tensor(a.group >= 0, device=DEV)] > 0).all()


@pytest.mark.parametrize('t', [1000, 3725, 40000, 100000])
@pytest.mark.parametrize('betas', [(0.0, 0.99), (0.9, 0.999)], ids=['b1=0', 'b1=0.9'])
def test_single_steps_at_large_t(betas, t):
    """the applied count loaded into the state block: inside the bias-correction table, at its end (0.99^t leaves 1 - 0.99^t == 1
    from t = 3725 on) and far behind it"""
    a, b = Arena(betas, True, seed=3), Arena(betas, True, seed=3)
    rng = np.random.default_rng(4)
    for x in (a, b):
        x.v.copy_(torch.as_tensor(np.random.default_rng(5).uniform(0, 1e-2, x.n), dtype=torch.float32))
        if x.m is not None:
            x.m.copy_(torch.as_tensor(np.random.default_rng(6).standard_normal(x.n) * 1e-2, dtype=torch.float32))
    g = _grad(rng, a.n)
    a.set_grad(g)
    b.set_grad(g)
    a.state[optim.GUARD_APPLIED] = float(t - 1)
    a.guarded()
    b.unguarded(t)
    print(f'STEPGUARDMEASURE t={t} betas={betas}: table {a.bias.shape[0]} entries, step_size {a.ctrl[2:3].view(torch.float32).item()!r} '
          f'inv_sqrt_bc2 {a.ctrl[3:4].view(torch.float32).item()!r}')
    assert not a.differs_from(b) and a.state_list()[0] == float(t)


# ---------------------------------------------------------------------------------------------- 2. bias correction follows the applied count
@pytest.mark.parametrize('betas', [(0.0, 0.99), (0.9, 0.999)], ids=['b1=0', 'b1=0.9'])
def test_after_skips_the_applied_steps_are_steps_1_2_3(betas):
    pattern = [1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1]
    a, b = Arena(betas, True, seed=7), Arena(betas, True, seed=7)
    rng = np.random.default_rng(8)
    applied = 0
    for i, ok in enumerate(pattern):
        g = _grad(rng, a.n)
        if not ok:
            g[(977 * i) % 5] = math.nan                              # inside the first parameter segment
        a.set_grad(g)
        a.guarded(skip=True)
        if ok:
            applied += 1
            b.set_grad(g)
            b.unguarded(applied)
        assert not a.differs_from(b), (i, a.differs_from(b))
    st = a.state_list()
    assert st[:5] == [6.0, 6.0, 0.0, 0.0, 3.0], st


# ---------------------------------------------------------------------------------------------- 3. skip
@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
@pytest.mark.parametrize('value', [math.nan, math.inf, -math.inf], ids=['nan', '+inf', '-inf'])
def test_one_nonfinite_element_skips_the_step(value, where):
    a = Arena((0.9, 0.999), True, seed=9)
    rng = np.random.default_rng(10)
    for _ in range(2):                                                # two applied steps first: non-trivial m / v
        a.set_grad(_grad(rng, a.n))
        a.guarded()
    before = a.copies()
    idx = {'first': 0, 'middle': 5 + 59 + 130 + 62 + 1 + 1000 + 259 + 2048, 'last': a.n - 1}[where]
    assert a.group[idx] == 0
    g = _grad(rng, a.n)
    g[idx] = value
    a.set_grad(g)
    a.guarded(skip=True)
    torch.cuda.synchronize()
    assert not a.differs_from(before), a.differs_from(before)
    st = a.state_list()
    assert a.ctrl[0].item() == 0 and st[:5] == [2.0, 1.0, 0.0, 1.0, 1.0] and st[5] == 2.0 and math.isfinite(st[7]) and st[7] > 0.0
    a.guarded(skip=True)                                              # the same gradient again: the run grows
    assert not a.differs_from(before) and a.state_list()[:5] == [2.0, 2.0, 0.0, 2.0, 2.0]
    a.set_grad(_grad(rng, a.n))
    a.guarded(skip=True)                                              # a finite gradient: step 3, the run ends, its length stays
    assert a.differs_from(before) == ['p', 'v', 'm', 'shadow'] and a.state_list()[:5] == [3.0, 2.0, 0.0, 0.0, 2.0]
    # skipping off: the same poisoned gradient is applied (and the NaN goes where torch.optim.AdamW would put it)
    a.set_grad(g)
    a.guarded(skip=False)
    assert a.ctrl[0].item() == 1 and a.state_list()[:2] == [4.0, 2.0] and not math.isfinite(a.p[idx].item())


def test_poisoned_padding_does_not_skip():
    a, b = Arena((0.0, 0.99), True, seed=11), Arena((0.0, 0.99), True, seed=11)
    g = _grad(np.random.default_rng(12), a.n)
    for idx in (5, 5 + 58, 5 + 59 + 130 + 10):                        # both padding segments
        assert a.group[idx] == -1
        g[idx] = math.nan
    a.set_grad(g)
    b.set_grad(g)
    a.guarded(skip=True)
    b.unguarded(1)
    assert a.ctrl[0].item() == 1 and a.state_list()[:2] == [1.0, 0.0] and a.out[5].item() == 0.0
    assert not a.differs_from(b)


# ---------------------------------------------------------------------------------------------- 4. clip
def _ulps32(x, y):
    return abs(int(np.float32(x).view(np.int32)) - int(np.float32(y).view(np.int32)))


@pytest.mark.parametrize('betas', [(0.0, 0.99), (0.9, 0.999)], ids=['b1=0', 'b1=0.9'])
def test_clip_by_global_norm(betas):
    """eff_scale against the float64 host formula on the device's own statistics row; the update against vqk_adamw at that scale;
    the whole against the float64 reference at the distance the UNGUARDED kernel keeps from it on the same inputs (x 2: the device
    rounds its own eff_scale, from its own statistics row)"""
    steps, scale, max_norm = 12, 0.5, 0.05
    a, b, c = Arena(betas, True, seed=13), Arena(betas, True, seed=13), Arena(betas, True, seed=13)
    mask = a.group >= 0
    ref = R.GuardedAdamW(a.p.cpu().double().numpy(), a.wd, LR, betas, EPS, skip_nonfinite=True, max_norm=max_norm)
    rng = np.random.default_rng(14)
    clipped = 0
    for t in range(1, steps + 1):
        g = _grad(rng, a.n, scale=1.0 if t % 4 else 1e-4)            # every fourth step stays below max_norm
        for x in (a, b, c):
            x.set_grad(g)
        a.guarded(skip=True, max_norm=max_norm, scale=scale)
        sumsq, _, nonfinite = a.out[3:6].tolist()
        _, coef, norm = R.verdict(sumsq, nonfinite, True, max_norm)
        want = R.eff_scale(scale, coef)
        got = a.eff_scale()
        if np.float32(got) != want:
            print(f'STEPGUARDMEASURE eff_scale step {t}: device {got!r} host {float(want)!r} distance {_ulps32(got, want)} ulp (bound 1)')
        assert _ulps32(got, want) <= 1
        clipped += coef < 1.0
        assert (coef < 1.0) == (norm + 1e-6 > max_norm) == bool(t % 4)
        if coef == 1.0:
            assert got == scale                                       # norm below max_norm: exactly 1
        b.unguarded(t, scale=got)                                     # the yardstick at the device's own scale: bitwise
        assert not a.differs_from(b), (t, a.differs_from(b))
        # the float64 reference, and the unguarded kernel on the same inputs: its float32 grad_scale is the reference's product
        _, coef_ref = ref.step(g.astype(np.float64), scale, mask=mask)
        c.unguarded(t, scale=float(R.eff_scale(scale, coef_ref)))
        assert abs(coef_ref - coef) <= 1e-12
    st = a.state_list()
    assert st[:3] == [float(steps), 0.0, float(clipped)] and clipped == 9 and st[6] < 1.0 and st[5] < steps
    assert st[5] == pytest.approx(ref.coef_sum, rel=1e-12) and st[6] == pytest.approx(ref.coef_min, rel=1e-12)

    def distance(arena, reference):
        p, v = arena.p.cpu().double().numpy()[mask], arena.v.cpu().double().numpy()[mask]
        return float(np.abs(p - reference.p[mask]).max()), float((np.abs(v - reference.v[mask]) / reference.v[mask]).max())
    base_p, base_v = distance(c, ref)                                 # the unguarded kernel against the reference: the yardstick
    got_p, got_v = distance(a, ref)
    print(f'STEPGUARDMEASURE clip betas={betas}: unguarded kernel vs float64 reference max |dp| {base_p:.3e} max rel dv {base_v:.3e}; '
          f'guarded {got_p:.3e} / {got_v:.3e} (bound: 2 x unguarded)')
    assert 0.0 < base_p < 1e-4 and 0.0 < base_v < 1e-4                # (sanity of the yardstick, not the bound: a float32 kernel near float64)
    assert got_p <= 2.0 * base_p and got_v <= 2.0 * base_v


def test_norm_below_max_norm_is_exactly_one():
    a = Arena((0.0, 0.99), False, seed=15)
    g = _grad(np.random.default_rng(16), a.n)
    a.set_grad(g)
    norm = math.sqrt(R.arena_row(g.astype(np.float64), 0.25, a.group >= 0)[0])
    for k, max_norm in enumerate((norm * 2.0, norm * 1.0001, 1e30)):
        a.guarded(max_norm=max_norm, scale=0.25)
        st = a.state_list()
        assert a.eff_scale() == 0.25 and st[2] == 0.0 and st[5] == float(k + 1) and st[6] == 1.0
        assert st[7] == pytest.approx(norm, rel=1e-11)
    a.guarded(max_norm=norm * 0.5, scale=0.25)
    st = a.state_list()
    assert a.eff_scale() < 0.25 and st[2] == 1.0 and st[6] == pytest.approx(0.5, rel=1e-5)


# ---------------------------------------------------------------------------------------------- 5. capture
def _captured_run(seed):
    a = Arena((0.9, 0.999), True, seed=17)
    warm = Arena((0.9, 0.999), True, seed=17)
    warm.guarded(max_norm=0.05)                                       # first launches outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.set_grad(np.zeros(a.n, dtype=np.float32))
        with torch.cuda.graph(graph, stream=s):
            a.guarded(skip=True, max_norm=0.05, scale=0.5)
    torch.cuda.current_stream().wait_stream(s)
    a.state.copy_(torch.tensor(optim.GUARD_STATE_INIT, dtype=torch.float64))
    rng = np.random.default_rng(seed)
    for i in range(8):
        g = _grad(rng, a.n, scale=1.0 if i % 3 else 1e-4)
        if i in (2, 3):
            g[4000 + i] = math.inf
        a.set_grad(g)
        graph.replay()
    torch.cuda.synchronize()
    return a


def test_the_three_launches_replay_from_a_graph():
    """captured once, replayed eight times (applied, clipped and skipped steps among them): two runs are bitwise equal, and equal
    to the same launches issued eagerly"""
    a, b = _captured_run(18), _captured_run(18)
    assert not a.differs_from(b) and a.state_list() == b.state_list() and torch.equal(a.ctrl, b.ctrl)
    e = Arena((0.9, 0.999), True, seed=17)
    rng = np.random.default_rng(18)
    for i in range(8):
        g = _grad(rng, e.n, scale=1.0 if i % 3 else 1e-4)
        if i in (2, 3):
            g[4000 + i] = math.inf
        e.set_grad(g)
        e.guarded(skip=True, max_norm=0.05, scale=0.5)
    assert not a.differs_from(e) and a.state_list() == e.state_list()
    st = a.state_list()
    assert st[:5] == [6.0, 2.0, 4.0, 0.0, 2.0], st


# ---------------------------------------------------------------------------------------------- 6. MiniTrainer end to end
S, B = 64, 4
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
QC_STD = dict(num_embeddings=64, embedding_dim=16, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
N_STEPS = 6


def _batches(count, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(B, 3, S, S, generator=g).to(DEV) for _ in range(count)]


def _train(graphed, guard, poison=(), leave_out=(), betas=(0.0, 0.99), max_grad_norm=None):
    """N_STEPS steps in deterministic fp32 mode.  ``poison``: steps on which a NaN is written into ``opt.flat_g`` behind the
    all-reduce; ``leave_out``: steps on which ``opt.step()`` is not called (the guard-off twin)."""
    torch.manual_seed(0)
    m = model_mod.VQVAE(S, AE, QC_STD, None, dict(TC, betas=betas), compute_dtype=torch.float32).to(DEV).train()
    tr = trainer_mod.MiniTrainer(max_epochs=1, num_training_batches=N_STEPS, deterministic=True)
    opt = tr.attach(m)[0]
    if guard:
        opt.enable_guard(skip_nonfinite=True, max_grad_norm=max_grad_norm)
    m.on_train_start()
    feed = _batches(N_STEPS, seed=21)
    now = {'i': None}
    real_reduce, real_step = opt.all_reduce_grads, opt.step

    def reduce_then_poison(*a, **k):
        out = real_reduce(*a, **k)
        if now['i'] in poison:
            opt.flat_g[int(opt.seg_end[0]) - 1] = math.nan          # the last element of the first tensor
        return out

    def step_or_not(*a, **k):
        return None if now['i'] in leave_out else real_step(*a, **k)
    opt.all_reduce_grads, opt.step = reduce_then_poison, step_or_not
    after_capture = None
    if graphed:
        tr.capture(m, feed[0], warmup=1, preserve_state=True)
        after_capture = opt.guard_state()
    run = tr.train_batch_graphed if graphed else tr.train_batch
    for i in range(N_STEPS):
        now['i'] = i
        run(m, feed[i], i)
    torch.cuda.synchronize()
    state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    state['optimizer.v'] = opt.flat_v.detach().cpu().clone()
    if opt.flat_m is not None:
        state['optimizer.m'] = opt.flat_m.detach().cpu().clone()
    sd = opt.state_dict()
    return dict(state=state, step=float(sd['state'][0]['step']), guard=opt.guard_state(), after_capture=after_capture, opt=opt, tr=tr,
                model=m)


def _differing(a, b):
    assert set(a) == set(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize('betas', [(0.0, 0.99), (0.9, 0.999)], ids=['b1=0', 'b1=0.9'])
@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
def test_trainer_guard_on_and_idle_is_bit_identical_to_guard_off(graphed, betas):
    off = _train(graphed, False, betas=betas)
    ops.set_deterministic(False)
    on = _train(graphed, True, betas=betas, max_grad_norm=1e9)
    differ = _differing(on['state'], off['state'])
    print(f'STEPGUARDMEASURE trainer graphed={graphed} betas={betas}: {len(differ)} of {len(on["state"])} tensors differ guard on / off {differ[:4]}')
    assert not differ and on['step'] == off['step'] == float(N_STEPS)
    g = on['guard']
    assert (g['applied'], g['skipped'], g['clipped'], g['max_consecutive_skipped']) == (N_STEPS, 0, 0, 0) and g['clip_coef_min'] == 1.0
    assert g['last_norm'] > 0.0 and off['guard'] is None
    if graphed:
        assert on['after_capture']['applied'] == 0 and on['after_capture']['skipped'] == 0 and on['after_capture']['clip_coef_sum'] == 0.0


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
def test_trainer_poisoned_steps_equal_steps_never_taken(graphed):
    bad = (1, 2, 4)
    on = _train(graphed, True, poison=bad)
    ops.set_deterministic(False)
    off = _train(graphed, False, leave_out=bad)
    differ = _differing(on['state'], off['state'])
    print(f'STEPGUARDMEASURE trainer graphed={graphed} poisoned {bad}: {len(differ)} tensors differ from the run without those steps {differ[:4]}')
    assert not differ
    g = on['guard']
    assert (g['applied'], g['skipped'], g['max_consecutive_skipped'], g['consecutive_skipped']) == (3, 3, 2, 0)
    assert on['step'] == off['step'] == 3.0                          # the checkpointed step is the applied count
    assert all(torch.isfinite(v).all() for v in on['state'].values() if v.dtype.is_floating_point)
    if graphed:
        assert on['after_capture']['applied'] == 0 and on['after_capture']['skipped'] == 0


def test_guard_settings_checkpoint_and_disable():
    run = _train(False, True, poison=(0,))
    opt, tr, m = run['opt'], run['tr'], run['model']
    assert run['guard']['applied'] == N_STEPS - 1 and opt.step_count == N_STEPS
    opt.enable_guard(skip_nonfinite=True, max_grad_norm=None)        # the same settings again: nothing happens
    assert opt.guard_state()['applied'] == N_STEPS - 1
    with pytest.raises(RuntimeError, match='other settings'):
        opt.enable_guard(skip_nonfinite=True, max_grad_norm=1.0)
    sd = opt.state_dict()
    assert all(float(e['step']) == N_STEPS - 1 for e in sd['state'].values())
    for e in sd['state'].values():
        e['step'] = torch.tensor(41.0)
    opt.load_state_dict(sd)
    assert opt.guard_state()['applied'] == 41 and opt.step_count == 41
    snap = tr._snapshot(m)
    opt.guard['state'][optim.GUARD_SKIPPED] = 9.0
    opt.guard['state'][optim.GUARD_APPLIED] = 50.0
    tr._restore(m, snap)
    assert opt.guard_state()['applied'] == 41 and opt.guard_state()['skipped'] == 1
    rec = opt.guard_epoch_end('autoencoder')
    assert rec['guard/autoencoder/skipped'] == 1 and rec['guard/autoencoder/max_consecutive_skipped'] == 1
    assert opt.guard_epoch_end('autoencoder')['guard/autoencoder/skipped'] == 0
    opt.disable_guard()
    assert opt.guard is None and opt.step_count == 41 and float(opt.state_dict()['state'][0]['step']) == 41.0
    opt.enable_guard(skip_nonfinite=False, max_grad_norm=1.0)        # after disable_guard other settings are fine
    assert opt.guard_state()['applied'] == 41 and opt.guard_state()['skipped'] == 0


def test_scalar_log_shares_its_statistics_pass_with_the_guard(tmp_path):
    """with a scalar log attached the guard launches no statistics pass of its own: it decides on the log's "all" row"""
    scalarlog = importlib.import_module(PKG + '.scalarlog')
    torch.manual_seed(0)
    m = model_mod.VQVAE(S, AE, QC_STD, None, TC, compute_dtype=torch.float32).to(DEV).train()
    m.scalar_log = scalarlog.ScalarLog(str(tmp_path))
    tr = trainer_mod.MiniTrainer(max_epochs=1, num_training_batches=4)
    opt = tr.attach(m)[0]
    opt.enable_guard(skip_nonfinite=True, max_grad_norm=1e-6)
    m.on_train_start()
    calls = {'n': 0}
    real = ops.arena_stats

    def counting(*a, **k):
        calls['n'] += 1
        return real(*a, **k)
    ops.arena_stats = counting
    try:
        feed = _batches(4, seed=22)
        real_stats = m.scalar_log.grad_stats

        def poisoned(o, name):
            if calls['n'] == 2:
                o.flat_g[int(o.seg_end[0]) - 1] = math.inf
            return real_stats(o, name)
        m.scalar_log.grad_stats = poisoned
        for i in range(4):
            tr.train_batch(m, feed[i], i)
        torch.cuda.synchronize()
    finally:
        ops.arena_stats = real
    assert calls['n'] == 4                                            # one pass per step, not two
    g = opt.guard_state()
    assert (g['applied'], g['skipped'], g['clipped']) == (3, 1, 3) and g['clip_coef_min'] < 1.0
    rec = tr.log_train_epoch(m, tr.guard_epoch_end(m))
    assert rec['guard/autoencoder/skipped'] == 1 and rec['grad/all/nonfinite'] == 1.0
    assert g['last_norm'] == pytest.approx(math.sqrt(float(m.scalar_log._opts['autoencoder']['out'][9])), rel=1e-15)
    m.scalar_log.close()


# ---------------------------------------------------------------------------------------------- 7. VQ-GAN: one verdict per optimizer
GAN_Q = dict(num_embeddings=64, embedding_dim=16, reinit_every_n_epochs=None, type='gumbel',
             params=dict(straight_through=False, temp=1.0, kl_cost=5e-4, kl_warmup_epochs=0.5, temp_decay_epochs=2, temp_final=0.25))
GAN_L = dict(l1_weight=0.8, l2_weight=0.2, perc_weight=1.0,
             adversarial_params=dict(start_epoch=0, loss_type='non-saturating', g_weight=0.1, use_adaptive=False,
                                     r1_reg_weight=10.0, r1_reg_every=2))


def test_vqgan_poisoned_discriminator_skips_only_the_discriminator():
    assert trainer_mod.GAN_OPT_OVERLAP                                # the autoencoder's optimizer runs on its side stream
    torch.manual_seed(0)
    m = model_mod.VQVAE(64, AE, GAN_Q, GAN_L, dict(TC, lr=1e-5)).to(DEV).train()
    tr = trainer_mod.MiniTrainer(num_training_batches=6)
    ae_opt, disc_opt = tr.attach(m)
    for o in (ae_opt, disc_opt):
        o.enable_guard(skip_nonfinite=True)
    m.on_train_start()
    images = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    now = {'i': None}
    real = disc_opt.all_reduce_grads

    def poisoned(*a, **k):
        out = real(*a, **k)
        if now['i'] in (1, 2):
            disc_opt.flat_g[int(disc_opt.seg_end[0]) - 1] = math.nan
            disc_opt.flat_g[0] = -math.inf
        return out
    disc_opt.all_reduce_grads = poisoned
    torch.manual_seed(1)
    tr.capture(m, images, warmup=2, preserve_state=True)
    assert ae_opt.guard_state()['applied'] == 0 and disc_opt.guard_state()['applied'] == 0
    for i in range(4):
        now['i'] = i
        torch.cuda.synchronize()
        before = (ae_opt.flat_p.clone(), disc_opt.flat_p.clone(), disc_opt.flat_v.clone())
        tr.train_batch_graphed(m, images, i)
        torch.cuda.synchronize()
        assert not torch.equal(before[0], ae_opt.flat_p), i           # the autoencoder always steps
        moved = not (_same_bits(before[1], disc_opt.flat_p) and _same_bits(before[2], disc_opt.flat_v))
        assert moved == (i not in (1, 2)), i
    a, d = ae_opt.guard_state(), disc_opt.guard_state()
    assert (a['applied'], a['skipped']) == (4, 0) and (d['applied'], d['skipped'], d['max_consecutive_skipped']) == (2, 2, 2)
    assert torch.isfinite(ae_opt.flat_p).all() and torch.isfinite(disc_opt.flat_p).all() and torch.isfinite(disc_opt.flat_v).all()
    assert float(disc_opt.state_dict()['state'][0]['step']) == 2.0 and float(ae_opt.state_dict()['state'][0]['step']) == 4.0


# ---------------------------------------------------------------------------------------------- 8. two ranks on one GPU over gloo
def _gloo_worker(rank, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK='0', WORLD_SIZE='2',
                      HSA_ENABLE_IPC_MODE_LEGACY='0', VQK_SPLIT_ENCODER_FRACTION='0.5')
    r, local, world = trainer_mod.init_distributed('gloo')
    assert dist.get_backend() == 'gloo' and world == 2 and local == 0
    torch.cuda.set_device(0)
    native.check(native.lib().vqk_set_tuning(b'GN_CLUSTER_MAX_HW', 0), 'set_tuning')     # two processes on one GPU (tests/test_gpu_dist.py)
    torch.manual_seed(0)
    m = model_mod.VQVAE(32, AE, QC_STD, None, dict(TC, lr=1e-5))
    with torch.no_grad():
        m.quantizer.codebook.weight.mul_(32.0)
    m = m.to(DEV).train()
    tr = trainer_mod.MiniTrainer(num_training_batches=100)
    opt = tr.attach(m)[0]
    opt.enable_guard(skip_nonfinite=True, max_grad_norm=None)
    m.on_train_start()
    g = torch.Generator().manual_seed(31)
    images = [torch.rand(4, 3, 32, 32, generator=g) for _ in range(2)][rank].to(DEV)
    now = {'i': None, 'done': False}
    real_range, real_flat = opt.all_reduce_range, opt.all_reduce_grads

    def poison():                                                     # ONE rank, ONE element, in front of the step's first collective
        if rank == 1 and now['i'] == 1 and not now['done']:
            now['done'] = True
            opt.flat_g[0] = math.nan

    def ranged(lo, hi, *a, **k):
        if lo == 0:
            poison()
        return real_range(lo, hi, *a, **k)

    def flat(*a, **k):
        poison()
        return real_flat(*a, **k)
    opt.all_reduce_range, opt.all_reduce_grads = ranged, flat
    tr.capture(m, images, warmup=2, preserve_state=True)
    assert opt.guard_state()['applied'] == 0
    states = []
    for i in range(3):
        now['i'] = i
        tr.train_batch_graphed(m, images, i)
        torch.cuda.synchronize()
        states.append(opt.guard_state())
    dist.barrier()
    out.put((rank, states, opt.flat_p.detach().cpu().numpy(), opt.flat_v.detach().cpu().numpy(), now['done']))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_poisoned_both_skip():
    """the verdict is taken on the all-reduced arena, which is the same on every rank: a NaN on one rank reaches both through the
    sum, both leave the step out, and the replicas stay identical -- without another collective"""
    ctx = mp.get_context('spawn')
    out = ctx.SimpleQueue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 29661, out)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    deadline = time.time() + 300
    try:
        # a worker that raises puts nothing on the queue (and leaves its peer waiting in a collective): never block on the queue
        while len(got) < 2 and time.time() < deadline and all(p.exitcode in (None, 0) for p in procs):
            if out.empty():
                if not any(p.is_alive() for p in procs):
                    break
                time.sleep(0.2)
                continue
            rank, states, p_, v_, done = out.get()
            got[rank] = (states, p_, v_, done)
        for p in procs:
            p.join(60 if len(got) == 2 else 1)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
    assert len(got) == 2 and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert got[1][3] and not got[0][3]
    for rank in (0, 1):
        states = got[rank][0]
        assert [(s['applied'], s['skipped']) for s in states] == [(1, 0), (1, 1), (2, 1)], (rank, states)
        assert np.isfinite(got[rank][1]).all() and np.isfinite(got[rank][2]).all()
    assert np.array_equal(got[0][1].view(np.int32), got[1][1].view(np.int32))
    assert np.array_equal(got[0][2].view(np.int32), got[1][2].view(np.int32))
    assert got[0][0][2]['last_norm'] == got[1][0][2]['last_norm']


# ---------------------------------------------------------------------------------------------- 9. train.py
def _train_py(tmp_path, graphed, bad_steps, capsys):
    """train.py on synthetic batches, 2 epochs x 4 steps; a NaN goes into the gradient arena on the guarded steps ``bad_steps``
    (counted by the guard itself: the settling step of the capture is put back and does not count)"""
    train = importlib.import_module(PKG + '.train')
    conf = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'example_confs', 'standard_vqvae.yaml')
    sets = [f'image_size={S}', 'autoencoder.channels=32', 'autoencoder.num_res_blocks=1', 'autoencoder.channel_multipliers=[1, 2]',
            'quantizer.num_embeddings=64', 'quantizer.embedding_dim=16', 'training.cumulative_bs=4']
    args = ['--params_file', conf, '--seed', '3', '--max_epochs', '2', '--batches_per_epoch', '4', '--dtype', 'bf16',
            '--log_dir', str(tmp_path), '--run_name', 'r1', '--skip_nonfinite_steps', '--gradient_clip_val', '1e-6']
    if not graphed:
        args.append('--no-graph')
    for item in sets:
        args += ['--set', item]
    real = optim.FlatAdamW.all_reduce_grads

    def poisoned(self, *a, **k):
        out = real(self, *a, **k)
        if self.guard is not None and (bad_steps == 'all' or self.guard['steps'] in bad_steps):
            self.flat_g[int(self.seg_end[0]) - 1] = math.nan
        return out
    optim.FlatAdamW.all_reduce_grads = poisoned
    capsys.readouterr()
    try:
        loss = train.main(args)
    finally:
        optim.FlatAdamW.all_reduce_grads = real
    text = capsys.readouterr().out
    assert ('eager launches' not in text) and np.isfinite(loss)
    return text, [json.loads(x) for x in open(tmp_path / 'r1' / 'metrics.jsonl', encoding='utf-8').read().splitlines()]


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
def test_train_py_flags_end_to_end(tmp_path, capsys, graphed):
    text, recs = _train_py(tmp_path, graphed, {1, 2, 6}, capsys)
    epochs = [r for r in recs if r['event'] == 'train_epoch']
    assert len(epochs) == 2
    pre = 'guard/autoencoder/'
    want = [dict(applied=2, skipped=2, clipped=2, max_consecutive_skipped=2), dict(applied=3, skipped=1, clipped=3, max_consecutive_skipped=1)]
    for e in range(2):
        for k, v in want[e].items():
            assert epochs[e][pre + k] == v, (e, k, epochs[e][pre + k])
        assert 0.0 < epochs[e][pre + 'clip_coef_min'] <= epochs[e][pre + 'clip_coef_mean'] < 1.0       # 1e-6 / norm
        assert epochs[e]['grad/all/nonfinite'] == want[e]['skipped'] and math.isfinite(epochs[e]['train/loss'])
        assert not any(k.startswith('guard/discriminator') for k in epochs[e])
    assert '[epoch 0] autoencoder: 2 steps skipped (non-finite gradients), 2 clipped, 2 applied' in text
    assert '[epoch 1] autoencoder: 1 steps skipped (non-finite gradients), 3 clipped, 3 applied' in text


def test_train_py_stops_when_every_step_of_an_epoch_is_skipped(tmp_path, capsys):
    with pytest.raises(RuntimeError, match='every one of the 4 autoencoder optimizer steps of epoch 0'):
        _train_py(tmp_path, True, 'all', capsys)
