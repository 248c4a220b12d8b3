"""tests/adamw_reference.py on the CPU: the float64 step is torch.optim.AdamW's, the rounding bound is reachable by a plain float32
evaluation in the kernel's operation order, and every case can see the mistakes a segment-searching, bias-correcting kernel
could make -- each mistake, applied to the float64 step, leaves 10 x the bound.  tests/test_gpu_adamw.py asserts 1 x the bound
on the same cases, so it is not vacuous.

Measured (step32 against step64, all cases): worst error / bound 0.60 on p, 0.44 on v, 0.47 on m."""
import numpy as np
import pytest
import torch

from tests import adamw_reference as A

CASES = A.all_cases()
UNIT = [c for c in CASES if c.kind == 'unit']
IDS = [c.name for c in CASES]


def _correct(case):
    x = case.inputs()
    res = A.step64(x['p'], x['g'], x['m'], x['v'], case.wd, **case.hyper())
    return x, res, A.bound(res['A'], res['U'], res['v'], res['M'])


def _leaves(wrong, right, bound):
    """elementwise: farther than 10 x bound (a non-finite wrong value is far)"""
    with np.errstate(all='ignore'):
        return ~(np.abs(wrong - right) <= 10.0 * bound)


def test_case_lists_cover_what_the_gpu_test_needs():
    names = {c.name for c in CASES}
    assert len(names) == len(CASES)
    big = A.TABLES
    assert sorted({int(e) % 4 for e in big['residues']()['ends']}) == [0, 1, 2, 3]
    ones = np.diff(big['ones']()['ends'])
    assert (ones == 1).sum() == 40 and big['ones']()['ends'][0] < A.CHUNK < big['ones']()['ends'][-2]
    assert {1024, 8191, 8192, 8193} <= set(big['edges']()['ends'].tolist())
    flat = big['flat']()
    sizes = np.diff(np.concatenate([[0], flat['ends']]))
    assert flat['pad'].sum() == 10 and all(int(e) % 64 == 0 for e in flat['ends'][flat['pad']]) and (sizes[:-1:2] % 64 != 0).all()
    many = big['many']()
    assert len(many['ends']) == 256 and len(set(many['wd'].tolist())) == 256
    assert (np.diff(big['empty']()['ends']) == 0).sum() == 3
    for fn in big.values():
        t = fn()
        assert int(t['ends'][-1]) == A.N_BIG
        sizes = np.diff(np.concatenate([[0], t['ends']]))
        wd = t['wd'][sizes > 0].astype(np.float64)                 # neighbouring non-empty segments, and empty ones and theirs
        assert (np.abs(np.diff(wd)) >= 0.0099).all() and (np.abs(np.diff(t['wd'].astype(np.float64))) >= 0.0099).all()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_float32_in_the_kernels_order_meets_the_bound(case):
    x = case.inputs()
    p, m, v = A.step32(x['p'], x['g'], x['m'], x['v'], case.wd, **case.hyper())
    assert np.isfinite(p).all() and np.isfinite(v).all() and np.isfinite(m).all()       # nothing overflows, also in 'wide'
    ok, ratios = A.check(case, x, p, v, m)
    print(f'ADAMWMEASURE cpu {case.name}: step32 / bound p {ratios["p"]:.3f} v {ratios["v"]:.3f} m {ratios["m"]:.3f}')
    assert ok, ratios
    pad = case.pad
    assert np.array_equal(p[pad].view(np.int32), x['p'][pad].view(np.int32)) and not v[pad].any() and not m[pad].any()
    if case.kind == 'zero':                                       # the update is exactly 0: p takes only its decay
        lr = np.float32(case.lr)
        assert np.array_equal(p, x['p'] * (np.float32(1.0) - lr * case.wd)) and not v.any()


# ---------------------------------------------------------------------------------------------- the mistakes
@pytest.mark.parametrize('case', UNIT, ids=[c.name for c in UNIT])
@pytest.mark.parametrize('shift', [-1, 1], ids=['previous', 'next'])
def test_decay_of_the_neighbouring_segment_is_seen(case, shift):
    """on every element that has a previous (next) segment -- so on every element whose neighbour lies in another one"""
    x, res, (bp, _, _) = _correct(case)
    wd, hit, boundary = case.neighbour_wd(shift)
    if len(case.seg_wd) == 1:
        assert not hit.any()
        return
    assert boundary.any() and (hit & boundary).sum() == boundary.sum()
    wrong = A.step64(x['p'], x['g'], x['m'], x['v'], wd, **case.hyper())
    assert _leaves(wrong['p'], res['p'], bp)[hit].all()


# a step count off by one in a bias correction moves the update by the relative change of that correction (half of it
# for bc2, under the root).  A 'unit' case has U >= lr / 8 and A <= 2, so 10 x bound is at most 10 * 2^-24 * (4 * 2 * 8 / lr + 16) U
# = 7.7e-4 U at lr = 0.05: a relative change of 4e-3 in either correction is seen on every element.  Smaller changes -- beta^t
# has died away -- are not a mistake a float32 kernel can be caught at, and are left out.
T_SHIFT_SEEN = 4e-3


@pytest.mark.parametrize('case', UNIT, ids=[c.name for c in UNIT])
@pytest.mark.parametrize('mutation', ['bc1_t-1', 'bc1_t+1', 'bc2_t-1', 'bc2_t+1'])
def test_step_count_off_by_one_is_seen(case, mutation):
    which, dt = (0 if mutation.startswith('bc1') else 1), (1 if mutation.endswith('+1') else -1)
    shift = A.bias_shift(case.betas[which], case.t, dt)
    if shift < T_SHIFT_SEEN:
        assert case.betas[which] == 0.0 or case.t >= 10
        return
    x, res, (bp, _, _) = _correct(case)
    wrong = A.step64(x['p'], x['g'], x['m'], x['v'], case.wd, mutate=mutation, **case.hyper())
    live = ~case.pad                                              # (padding holds g = v = m = 0: there is no update to get wrong)
    assert _leaves(wrong['p'], res['p'], bp)[live].all()


def test_step_count_mistakes_are_checked_where_they_matter():
    """the selection above keeps every beta pair at t = 1, 2, 3 and 10"""
    for mf, (betas, _) in A.M_FORMS.items():
        for t in (1, 2, 3, 10):
            for dt in (-1, 1):
                assert A.bias_shift(betas[1], t, dt) >= T_SHIFT_SEEN
                assert betas[0] == 0.0 or (betas[0] == 0.5 and t == 10) or A.bias_shift(betas[0], t, dt) >= T_SHIFT_SEEN
    assert {c.t for c in UNIT} == set(A.T_VALUES)


@pytest.mark.parametrize('case', UNIT, ids=[c.name for c in UNIT])
def test_wrong_moments_and_scale_are_seen(case):
    x, res, (bp, bv, bm) = _correct(case)
    live = ~case.pad

    def wrong(mutation):
        return A.step64(x['p'], x['g'], x['m'], x['v'], case.wd, mutate=mutation, **case.hyper())
    w = wrong('eps_in_sqrt')
    assert _leaves(w['p'], res['p'], bp)[live].all()
    if case.grad_scale != 1.0:
        w = wrong('scale_dropped')
        assert _leaves(w['v'], res['v'], bv)[live].all()
        assert _leaves(w['m'], res['m'], bm)[live].mean() >= 0.99
        w = wrong('v_unscaled_g')
        assert _leaves(w['v'], res['v'], bv)[live].all()
    if case.store_m:
        w = wrong('m_not_updated')
        assert _leaves(w['m'], res['m'], bm)[live].mean() >= 0.99
        if case.betas[0] != 0.0:                                  # (with beta1 = 0 the stored moment does not reach p)
            assert _leaves(w['p'], res['p'], bp)[live].mean() >= 0.99


def test_scale_mistakes_are_checked():
    assert sum(c.grad_scale != 1.0 for c in UNIT) >= len(UNIT) - 2 and {c.grad_scale for c in UNIT} == set(A.SCALES)


# ---------------------------------------------------------------------------------------------- torch.optim.AdamW
@pytest.mark.parametrize('m_form', ['b1=0,m=null', 'b1=0.9', 'b1=0.5'])
def test_step64_is_torch_adamw(m_form):
    """three steps, two groups (decay 0.1 and 0), a per-step lr, float32-rounded hyper-parameters on both sides"""
    betas, store_m = A.M_FORMS[m_form]
    rng = np.random.default_rng(7)
    sizes, wds = (37, 91), (0.1, 0.0)
    n = sum(sizes)
    wd = np.repeat(np.asarray(wds, dtype=np.float32), sizes)
    p0 = rng.standard_normal(n).astype(np.float32)
    params = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in np.split(p0.astype(np.float64), [sizes[0]])]
    opt = torch.optim.AdamW([dict(params=[q], weight_decay=A.f32(w)) for q, w in zip(params, wds)], lr=1.0,
                            betas=(A.f32(betas[0]), A.f32(betas[1])), eps=A.f32(1e-8))
    p, m, v = p0.astype(np.float64), (np.zeros(n) if store_m else None), np.zeros(n)
    for t, lr in enumerate((0.05, 0.03, 2e-3), start=1):
        g = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        for grp in opt.param_groups:
            grp['lr'] = A.f32(lr)
        for q, gq in zip(params, np.split(g.astype(np.float64) * 0.5, [sizes[0]])):
            q.grad = torch.tensor(gq)
        opt.step()
        res = A.step64(p, g, m, v, wd, lr, betas[0], betas[1], 1e-8, t, grad_scale=0.5)
        p, v = res['p'], res['v']
        m = res['m'] if store_m else None
        want = torch.cat([q.detach() for q in params]).numpy()
        want_v = torch.cat([opt.state[q]['exp_avg_sq'] for q in params]).numpy()
        want_m = torch.cat([opt.state[q]['exp_avg'] for q in params]).numpy()
        np.testing.assert_allclose(p, want, rtol=1e-13, atol=0)
        np.testing.assert_allclose(v, want_v, rtol=1e-13, atol=0)
        np.testing.assert_allclose(res['m'], want_m, rtol=1e-13, atol=1e-300)
    # the unrounded 0.9 / 0.999 would not do: it moves the result by several bounds
    if betas[0]:
        x = A.Case('probe', A.table_single(4096), m_form=m_form, t=10).inputs()
        wd1 = np.full(4096, np.float32(0.1))
        res = A.step64(x['p'], x['g'], x['m'], x['v'], wd1, 0.05, betas[0], betas[1], 1e-8, 10, 0.5)
        bp, _, _ = A.bound(res['A'], res['U'], res['v'], res['M'])
        b1, b2 = betas
        pp, mm, vv = x['p'].astype(np.float64), b1 * x['m'].astype(np.float64), b2 * x['v'].astype(np.float64)
        gs = x['g'].astype(np.float64) * 0.5
        mm += (1 - b1) * gs
        vv += (1 - b2) * gs * gs
        lr = A.f32(0.05)
        unrounded = pp * (1 - lr * 0.1) - lr / (1 - b1 ** 10) * mm / (np.sqrt(vv) / np.sqrt(1 - b2 ** 10) + A.f32(1e-8))
        if m_form == 'b1=0.9':
            assert (np.abs(unrounded - res['p']) / bp).max() > 2.0
