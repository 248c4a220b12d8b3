"""CPU side of the pointwise / column-sum / metric kernel tests: keeps tests/pointwise_reference.py honest.  Every float64 closed form
against an independent float64 evaluation (avg_pool2d, nearest interpolation, autograd through tanh and mse_loss, x.sum(0), scipy's
valid correlation for SSIM), the premises of the ``exact`` input kind for every listed case (the result is representable in the
output type; the sum of the absolute terms stays below 2^24, so every fp32 partial sum is exact in any order), the launcher mirrors
against the numbers derived by hand in the case tables, and the SSIM ``TABLE`` against a fresh run of the fp32 restatement.
Figures are printed (``PWMEASURE cpu``) before they are asserted."""
import pytest
import torch
import torch.nn.functional as F

import pointwise_reference as R

D = torch.float64
KINDS = ('exact', 'real')


def _close(got, want, tol=1e-12):
    err = float((got - want).abs().max() / max(float(want.abs().max()), 1e-300))
    assert err <= tol, err


# ---------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize('scale', R.POOL_SCALES)
def test_pool_and_unpool_closed_forms(scale):
    x = R.pool_input('real', 'fp32', 3, 6, 10, 8)
    nchw = x.permute(0, 3, 1, 2)
    _close(R.pool(x, scale), (F.avg_pool2d(nchw, 2) * 4.0 * scale).permute(0, 2, 3, 1))
    _close(R.unpool(x, scale), (F.interpolate(nchw, scale_factor=2, mode='nearest') * scale).permute(0, 2, 3, 1), 0.0)
    assert float(R.pool_terms(x, scale).min()) >= 0 and bool((R.pool_terms(x, scale) >= R.pool(x, scale).abs() - 1e-15).all())
    # adjointness: <pool(x), y> == <x, unpool(y)> at equal scale
    y = R.pool_input('exact', 'fp32', 3, 3, 5, 8, tag='adj')
    xe = R.pool_input('exact', 'fp32', 3, 6, 10, 8)
    assert float((R.pool(xe, scale) * y).sum()) == float((xe * R.unpool(y, scale)).sum())


def test_preprocess_closed_form():
    img = R.preprocess_input('real', 2, 3, 5)
    out, terms = R.preprocess(img, 8)
    assert bool((out[..., 3:] == 0).all()) and bool((terms[..., 3:] == 0).all())
    _close(out[..., :3], (img.clamp(0, 1) * 2 - 1).permute(0, 2, 3, 1), 1e-15)
    vals = set(img.float().view(-1).tolist())
    assert all(torch.tensor(v, dtype=torch.float32).item() in vals for v in R.PRE_SPECIAL)       # the edge values are in the input
    assert float(img.min()) < 0 and float(img.max()) > 1


@pytest.mark.parametrize('through', (0, 1))
@pytest.mark.parametrize('gs', (None, 0.5))
def test_loss_backward_closed_forms_equal_autograd(through, gs):
    """y = tanh(u): d loss / d u through autograd against mse_bwd (through_tanh) and tanh_bwd"""
    g = R.gen('autograd', through, gs)
    u = torch.randn(257, generator=g, dtype=D).requires_grad_(True)
    t = torch.randn(257, generator=g, dtype=D)
    y = torch.tanh(u)
    leaf = u if through else y
    loss = F.mse_loss(y, t, reduction='sum') * R.MSE_GSCALE * (1.0 if gs is None else gs)
    want, = torch.autograd.grad(loss, leaf)
    got, terms = R.mse_bwd(y.detach(), t, R.MSE_GSCALE, gs, through)
    _close(got, want)
    assert bool((terms >= got.abs() - 1e-15).all())
    _close(R.sse(y.detach(), t), F.mse_loss(y.detach(), t, reduction='sum'))
    dy = torch.randn(257, generator=g, dtype=D)
    want2, = torch.autograd.grad(torch.tanh(u), u, dy)
    _close(R.tanh_bwd(dy, y.detach())[0], want2)


def test_axpby_colsum_and_pair_stats_closed_forms():
    x, y2 = R.axpby_input('real', 'fp32', 64)
    _close(R.axpby(x, y2, -2.0, 0.25)[0], torch.add(-2.0 * x, y2, alpha=0.25))
    _close(R.axpby(x, None, 0.5, 0.0)[0], x / 2, 0.0)
    m, pre = R.colsum_input('real', 'bf16', 130, 12, 5)
    _close(R.colsum(m, 5, 0.25, pre), pre + 0.25 * m.sum(0)[:5])
    _close(R.colsum(m, 12, 1.0, torch.zeros(12, dtype=D)), (torch.ones(1, 130, dtype=D) @ m)[0])
    p, t = R.pair_input('real', 300)
    a = R.pair_stats(p, t)
    assert a.tolist() == [float(((p - t) ** 2).sum()), float(torch.amin(t)), float(torch.amax(t)), float(torch.amin(p)), float(torch.amax(p))]
    p2, t2 = R.pair_input('real', 300, negative=True)
    both = R.pair_stats(p2, t2, a)
    cat = R.pair_stats(torch.cat([p, p2]), torch.cat([t, t2]))
    _close(both[:1], cat[:1])
    assert both[1:].tolist() == cat[1:].tolist() and float(t2.max()) < 0 and float(p2.max()) < 0


@pytest.mark.parametrize('ks', (11, 7))
def test_ssim_closed_form_equals_valid_correlation(ks):
    from scipy.signal import correlate2d
    sigma = R.SSIM_SIGMA[ks]
    win = R.ssim_window(sigma)
    assert tuple(win.shape) == (ks, ks) and abs(float(win.double().sum()) - 1.0) < 1e-6
    shape = R.SSIM_SHAPES[ks][2]
    p, t = R.ssim_input('noisy', shape)
    got = R.ssim_per_image(p, t, sigma).numpy()
    pd, td, wd = p.double().numpy(), t.double().numpy(), win.double().numpy()
    rng = max(pd.max() - pd.min(), td.max() - td.min())
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    for b in range(shape[0]):
        maps = []
        for c in range(shape[1]):
            f = lambda z: correlate2d(z, wd, mode='valid')                     # noqa: E731
            a, q = pd[b, c], td[b, c]
            ma, mq = f(a), f(q)
            saa, sqq, saq = f(a * a) - ma * ma, f(q * q) - mq * mq, f(a * q) - ma * mq
            maps.append(((2 * ma * mq + c1) * (2 * saq + c2)) / ((ma * ma + mq * mq + c1) * (saa + sqq + c2)))
        err = abs(float(sum(m.mean() for m in maps)) / shape[1] - got[b])
        print(f'PWMEASURE cpu ssim-closed-form ks{ks} image {b} {err:.2e}/1.0e-12')
        assert err < 1e-12


def test_ssim_inputs_are_what_their_names_say():
    for ks, shapes in R.SSIM_SHAPES.items():
        for shape in shapes:
            rng = lambda z: float(z.max() - z.min())                           # noqa: E731
            p, t = R.ssim_input('noisy', shape)
            assert rng(t) == 1.0 and rng(p) <= 0.9 + 1e-6
            p, t = R.ssim_input('prange', shape)
            assert rng(p) == 1.0 and rng(t) <= 0.9 + 1e-6
            p, t = R.ssim_input('same', shape)
            assert torch.equal(p, t)
            per = R.ssim_per_image(*R.ssim_input('noisy', shape), R.SSIM_SIGMA[ks])
            assert float(per.max() - per.min()) > 0.2, per                      # a sum in the wrong image's slot is visible
            assert torch.allclose(R.ssim_per_image(p, t, R.SSIM_SIGMA[ks]), torch.ones(shape[0], dtype=D), atol=1e-14, rtol=0)


# ---------------------------------------------------------------------------------------------- premises of the exact kind
def _exact_sum_ok(terms_abs_sum):
    return float(terms_abs_sum) < 2.0 ** 24


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_exact_premises_elementwise(dtype):
    for case in R.POOL_SHAPES:
        n, h, w, c = R.pool_shape(case, dtype)
        if case[0] == 'past-cap':
            n, h, w = 1, 8, 8                                                   # the same maker: values do not depend on the size
        x = R.pool_input('exact', dtype, n, h, w, c)
        for scale in R.POOL_SCALES:
            assert R.representable(x, dtype) and R.representable(R.pool(x, scale), dtype) and R.representable(R.unpool(x, scale), dtype)
    for name, n, h, w in R.PRE_SHAPES:
        img = R.preprocess_input('exact', n, min(h, 64), min(w, 64))
        assert R.representable(img, 'fp32') and R.representable(R.preprocess(img, R.vec(dtype))[0], dtype)
    for n in R.SMALL_N + (4099,):
        dy, y = R.tanh_bwd_input('exact', dtype, n)
        assert R.representable(dy, dtype) and R.representable(y, dtype) and R.representable(R.tanh_bwd(dy, y)[0], dtype)
        assert R.representable(1.0 - y * y, 'fp32')
        r, t = R.mse_bwd_input('exact', dtype, n)
        assert R.representable(r, dtype) and R.representable(t, 'fp32') and R.representable(r - t, 'fp32')
        for through in (0, 1):
            for gs in (None, 0.5):
                assert R.representable(R.mse_bwd(r, t, R.MSE_GSCALE, gs, through)[0], dtype)
        if n >= 3:
            assert float(R.mse_bwd(r, t, 1.0, None, 1)[0][n // 2]) == 0.0 and abs(float(r[n // 2])) == 1.0
        x, y2 = R.axpby_input('exact', dtype, 8 * n)
        for a, b in R.AXPBY_AB:
            assert R.representable(R.axpby(x, y2, a, b)[0], dtype) and R.representable(R.axpby(x, None, a, 0.0)[0], dtype)


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_exact_premises_sums(dtype):
    for n in R.SMALL_N + R.SUM_EDGE_N + (R.PAST_SSE,):
        r, t = R.sse_input('exact', dtype, n)
        assert R.representable(r, dtype) and R.representable(t, 'fp32')
        assert _exact_sum_ok(((r - t) ** 2).sum() + 8) and R.representable(R.sse(r, t) + 5.0, 'fp32')
        if dtype == 'fp32':
            for neg in (False, True):
                p, t = R.pair_input('exact', n, neg)
                assert R.representable(p, 'fp32') and R.representable(t, 'fp32') and _exact_sum_ok(2 * ((p - t) ** 2).sum())
                assert (not neg) or (float(t.max()) < 0 and float(p.max()) < 0)
    for case in R.COLSUM_CASES:
        if case[1] != dtype:
            continue
        name, _, rows, c, lead, scale = case[:6]
        x, pre = R.colsum_input('exact', dtype, rows, c, lead or c)
        assert R.representable(x, dtype) and _exact_sum_ok(x.abs().sum(0).max() + 8)
        assert R.representable(R.colsum(x, lead or c, scale, pre), 'fp32') and scale in (1.0, 0.5, 0.25)
    for name, dt, rows, c, room, _ in R.HALVING_CASES:
        if dt == dtype:
            x, pre = R.colsum_input('exact', dtype, rows, c, c)
            assert _exact_sum_ok(x.abs().sum(0).max() + 8)


# ---------------------------------------------------------------------------------------------- launcher mirrors
def test_colsum_mirror_reproduces_the_hand_derived_table():
    assert R.colsum_plan('fp32', 130, 96)['rstep'] == 10 and R.colsum_plan('fp32', 130, 96)['idle'] == 16
    assert R.colsum_plan('bf16', 130, 24)['rstep'] == 85 and R.colsum_plan('bf16', 130, 24)['idle'] == 1
    p = R.colsum_plan('bf16', 130, 128)
    assert (p['form'], p['blocks'], p['rpb'], p['idle']) == ('vector', 3, 44, 0)
    assert R.colsum_plan('fp32', 70, 1028)['slot_trips'] == 2 and R.colsum_plan('fp32', 70, 1024)['form'] == 'vector'
    assert R.colsum_plan('bf16', 130, 65)['col_trips'] == 2
    p = R.colsum_plan('bf16', 1000, 128, det=True, ws_bytes=4 * 128 * 4)
    assert (p['nb_first'], p['nb_halved'], p['blocks'], p['rpb']) == (16, 4, 4, 250)
    assert R.colsum_plan('fp32', 2200, 4, det=True)['reduce_trips'] == 2 and R.colsum_plan('fp32', 2000, 4, det=True)['reduce_trips'] == 1
    assert R.colsum_plan('bf16', 130, 128, det=True, ws_bytes=128 * 4 - 4)['status'] == R.ERR_ARG
    assert R.colsum_plan('bf16', 130, 8193)['status'] == R.ERR_SHAPE and R.colsum_plan('bf16', 0, 8)['form'] == 'none'
    for case in R.COLSUM_CASES:
        name, dtype, rows, c, lead, scale, off, atomic, det = case
        p = R.colsum_plan(dtype, rows, c, aligned=off == 0)
        assert (p['form'], p['blocks'], p['rpb'], p['rstep']) == atomic, (name, p)
        assert (p['blocks'] - 1) * p['rpb'] < rows <= p['blocks'] * p['rpb']
        q = R.colsum_plan(dtype, rows, c, aligned=off == 0, det=True)
        assert (q['form'], q['blocks'], q['rpb']) == det and q['nb_halved'] == q['nb_first'], (name, q)
    for name, dtype, rows, c, room, want in R.HALVING_CASES:
        q = R.colsum_plan(dtype, rows, c, det=True, ws_bytes=room * c * 4)
        assert (q['form'], q['nb_first'], q['nb_halved'], q['blocks'], q['rpb']) == want, (name, q)
    forms = {R.colsum_plan(cs[1], cs[2], cs[3], aligned=cs[6] == 0)['form'] for cs in R.COLSUM_CASES}
    assert forms == {'vector', 'wide', 'column'}


def test_grid_mirrors_put_the_large_cases_past_their_caps():
    assert R.pool_plan('fp32', 1, 1448, 1460, 8) == dict(items=1057040, grid=4096, trips=2, capped=True)
    assert R.pool_plan('bf16', 1, 1448, 1460, 16)['trips'] == 2 and R.unpool_plan('fp32', 1, 362, 365, 8)['trips'] == 2
    for dtype in R.DTYPES:
        for case in R.POOL_SHAPES:
            past = case[0] == 'past-cap'
            assert R.pool_plan(dtype, *R.pool_shape(case, dtype))['trips'] == (2 if past else 1)
            assert R.unpool_plan(dtype, *R.unpool_shape(case, dtype))['trips'] == (2 if past else 1)
    assert R.pool_plan('fp32', 3, 6, 10, 4) == dict(items=45, grid=1, trips=1, capped=False)
    assert R.preprocess_plan(1, 1024, 1025) == dict(items=1049600, grid=4096, trips=2, capped=True)
    assert R.preprocess_plan(2, 3, 5)['trips'] == 1
    assert R.sse_plan(R.PAST_SSE) == dict(items=4196355, grid=2048, trips=9, capped=True, form='ordered')
    assert R.sse_plan(R.PAST_SSE, scratch=False)['form'] == 'atomic'
    assert R.sse_plan(2048 * 2048)['trips'] == 8 and not R.sse_plan(2048 * 2048)['capped']
    assert [(R.sse_plan(n)['grid'], R.sse_plan(n)['form']) for n in R.SUM_EDGE_N] == [(32, 'atomic'), (33, 'ordered')]
    assert R.bwd_plan(R.PAST_BWD) == dict(items=2098179, grid=2048, trips=5, capped=True)
    assert R.bwd_plan(2048 * 1024)['trips'] == 4 and not R.bwd_plan(2048 * 1024)['capped']
    for n in R.SMALL_N:
        assert R.sse_plan(n)['grid'] == 1 and R.sse_plan(n)['form'] == 'atomic' and R.bwd_plan(n)['grid'] == 1 and R.sse_plan(n)['trips'] == (2 if n == 257 else 1)
    for dtype in R.DTYPES:
        assert R.axpby_plan(dtype, R.PAST_VEC * R.vec(dtype)) == dict(items=R.PAST_VEC, grid=4096, trips=2, capped=True)
        assert R.axpby_plan(dtype, R.vec(dtype)) == dict(items=1, grid=1, trips=1, capped=False)


def test_ssim_mirror():
    assert R.ssim_plan(3, 1, 11, 30, 11)['grid'] == (2, 1, 3) and R.ssim_plan(3, 1, 11, 30, 11)['oh'] == 1
    assert R.ssim_plan(3, 3, 26, 26, 11)['grid'] == (1, 1, 9) and R.ssim_plan(3, 3, 26, 26, 11)['last_rows'] == 16
    p = R.ssim_plan(3, 3, 27, 27, 11)
    assert p['grid'] == (2, 2, 9) and p['last_rows'] == 1 and p['last_cols'] == 1
    assert R.ssim_plan(3, 1, 27, 43, 11)['grid'] == (3, 2, 3)
    assert [R.ssim_plan(*s, 7)['grid'] for s in R.SSIM_SHAPES[7]] == [(2, 1, 3), (1, 1, 9), (2, 2, 9), (3, 2, 3)]
    for ks, shapes in R.SSIM_SHAPES.items():
        for shape in shapes:
            q = R.ssim_plan(*shape, ks)
            assert (q['grid'], q['last_rows'], q['last_cols']) == R.SSIM_EXPECT[(ks, shape)]
    assert R.ssim_plan(1, 1, 10, 30, 11)['status'] == R.ERR_SHAPE and R.ssim_plan(1, 1, 30, 30, 9)['status'] == R.ERR_ARG


# ---------------------------------------------------------------------------------------------- the SSIM table
@pytest.mark.parametrize('ks', (11, 7))
@pytest.mark.parametrize('kind', R.SSIM_KINDS)
def test_ssim_table_is_honest(kind, ks):
    worst = 0.0
    win = R.ssim_window(R.SSIM_SIGMA[ks])
    for shape in R.SSIM_SHAPES[ks]:
        p, t = R.ssim_input(kind, shape)
        sums = R.ssim_restate(p, t, win)
        if kind == 'same':
            assert sums.tolist() == [float(shape[1] * (shape[2] - ks + 1) * (shape[3] - ks + 1))] * shape[0]      # 1 exactly
        f = R.ssim_figure(sums, R.ssim_per_image(p, t, R.SSIM_SIGMA[ks]), shape, ks)
        print(f'PWMEASURE cpu ssim-restate {kind} ks{ks} {shape} {f:.3e}')
        worst = max(worst, f)
    entry = R.TABLE[(kind, ks)]
    print(f'PWMEASURE cpu ssim-table {kind} ks{ks} measured {worst:.3e} entry {entry:.1e}')
    assert worst <= entry
    if kind != 'same':
        assert entry <= 2 * worst, 'a table entry far above what is measured licenses nothing: re-measure it'
