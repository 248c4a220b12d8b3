"""tests/entropy_reference.py (the float64 reference of the Entropy and Gumbel quantizer tests) held against what it must agree with
on the CPU: torch's float64 autograd of the oracle (oracle/vqvae_oracle.py: vq_entropy both loss types, vq_gumbel soft and hard),
central finite differences of its two analytic row gradients, the zero row sums of the distance cotangent, the truncation of the
split-product scheme, and its own input makers (no row left out, the planted tie, a seed per case).  The last test evaluates the bound
of every case of the two GPU modules from the reference alone: each must be small enough to tell a wrong kernel from a right one."""
import numpy as np
import pytest
import torch

from oracle import vqvae_oracle as O
from tests import entropy_reference as R

SHAPES = [(5, 4, 3), (37, 20, 8), (64, 68, 16)]           # (N, K, D)
BETA, RATIO, GLOSS = 0.25, 0.1, 1.7


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def rows_to_map(a):
    """[N, C] rows -> the [1, C, N, 1] map whose pixels are the rows"""
    return t64(a).t().reshape(1, a.shape[1], a.shape[0], 1)


def map_to_rows(t):
    return t.detach()[0, :, :, 0].t().numpy()


@pytest.mark.parametrize('loss_type', ['softmax', 'argmax'])
@pytest.mark.parametrize('temperature', [1.0, 0.05])
@pytest.mark.parametrize('shape', SHAPES)
def test_entropy_vq_agrees_with_float64_autograd_of_the_oracle(shape, temperature, loss_type):
    n, k, dim = shape
    inp = R.make_entropy_inputs(100 + n, n, k, dim, 1.0 if temperature == 1.0 else 0.2)
    assert inp['rounds'] < R.ROUNDS
    dq = inp['dq'] * 1e3
    z, e = rows_to_map(inp['z']).requires_grad_(True), t64(inp['E']).requires_grad_(True)
    q, idx, loss = O.vq_entropy(z, e, BETA, RATIO, temperature, loss_type)
    ref = R.entropy_vq(inp['z'], inp['E'], BETA, RATIO, temperature, loss_type, dq, GLOSS)
    np.testing.assert_array_equal(idx.reshape(-1).numpy(), ref['idx'])
    assert R.distance(map_to_rows(q), ref['q']) <= 1e-10
    assert R.distance(loss.item(), ref['loss']) <= 1e-10
    for cot_q, cot_l in ((dq, GLOSS), (dq, None), (None, GLOSS)):
        outs = [o for o, c in ((q, cot_q), (loss, cot_l)) if c is not None]
        cots = [rows_to_map(c) if isinstance(c, np.ndarray) else t64(c) for c in (cot_q, cot_l) if c is not None]
        gz, ge = torch.autograd.grad(outs, [z, e], cots, retain_graph=True, allow_unused=True)
        r = R.entropy_vq(inp['z'], inp['E'], BETA, RATIO, temperature, loss_type, cot_q, cot_l)
        assert R.distance(map_to_rows(gz), r['dz']) <= 1e-10
        if cot_l is None:
            assert ge is None or float(ge.abs().max()) == 0.0
            assert not r['dE'].any()
        else:
            assert R.distance(ge.numpy(), r['dE']) <= 1e-10


@pytest.mark.parametrize('hard', [False, True])
@pytest.mark.parametrize('tau', [1.0, 0.3])
@pytest.mark.parametrize('shape', SHAPES)
def test_gumbel_vq_agrees_with_float64_autograd_of_the_oracle(shape, tau, hard):
    n, k, dim = shape
    inp = R.make_gumbel_inputs(200 + n, n, k, tau, ties=[(1, 3)])
    assert inp['rounds'] < R.ROUNDS
    rng = np.random.default_rng(n)
    e_np, dq = rng.standard_normal((k, dim)), rng.standard_normal((n, dim))
    x, e = rows_to_map(inp['logits']).requires_grad_(True), t64(e_np).requires_grad_(True)
    w = torch.eye(k, dtype=torch.float64).reshape(k, k, 1, 1)
    q, idx, kl = O.vq_gumbel(x, e, w, torch.zeros(k, dtype=torch.float64), tau, 5e-2, rows_to_map(inp['noise']), hard)
    ref = R.gumbel_vq(inp['logits'], e_np, inp['noise'], tau, 5e-2, hard, dq, GLOSS)
    np.testing.assert_array_equal(idx.reshape(-1).numpy(), ref['idx'])
    assert R.distance(map_to_rows(q), ref['q']) <= 1e-10
    assert R.distance(kl.item(), ref['kl']) <= 1e-10
    gx, ge = torch.autograd.grad([q, kl], [x, e], [rows_to_map(dq), t64(GLOSS)], retain_graph=True)
    assert R.distance(map_to_rows(gx), ref['dlogits']) <= 1e-10
    assert R.distance(ge.numpy(), ref['dE']) <= 1e-10
    gx, = torch.autograd.grad([q], [x], [rows_to_map(dq)])
    assert R.distance(map_to_rows(gx), R.gumbel_vq(inp['logits'], e_np, inp['noise'], tau, 5e-2, hard, dq, None)['dlogits']) <= 1e-10


def _central(f, x, h):
    g = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (f(xp) - f(xm)) / (2 * h)
    return g


@pytest.mark.parametrize('loss_type', ['softmax', 'argmax'])
def test_entropy_dd_is_the_central_difference_of_the_loss(loss_type):
    n, k, temperature = 6, 8, 0.5
    d = R.make_dmat(3, n, k, 2.0)
    idx = d.argmin(-1)
    hist = np.bincount(idx, minlength=k)

    def loss(dm):
        if loss_type == 'softmax':
            return RATIO * (R.entropy_rows(dm, temperature)[2] / n + R.entropy_cols(dm, temperature)[2])
        # one-hot targets with p's gradient: in a neighbourhood the VALUE of the target is p - stop(p - one_hot)
        _, p, lp = R._softmax_parts(-dm / temperature)
        _, p0, _ = R._softmax_parts(-d / temperature)
        one_hot = np.eye(k)[idx]
        tgt = p - (p0 - one_hot)
        avg = tgt.mean(0)
        return RATIO * (-(tgt * lp).sum(-1).mean() + (avg * np.log(avg + R.EPS_ENT)).sum())
    want = GLOSS * _central(loss, d, 1e-7)           # (log(avg + 1e-5) near avg = 0: a short step)
    assert R.distance(R.entropy_dd(d, temperature, RATIO, GLOSS, loss_type, idx), want) <= 1e-7
    if loss_type == 'argmax':
        f = R.entropy_argmax_forward(d, idx, hist, temperature)
        assert abs(RATIO * (f[3] / n + f[6]) - loss(d)) <= 1e-12


def test_gumbel_rows_backward_is_the_central_difference():
    n, k, tau, klc = 5, 7, 0.6, 0.3
    inp = R.make_gumbel_inputs(5, n, k, tau)
    dy = np.random.default_rng(1).standard_normal((n, k))

    def f(lg):
        _, y, _ = R._softmax_parts(R.gumbel_t(lg, inp['noise'], tau))
        return (y * dy).sum() + klc * R.gumbel_rows(lg, inp['noise'], tau, False)[2]
    assert R.distance(R.gumbel_rows_backward(inp['logits'], inp['noise'], dy, tau, klc), _central(f, inp['logits'], 1e-6)) <= 1e-7


@pytest.mark.parametrize('loss_type', ['softmax', 'argmax'])
@pytest.mark.parametrize('temperature,scale', [(1.0, 32.0), (0.01, 0.3)])
def test_rows_of_entropy_dd_sum_to_zero(temperature, scale, loss_type):
    """both forms: sum_k p (G - sum p G) = 0 and, for 'argmax', sum_k (one_hot - p) = 1 - 1 = 0 -- the analytic row sum is zero, which
    is why the kernels' dz drops the 2 z rowsum(dd) term"""
    d = R.make_dmat(9, 67, 100, scale)
    dd = R.entropy_dd(d, temperature, RATIO, GLOSS, loss_type, d.argmin(-1))
    assert np.abs(dd.sum(-1)).max() <= 1e-14 * np.abs(dd).sum(-1).max()
    assert np.abs(dd).max() > 0


def test_split_emulation_is_within_2_to_the_minus_15_of_the_exact_products():
    rng = np.random.default_rng(11)
    d = R.make_dmat(11, 128, 128, 0.3)
    dd = R.f32(R.entropy_dd(d, 0.01, RATIO, GLOSS, 'softmax'))
    e, z = R.f32(0.05 * rng.standard_normal((128, 64))), R.f32(0.05 * rng.standard_normal((128, 64)))
    pe, pz = R.split_emulation(dd, e, z)
    assert R.distance(pe, dd @ e) <= 2.0 ** -15
    assert R.distance(pz, dd.T @ z) <= 2.0 ** -15
    assert R.distance(pe, dd @ e) > 0                      # it IS a truncation
    hi = R.bf16(dd)
    assert np.abs(hi + R.bf16(dd - hi) - dd).max() <= 2.0 ** -16 * np.abs(dd).max()
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.3, 0.0])      # ties go to the even significand
    np.testing.assert_array_equal(R.bf16(x), torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).double().numpy())
    np.testing.assert_array_equal(R.bf16_ulp(np.array([1.0, 1.99, 2.0, -0.75])), 2.0 ** np.array([-7.0, -7.0, -6.0, -8.0]))


def test_sequential_float32_sums_differ_from_pairwise():
    x = np.random.default_rng(0).uniform(0.5, 1.5, 5000)
    s = R.seq_sum(x, np.float32)
    acc = np.float32(0)
    for v in x.astype(np.float32):
        acc = np.float32(acc + v)
    assert s.dtype == np.float32 and s == acc
    assert R.seq_sum(x, np.float64) == x.sum()


@pytest.mark.parametrize('n,k,dim,scale', [(67, 68, 16, 1.0), (515, 1000, 64, 0.05), (259, 128, 256, 0.05)])
def test_entropy_maker_leaves_out_no_row_and_plants_the_tie(n, k, dim, scale):
    inp = R.make_entropy_inputs(7, n, k, dim, scale)
    assert inp['rounds'] < R.ROUNDS
    a, b = inp['tie']
    assert a < b and np.array_equal(inp['E'][a], inp['E'][b])
    d = R.entropy_distances(inp['z'], inp['E'])
    assert d[0, a] == d[0, b] == d[0].min() and d[0].argmin() == a
    s = np.sort(np.delete(d, b, axis=1), -1)
    assert ((s[:, 1] - s[:, 0]) >= R.MARGIN * np.maximum(1.0, np.abs(d).max(-1))).all()          # every row, row 0 included
    for key in ('z', 'E', 'dq'):
        assert np.array_equal(inp[key], R.f32(inp[key]))
    again = R.make_entropy_inputs(7, n, k, dim, scale)
    assert all(np.array_equal(inp[key], again[key]) for key in ('z', 'E', 'dq'))
    assert not np.array_equal(inp['z'], R.make_entropy_inputs(8, n, k, dim, scale)['z'])


@pytest.mark.parametrize('n,k,tau', [(3, 5, 1.0), (67, 100, 0.05), (515, 1000, 1.0), (1, 1, 1.0)])
def test_gumbel_maker_leaves_out_no_row_and_plants_the_ties(n, k, tau):
    inp = R.make_gumbel_inputs(7, n, k, tau, ties=[(7, 71), (3, 40)], wide_row=2 if n > 2 else None)
    assert inp['rounds'] < R.ROUNDS
    noise, logits = inp['noise'], inp['logits']
    assert np.isfinite(noise).all() and noise.min() >= np.float32(R.NOISE_MIN) and noise.max() <= R.NOISE_MAX
    assert len(inp['ties']) == sum(b < k for _, b in [(7, 71), (3, 40)])
    t = R.gumbel_t(logits, noise, tau)
    for r, (a, b) in enumerate(inp['ties']):
        assert logits[r, a] == logits[r, b] and noise[r, a] == noise[r, b]
        assert t[r, a] == t[r, b] == t[r].max() and t[r].argmax() == a
        t[r, b] = t[r].min()
    if k > 1:
        s = np.sort(t, -1)
        assert ((s[:, -1] - s[:, -2]) >= R.MARGIN * np.maximum(1.0, np.abs(t).max(-1))).all()
    if n > 2:
        assert noise[2].min() == np.float32(R.NOISE_MIN) and noise[2].max() == R.NOISE_MAX
    again = R.make_gumbel_inputs(7, n, k, tau, ties=[(7, 71), (3, 40)], wide_row=2 if n > 2 else None)
    assert np.array_equal(noise, again['noise']) and np.array_equal(logits, again['logits'])


def test_every_gpu_case_has_a_bound_that_discriminates():
    """the fp32 bound of every quantity of tests/test_gpu_entropy.py and tests/test_gpu_gumbel.py, cases (a) to (e) and row_scale_add,
    from the reference alone (no device; case (b) with the host's float32 distance matrix for the device's): at most 1e-3, so that a
    wrong term, stride or dropped slab (>= 1e-2 in this metric) cannot hide under it.  Not covered (``cpu_bounds`` says why): three
    quantities that are degenerate at any data scale, and the bf16 results of (e), whose bounds come from the number format."""
    from tests import entropy_cases as C
    worst = C.cpu_bounds()
    for name, (b, case) in sorted(worst.items()):
        print(f'ENTMEASURE cpu-bound {name} {b:.3e} at {case}')
    assert worst and all(b <= 1e-3 for b, _ in worst.values()), worst
