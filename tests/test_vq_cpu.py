"""The standard and EMA quantizers without a GPU: the float64 reference (tests/vq_reference.py) checked against torch.autograd, the
CPU oracle and the goldens of the reference project, the C oracle of the assignment against the acceptance rule, the separation of the
shared inputs, the two readings of ``1 - decay`` -- and the tolerance accounting of tests/test_gpu_vq.py.

TOLERANCES of dz and de.  The base bounds are the project's for these two quantities (tests/test_rot_cpu.py::TOL: dz rtol 1e-5 / atol
1e-7, de rtol 1e-4 / atol 1e-7), applied per element with the atol scaled as ``vq_reference.grad_bounds`` states (the one place).
``RESTATEMENT`` records, per (kind, D) of the GPU tests, the worst error / bound of ``vq_reference.staged_f32`` -- an fp32 torch
evaluation on the CPU, NOT the kernels -- against float64 over the row counts of ``restatement_rows``, dq absent / fp32 / bf16-rounded,
the codebook gradient into a zeroed and into a pre-filled buffer, measured here (test_restatement_error_is_the_recorded_one re-measures
it on every run).  Where that figure exceeds 1 the GPU bound of that (kind, D) is 4 x the figure (``bound_scale``), everywhere else the
stated bound itself.  Every figure is below 0.5 (the largest are single additions into a pre-filled buffer, one
rounding where the bound allows for two): no case is scaled.

1 - DECAY.  ``DECAY_DISTANCE`` records, per tested decay, the relative distance between the kernel's factor (1.0f - fp32(decay)) and the
reference project's (fp32(1 - decay) with the subtraction in double), and the worst error / bound the project's variant would score
against the GPU bound of ``ema_weight`` (3 2^-24 (|decay w| + |(1 - decay) dw|)) on the update cases.  At 0.95 the distance is 2.2e-7 =
3.75 x 2^-24 and the variant scores 1.25 (at 0.99: 9.3e-7 and 5.2): the GPU bound does not absorb the difference, the GPU test has to use ``vq_reference.ema_update``."""
import numpy as np
import pytest
import torch

from oracle import vq_c
from oracle import vqvae_oracle as O
from tests import vq_reference as V

BETA = 0.25
GS = 0.7
TOL = dict(dz=(1e-5, 1e-7), de=(1e-4, 1e-7))                    # (rtol, atol) of tests/test_rot_cpu.py
BWD_D = (8, 24, 264, 1024)                                      # vqk_vq_backward_f32
BWD_N = (1, 300, 16385)
BWD_KINDS = ('scale1', 'onecode', 'spread')
FUSED_N = (1, 31, 33, 2051)                                     # vqk_vq_backward_fused_f32, D = 256
FUSED_KINDS = ('onecode', 'spread', 'collapsed')
DECAYS = (0.0, 0.95, 0.99)
EPS = 1e-5

# worst error / bound of staged_f32 against float64 (dz and de together).  Measured on the CPU.
RESTATEMENT = {
    ('scale1', 8): 0.114, ('scale1', 24): 0.15, ('scale1', 264): 0.238, ('scale1', 1024): 0.402, ('scale1', 64): 0.0954, ('scale1', 256): 0.122,
    ('onecode', 8): 0.246, ('onecode', 24): 0.257, ('onecode', 264): 0.198, ('onecode', 1024): 0.348, ('onecode', 256): 0.184,
    ('spread', 8): 0.462, ('spread', 24): 0.475, ('spread', 264): 0.455, ('spread', 1024): 0.483, ('spread', 256): 0.483,
    ('collapsed', 256): 0.147,
}
# decay -> (relative distance of the two (1 - decay) factors, worst error / GPU bound of the project's variant of ema_weight)
DECAY_DISTANCE = {0.0: (0.0, 0.0), 0.95: (2.235e-7, 1.25), 0.99: (9.313e-7, 5.21)}


def bound_scale(kind: str, d: int) -> float:
    """factor on the GPU bounds of dz and de: 1, or 4 x the restatement's own figure where that exceeds 1"""
    r = RESTATEMENT[(kind, d)]
    return 4.0 * r if r > 1.0 else 1.0


def bwd_k(n: int, kind: str) -> int:
    """codes of a backward case: spread needs one code per row"""
    return {'scale1': 64, 'collapsed': 64, 'onecode': 16}.get(kind, max(n, 2))


def bwd_case(n: int, d: int, kind: str):
    """(z, e, idx) of a backward case: the kernels take the indices as an input (the planted ones / the float64 argmin)"""
    k = bwd_k(n, kind)
    z, e = V.make_case(n, k, d, kind)
    return z, e, V.planted(n, k, d, kind)


def upstream(n: int, d: int, name: str):
    """dq of a backward case: None, fp32 randn, or the same rounded to bf16"""
    if name == 'none':
        return None
    dq = torch.randn(n, d, generator=torch.Generator().manual_seed(11))
    return dq.to(torch.bfloat16) if name == 'bf16' else dq


def prefill_like(e, ce: float):
    """what an optimizer arena may hold when the kernel adds into it: random values at the scale of the gradient"""
    return (torch.randn(e.shape, generator=torch.Generator().manual_seed(13)) * ce).float()


def restatement_rows(kind: str, d: int):
    """row counts the restatement is measured at: every N of the GPU tests, the 16385-row cases at the two narrow widths only (the
    float64 side of 16385 x 1024 elements per variant adds minutes, not information)"""
    if kind == 'scale1' and d in (64, 256):
        return tuple(s[0] for s in V.LOOKUP_SHAPES if s[2] == d)
    if d == 256:
        return FUSED_N
    return BWD_N if d <= 24 else BWD_N[:2]


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('ema', [False, True], ids=['standard', 'ema'])
@pytest.mark.parametrize('kind,with_dq', [('scale1', True), ('init', True), ('collapsed', True), ('onecode', True), ('scale1', False)])
def test_closed_form_gradients_match_autograd(kind, with_dq, ema):
    n, k, d = 23, 16, 8
    z, e = V.make_case(n, k, d, kind)
    idx = V.forward(z, e)['idx']
    if kind == 'collapsed':
        assert int(idx.max()) < 4
    dq = upstream(n, d, 'fp32' if with_dq else 'none')
    cz, ce = V.coefficients(n, d, BETA)
    dz, de = V.gradients(z, e, idx, dq, cz, ce, GS)
    loss, a_dz, a_de = V.autograd_gradients(z, e, idx, dq, BETA, GS, ema)
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp_min(1e-300))[b != 0].max())
    print(f'VQMEASURE closed forms against autograd {kind} ema {int(ema)}: dz {rel(dz, a_dz):.3e}' + ('' if ema else f', de {rel(de, a_de):.3e}'))
    assert rel(dz, a_dz) <= 1e-12
    np.testing.assert_allclose(loss.item(), V.quantities(z, e, idx, BETA, ema)['loss'].item(), rtol=1e-12)
    if not ema:
        assert rel(de, a_de) <= 1e-12
        unused = V.hist(idx, k) == 0
        assert bool(unused.any()) and float(de[unused].abs().max()) == 0.0 and float(a_de[unused].abs().max()) == 0.0


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize('tag', ['std_a', 'std_b', 'std_c'])
def test_forward_agrees_with_the_oracle_on_the_standard_goldens(golden, tag):
    g = golden('vq')
    z4, e = torch.from_numpy(g[f'{tag}.z']), torch.from_numpy(g[f'{tag}.e'])
    z = _rows(z4).contiguous()
    n, d = z.shape
    f = V.forward(z, e)
    q_o, idx_o, loss_o = O.vq_standard(z4, e, BETA)
    assert torch.equal(f['idx'], idx_o.reshape(-1)) and np.array_equal(f['idx'].numpy(), g[f'{tag}.idx'].reshape(-1))
    V.check_acceptance(z, e, f['idx'])
    fq = V.quantities(z, e, f['idx'], BETA)
    np.testing.assert_allclose(fq['q'].numpy(), _rows(torch.from_numpy(g[f'{tag}.q'])).numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(fq['loss'].item(), loss_o.item(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(fq['loss'].item(), g[f'{tag}.loss'], rtol=1e-5, atol=1e-6)
    dq = _rows(torch.from_numpy(g[f'{tag}.dq']))
    dz, de = V.gradients(z, e, f['idx'], dq, *V.coefficients(n, d, BETA))
    np.testing.assert_allclose(dz.numpy(), _rows(torch.from_numpy(g[f'{tag}.dz'])).numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(de.numpy(), g[f'{tag}.de'], rtol=1e-5, atol=1e-6)


def test_forward_and_update_agree_with_the_oracle_on_the_ema_trajectory(golden):
    g = golden('vq')
    T = torch.from_numpy
    cb, cnt, w = T(g['ema.e0']), T(g['ema.c0']), T(g['ema.w0'])
    cb64, cnt64, w64 = cb.double(), cnt.double(), w.double()
    for s in range(3):
        z4 = T(g[f'ema.z{s}'])
        z = _rows(z4).contiguous()
        n, d = z.shape
        f = V.forward(z, cb64.float())
        _, idx_o, loss_o, cnt, w, cb = O.vq_ema(z4, cb, cnt, w, BETA, 0.95, EPS)
        assert np.array_equal(f['idx'].numpy(), g[f'ema.idx{s}'].reshape(-1))
        fq = V.quantities(z, cb64.float(), f['idx'], BETA, ema=True)
        np.testing.assert_allclose(fq['loss'].item(), g[f'ema.loss{s}'], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(fq['loss'].item(), loss_o.item(), rtol=1e-5, atol=1e-6)
        dz, _ = V.gradients(z, cb64.float(), f['idx'], _rows(T(g[f'ema.dq{s}'])), *V.coefficients(n, d, BETA))
        np.testing.assert_allclose(dz.numpy(), _rows(T(g[f'ema.dz{s}'])).numpy(), rtol=1e-5, atol=1e-6)
        counts, dw, _ = V.ema_stats(z, f['idx'], cb.shape[0])
        for fn in (V.ema_update, V.ema_update_project):
            u = fn(cnt64, w64, counts, dw, 0.95, EPS, float(z4.shape[0]))
            np.testing.assert_allclose(u['count'].numpy(), g[f'ema.count{s}'], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(u['weight'].numpy(), g[f'ema.weight{s}'], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(u['codebook'].numpy(), g[f'ema.cb{s}'], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(u['codebook'].numpy(), cb.numpy(), rtol=1e-5, atol=1e-6)
        u = V.ema_update(cnt64, w64, counts, dw, 0.95, EPS, float(z4.shape[0]))
        # (the next step ranks against the golden's fp32 codebook, as the oracle does: the trajectories cannot drift apart)
        cb64, cnt64, w64 = T(g[f'ema.cb{s}']).double(), u['count'], u['weight']


@pytest.mark.parametrize('assoc', [0, 1])
@pytest.mark.parametrize('kind', V.ASSIGN_KINDS)
@pytest.mark.parametrize('shape', V.ASSIGN_SHAPES + V.LOOKUP_SHAPES, ids=str)
def test_c_oracle_meets_the_acceptance_rule(shape, kind, assoc):
    """the canonical-order fp32 assignment (oracle/vq_oracle.c) judged as the kernels will be: the rule is one an exact fp32
    evaluation passes at every width, 1264 included"""
    n = min(shape[0], 300)                                         # (the scalar oracle: ~0.5 ms per row against 1024 x 256 codes)
    z, e = V.make_case(*shape, kind)
    idx, _, z2, e2 = vq_c.assign(z[:n].numpy(), e.numpy(), assoc)
    idx = torch.from_numpy(idx)
    sep = V.check_acceptance(z[:n], e, idx, assoc)
    inv, first_of = V.first_of_class(e)
    assert torch.equal(idx, first_of[inv[idx]])                    # the lowest of bitwise-equal rows
    d = shape[2]
    for x, x2 in ((z[:n], z2), (e, e2)):                           # the row norms' bound of the GPU test holds for the canonical order
        want = (x.double() ** 2).sum(1)
        assert bool(((torch.from_numpy(x2).double() - want).abs() <= d * 2.0 ** -24 * want).all())
    print(f'VQMEASURE C oracle {shape} {kind} assoc {assoc}: separated {sep:.4f}')


# ---------------------------------------------------------------------------------------------- the shared inputs
# vq_reference.SEED = 9, the first of 1 .. 15 to meet the condition on every shape (9 and 12 do).  Measured share of separated rows, the
# smaller of the two associations: 1.0 on every shape but (2051, 1024, 256): 0.9922 and (2048, 64, 256): 0.9961.


@pytest.mark.parametrize('shape', V.ASSIGN_SHAPES + V.LOOKUP_SHAPES, ids=str)
def test_inputs_are_separated(shape):
    z, e = V.make_case(*shape, 'scale1')
    f = V.reference(*shape, 'scale1')
    for assoc in (0, 1):
        t = V.teacher_forced(z, e, f['idx'], assoc)
        sep = float((t['gap'] > t['eta2']).double().mean())
        print(f'VQMEASURE seed {V.SEED} {shape} assoc {assoc}: separated rows {sep:.4f}')
        assert sep >= 0.99
        assert torch.equal(t['argmin'], f['idx'])


@pytest.mark.parametrize('kind', ['onecode', 'spread'])
def test_planted_indices_are_the_float64_argmin(kind):
    for n, k, d in ((1, 2, 8), (33, 64, 256), (300, 300, 24), (300, 16, 8) if kind == 'onecode' else (300, 300, 8), (16, 16, 1024)):
        z, e = V.make_case(n, k, d, kind)
        idx = V.planted(n, k, d, kind)
        assert torch.equal(V.forward(z, e)['idx'], idx)
        if kind == 'spread':
            assert len(set(idx.tolist())) == n
    z, idx = V.ema_case(777, 8, 300, 'mixed')
    assert not bool((idx == 1).any()) and float(z.abs().max()) > 100.0 and float(z.abs().min()) < 1e-3
    assert int(V.reference(33, 40, 8, 'collapsed')['idx'].max()) < 4


# ---------------------------------------------------------------------------------------------- the fp32 restatement
def _ratio(got, want, allowed):
    err = (got.double() - want).abs()
    return float((err / allowed.clamp_min(1e-300))[err > 0].max()) if bool((err > 0).any()) else 0.0


@pytest.mark.parametrize('key', sorted(RESTATEMENT), ids=str)
def test_restatement_error_is_the_recorded_one(key):
    kind, d = key
    worst = 0.0
    for n in restatement_rows(kind, d):
        if d in (64, 256) and kind == 'scale1':
            z, e = V.make_case(n, 64, d, kind)
            idx = V.reference(n, 64, d, kind)['idx']
        else:
            z, e, idx = bwd_case(n, d, kind)
        cz, ce = V.coefficients(z.shape[0], d, BETA)
        pre = prefill_like(e, ce)
        for name in ('none', 'fp32', 'bf16'):
            dq = upstream(z.shape[0], d, name)
            dq = None if dq is None else dq.float()
            dz, de = V.gradients(z, e, idx, dq, cz, ce, GS)
            s = V.staged_f32(z, e, dq, cz, ce, GS, idx=idx)
            dz_a, de_a = V.grad_bounds(z, e, idx, dz, de, cz, ce, GS, TOL)
            worst = max(worst, _ratio(s['dz'], dz, dz_a), _ratio(s['de'], de, de_a))
            _, de_p = V.grad_bounds(z, e, idx, dz, de + pre.double(), cz, ce, GS, TOL, prefill=pre)
            worst = max(worst, _ratio(pre + s['de'], de + pre.double(), de_p))
    print(f'VQMEASURE restatement {key}: {worst:.4g} (recorded {RESTATEMENT[key]}), bound scale {bound_scale(*key):.3g}')
    # the table is no understatement of what this loop measures (the host's summation order may move the worst element)
    assert worst <= 2.0 * RESTATEMENT[key]
    assert bound_scale(*key) <= 8.0


def test_restatement_table_covers_the_gpu_cases():
    want = {(k, d) for k in BWD_KINDS for d in BWD_D} | {(k, 256) for k in FUSED_KINDS} | {('scale1', s[2]) for s in V.LOOKUP_SHAPES}
    assert want == set(RESTATEMENT)
    assert all(bound_scale(*key) == 1.0 for key in RESTATEMENT)


# ---------------------------------------------------------------------------------------------- the two readings of 1 - decay
def update_case(k: int, d: int, n: int = 4096):
    """(ema_count, ema_weight, counts, dw) of an update case: a quarter of the codes without rows (counts = 0, dw = 0), a quarter of the
    running counts at zero"""
    g = torch.Generator().manual_seed(17 + k + d)
    counts = torch.randint(0, 2 * max(n // k, 2), (k,), generator=g).float()
    counts[torch.rand(k, generator=g) < 0.25] = 0.0
    if k > 1:
        counts[0] = 0.0
    dw = torch.randn(k, d, generator=g) * counts.sqrt()[:, None]
    c = torch.rand(k, generator=g) * 8.0
    c[torch.rand(k, generator=g) < 0.25] = 0.0
    if k > 1:
        c[0] = 0.0
    return c, torch.randn(k, d, generator=g), counts, dw


def test_decay_factor_distance_is_the_recorded_one():
    for decay in DECAYS:
        kernel = float(np.float32(1.0) - np.float32(decay))
        project = float(np.float32(1.0 - decay))
        dist = abs(kernel - project) / project
        worst = 0.0
        for k, d in ((1, 8), (257, 8), (1000, 256)):
            c, w, counts, dw = update_case(k, d)
            a = V.ema_update(c, w, counts, dw, decay, EPS, 4.0)
            b = V.ema_update_project(c, w, counts, dw, decay, EPS, 4.0)
            bound = 3.0 * 2.0 ** -24 * (a['wa'] + a['wb'])
            worst = max(worst, _ratio(b['weight'], a['weight'], bound))
        rec = DECAY_DISTANCE[decay]
        print(f'VQMEASURE decay {decay}: |1.0f - decay_f32| against fp32(1 - decay) relative {dist:.3e} (recorded {rec[0]}), the project\'s '
              f'ema_weight against the GPU bound {worst:.3g} (recorded {rec[1]})')
        assert abs(dist - rec[0]) <= 0.01 * rec[0] and abs(worst - rec[1]) <= 0.05 * rec[1]
    assert DECAY_DISTANCE[0.95][1] > 1.0                               # not absorbed: the GPU test must take the kernel's reading
