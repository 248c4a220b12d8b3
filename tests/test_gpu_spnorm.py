"""The spatially conditioned GroupNorm kernels (csrc/spnorm.hip, ops.spatial_norm) against the float64 reference of
tests/spnorm_reference.py on the inputs as the kernel sees them (bf16 mode: the bf16-rounded f and dy), both dtypes, SiLU on and off,
dgamma / dbeta accumulated onto non-zero values (a kernel that stores instead of adding fails).

Cases (N, C, latent h x w, r):
  2, 64, 4x4, 1      r = 1: one map pixel per latent pixel, `teams` latent pixels side by side in a block
  1, 32, 3x5, 2      one channel per group, ragged non-square map
  2, 96, 4x4, 2      3 channels per group, 24 / 12 vector slots per pixel: not every thread of a block owns a slot
  3, 512, 2x3, 4     widest channel count: two channels per thread in the channel sums
  2, 128, 2x2, 16    the full-resolution head: a 16x16 block per latent pixel, several vectors per thread
  1, 128, 1x1, 8     a single latent pixel
  1, 64, 1x2, 32     largest ratio: 1024 map pixels per latent pixel
  2, 48, 3x4, 2 in 16 groups: not served -- must take the staged route and agree
Inputs: f = randn + 0.5, M = 1 + 0.5 randn, A = 0.5 randn, gamma = 1 + 0.2 randn, beta = 0.2 randn; every group has at least 32
elements, the function is smooth: no case is excluded, no element masked.

Error measures (tests/spnorm_reference.py::errors, those of tests/test_gpu_gn_forms.py): fp32 out / df: max |got - ref| / max |ref|;
bf16 out / df: the worst element in units of one bf16 rounding, 2^-8 * (|ref| + mean |ref|), and the relative norm; dM / dA / dgamma
/ dbeta: relative norm; mean: max |got - ref| * rstd_ref; rstd: max relative error.

Measured worst errors over the cases on MI355X and the bounds (_BOUNDS: about 10x the worst; the bf16 per-element rule is fixed at
one rounding):
            measure            fused kernels   staged route   worst     bound
  fp32      out                1.8e-7          1.8e-7         1.8e-7    2e-6
            df                 3.0e-7          2.3e-7         3.0e-7    3e-6
            dM / dA            1.2e-7 / 1.0e-7 3.0e-7 / 3.0e-7 3.0e-7   3e-6
            dgamma / dbeta     1.3e-7 / 1.0e-7 1.4e-7 / 1.5e-7 1.5e-7   1.5e-6
            mean / rstd        3.7e-8 / 6.6e-8 -              -         4e-7 / 7e-7
  bf16      out, df            0.91, 0.94      0.91, 0.90     0.94      1 rounding (relative norm 1.7e-3; 3e-3 as for GroupNorm: the
                                                                        statistics of one bf16 rounding, not a summation error)
            dM / dA            1.1e-7 / 1.0e-7 3.0e-7 / 3.1e-7 3.1e-7   3e-6
            dgamma / dbeta     1.3e-7 / 1.1e-7 1.5e-7 / 1.5e-7 1.5e-7   1.5e-6
            mean / rstd        3.1e-8 / 6.8e-8 -              -         3e-7 / 7e-7
Every measured value lies below the plain GroupNorm's bound for the same measure (2e-6 y, 5e-6 dx / dW in fp32): nothing to explain.
The staged route's dM / dA are the larger ones at r = 16 (torch sums the 256 upsampled cotangents in fp32; the kernels add fp32 runs
of 16 terms in double).  One set of bounds serves both routes.
"""
import contextlib
import functools
import importlib

import pytest
import torch

from tests import spnorm_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
spn = importlib.import_module(PKG + '._ops_spnorm')
DEV, F32, BF, CL = 'cuda:0', torch.float32, torch.bfloat16, torch.channels_last
DTYPES = [F32, BF]
DT_ID = {F32: 'fp32', BF: 'bf16'}

_BOUNDS = {
    F32: dict(out=2e-6, df=3e-6, dM=3e-6, dA=3e-6, dgamma=1.5e-6, dbeta=1.5e-6, mean=4e-7, rstd=7e-7),
    BF: dict(out=1.0, out_rel=3e-3, df=1.0, df_rel=3e-3, dM=3e-6, dA=3e-6, dgamma=1.5e-6, dbeta=1.5e-6, mean=3e-7, rstd=7e-7),
}


@functools.lru_cache(maxsize=None)
def _problem(case, dt, silu):
    """(device inputs as the kernel sees them, float64 reference on exactly those) -- computed once, shared, never modified"""
    groups = 16 if case == R.UNSERVED else 32
    raw = R.make_inputs(case)
    inp = {k: v.to(DEV, F32) for k, v in raw.items()}
    for k in ('f', 'dy'):
        inp[k] = inp[k].to(dt).contiguous(memory_format=CL)
    for k in ('M', 'A'):
        inp[k] = inp[k].contiguous(memory_format=CL)
    return inp, R.reference(inp, silu, groups)


def _prefill(c, seed):
    return torch.randn(c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _run_raw(inp, silu):
    """the launchers of the autograd Function, dgamma / dbeta added onto non-zero values"""
    c = inp['f'].shape[1]
    out, stats = ops.raw_spnorm_forward(inp['f'], inp['M'], inp['A'], inp['gamma'], inp['beta'], R.EPS, silu)
    dg0, db0 = _prefill(c, 1), _prefill(c, 2)
    dg, db = dg0.clone(), db0.clone()
    df, dm, da, _, _ = ops.raw_spnorm_backward(inp['f'], stats, inp['M'], inp['A'], inp['gamma'], inp['beta'], inp['dy'], silu, dg, db)
    torch.cuda.synchronize()
    return dict(out=out, stats=stats, df=df, dM=dm, dA=da, dgamma=dg.double() - dg0.double(), dbeta=db.double() - db0.double(),
                dgamma_raw=dg, dbeta_raw=db)


def _run_autograd(inp, silu, groups=32):
    """ops.spatial_norm under autograd, the GroupNorm affine in its module shape [1, C, 1, 1]"""
    t = {k: v.detach().clone().requires_grad_(k != 'dy') for k, v in inp.items()}
    out = ops.spatial_norm(t['f'], t['M'], t['A'], t['gamma'].view(1, -1, 1, 1), t['beta'].view(1, -1, 1, 1), groups, R.EPS, silu)
    out.backward(t['dy'])
    torch.cuda.synchronize()
    return dict(out=out.detach(), df=t['f'].grad, dM=t['M'].grad, dA=t['A'].grad, dgamma=t['gamma'].grad, dbeta=t['beta'].grad)


def _check_all(tag, dt, got, ref):
    fig = R.errors(dt == BF, got, ref)
    print(f'SPNMEASURE gpu {tag} {DT_ID[dt]} ' + ' '.join(f'{k} {v:.2e}' for k, v in fig.items()))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    for k, v in fig.items():
        assert v < _BOUNDS[dt][k], (tag, k, v, _BOUNDS[dt][k])


@contextlib.contextmanager
def _deterministic(on):
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(False)


# ---------------------------------------------------------------------------------------------- 1. the kernels against float64
@pytest.mark.parametrize('silu', [False, True], ids=['id', 'silu'])
@pytest.mark.parametrize('dt', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_fused_matches_fp64(case, dt, silu):
    inp, ref = _problem(case, dt, silu)
    assert ops.spnorm_fused_serves(inp['f'], inp['M'])
    got = _run_raw(inp, silu)
    assert got['out'].dtype == dt and got['df'].dtype == dt and got['dM'].dtype == F32 and got['dA'].shape == inp['A'].shape
    assert got['out'].is_contiguous(memory_format=CL) and got['dM'].is_contiguous(memory_format=CL)
    _check_all(f'fused {R.case_id(case)} {"silu" if silu else "id"}', dt, {k: v for k, v in got.items() if not k.endswith('_raw')}, ref)


# ---------------------------------------------------------------------------------------------- 2. the routes
@pytest.mark.parametrize('silu', [False, True], ids=['id', 'silu'])
@pytest.mark.parametrize('dt', DTYPES, ids=DT_ID.get)
def test_unserved_shape_takes_the_staged_route(dt, silu, monkeypatch):
    inp, ref = _problem(R.UNSERVED, dt, silu)
    assert not ops.spnorm_fused_serves(inp['f'], inp['M'], 16)

    def refuse(*a, **k):
        raise AssertionError('the fused kernels were launched on a shape they do not serve')
    monkeypatch.setattr(spn, 'raw_spnorm_forward', refuse)
    got = _run_autograd(inp, silu, groups=16)
    assert got['out'].dtype == dt
    _check_all(f'staged-unserved {R.case_id(R.UNSERVED)} {"silu" if silu else "id"}', dt, got, ref)


@pytest.mark.parametrize('silu', [False, True], ids=['id', 'silu'])
@pytest.mark.parametrize('dt', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('case', [R.CASES[1], R.CASES[2], R.CASES[4]], ids=R.case_id)
def test_fused_and_staged_routes_agree(case, dt, silu, monkeypatch):
    """both routes of ops.spatial_norm under autograd, each inside the bounds of the float64 reference (``ops.SPNORM_FUSED`` selects);
    in fp32 the two also lie within two bounds of each other"""
    inp, ref = _problem(case, dt, silu)
    calls = []
    real = spn.raw_spnorm_forward
    monkeypatch.setattr(spn, 'raw_spnorm_forward', lambda *a: (calls.append(1), real(*a))[1])
    fused = _run_autograd(inp, silu)
    assert len(calls) == 1
    monkeypatch.setattr(ops, 'SPNORM_FUSED', False)
    staged = _run_autograd(inp, silu)
    assert len(calls) == 1
    _check_all(f'route-fused {R.case_id(case)} {"silu" if silu else "id"}', dt, fused, ref)
    _check_all(f'route-staged {R.case_id(case)} {"silu" if silu else "id"}', dt, staged, ref)
    if dt == F32:
        fig = R.errors(False, fused, {k: v.double().cpu() for k, v in staged.items()})
        print(f'SPNMEASURE gpu fused-vs-staged {R.case_id(case)} ' + ' '.join(f'{k} {v:.2e}' for k, v in fig.items()))
        assert all(v < 2 * _BOUNDS[F32][k] for k, v in fig.items()), fig


# ---------------------------------------------------------------------------------------------- 3. the same bits on every run
@pytest.mark.parametrize('deterministic', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('dt', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[3], R.CASES[4], (4, 128, 16, 16, 2)], ids=R.case_id)
def test_two_runs_are_bit_equal(case, dt, deterministic):
    """no float atomics, fixed summation order: forward + backward twice give the same bits, in default and deterministic mode (one
    code path: the mode changes nothing).  The last case has 64 blocks per sample and several segments in the channel finish."""
    inp, _ = _problem(case, dt, True)
    with _deterministic(deterministic):
        a = _run_raw(inp, True)
        b = _run_raw(inp, True)
    for k in ('out', 'stats', 'df', 'dM', 'dA', 'dgamma_raw', 'dbeta_raw'):
        assert torch.equal(a[k], b[k]), k
    if deterministic:
        c = _run_raw(inp, True)
        assert all(torch.equal(a[k], c[k]) for k in ('out', 'stats', 'df', 'dM', 'dA', 'dgamma_raw', 'dbeta_raw'))


def test_larger_map_matches_fp64():
    """4 x 128 @ 32x32 from 16x16 latents (r = 2): 64 blocks per sample, four segments in the channel finish, block partials of
    every kind added in order"""
    for dt in DTYPES:
        inp, ref = _problem((4, 128, 16, 16, 2), dt, True)
        got = _run_raw(inp, True)
        _check_all('fused 4x128x16x16-r2 silu', dt, {k: v for k, v in got.items() if not k.endswith('_raw')}, ref)


# ---------------------------------------------------------------------------------------------- 4. the autograd Function
def test_direct_gradients_accumulate_into_the_arena():
    """what FlatAdamW does to its parameters: a gradient the kernels add into; the Function then returns None for gamma / beta"""
    inp, ref = _problem(R.CASES[2], F32, True)
    gamma = inp['gamma'].clone().view(1, -1, 1, 1).requires_grad_(True)
    beta = inp['beta'].clone().view(1, -1, 1, 1).requires_grad_(True)
    pre = {}
    for name, p in (('dgamma', gamma), ('dbeta', beta)):
        p.grad = _prefill(p.numel(), 7).view_as(p).clone()
        pre[name] = p.grad.clone()
        p._vqk_direct_grad = True
    f = inp['f'].clone().requires_grad_(True)
    out = ops.spatial_norm(f, inp['M'], inp['A'], gamma, beta, 32, R.EPS, True)
    out.backward(inp['dy'])
    torch.cuda.synchronize()
    got = dict(out=out.detach(), df=f.grad, dgamma=(gamma.grad.double() - pre['dgamma'].double()).view(-1),
               dbeta=(beta.grad.double() - pre['dbeta'].double()).view(-1))
    _check_all('direct', F32, got, ref)
    with ops.no_direct_grad():
        g2, = ops.autograd_grad(ops.spatial_norm(f, inp['M'], inp['A'], gamma, beta, 32, R.EPS, True), [gamma], inp['dy'])
    assert g2.shape == gamma.shape and R.relnorm(g2.view(-1), ref['dgamma']) < _BOUNDS[F32]['dgamma']


def test_captures_into_a_graph():
    """workspaces come from torch's allocator, no host synchronisation: forward + backward capture and replay to the eager bits"""
    inp, _ = _problem(R.CASES[4], BF, True)
    eager = _run_raw(inp, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run_raw(inp, True)                                                   # settle lazy state on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    c = inp['f'].shape[1]
    dg, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    with torch.cuda.graph(g, stream=side):
        out, stats = ops.raw_spnorm_forward(inp['f'], inp['M'], inp['A'], inp['gamma'], inp['beta'], R.EPS, True)
        df, dm, da, _, _ = ops.raw_spnorm_backward(inp['f'], stats, inp['M'], inp['A'], inp['gamma'], inp['beta'], inp['dy'], True, dg, db)
    for _ in range(2):
        dg.zero_()
        db.zero_()
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager['out']) and torch.equal(df, eager['df']) and torch.equal(dm, eager['dM']) and torch.equal(da, eager['dA'])
    # (the eager sums were added onto O(1) values and taken back: one fp32 rounding of those, relative to sums of O(10) and more)
    assert R.relnorm(dg, eager['dgamma'].cpu()) < 1e-5 and R.relnorm(db, eager['dbeta'].cpu()) < 1e-5
