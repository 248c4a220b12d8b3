"""float64 numpy reference of the spatially conditioned GroupNorm (csrc/spnorm.hip, ops.spatial_norm), shared by
tests/test_spnorm_cpu.py and tests/test_gpu_spnorm.py:

    u   = GroupNorm_32(f) * gamma + beta        per (sample, group) mean, UNBIASED variance, eps 1e-6
    out = act(u * M[:, :, i // r, j // r] + A[:, :, i // r, j // r])            act: identity or SiLU

forward, the statistics and the closed-form gradients (the algebra of DESIGN 8q), all NCHW float64 arrays, plus the case table,
the input conditioning and the error measures of the GPU test (those of tests/test_gpu_gn_forms.py)."""
import numpy as np
import torch

EPS = 1e-6
BF_EPS = 2.0 ** -8

# N, C, latent h, latent w, r -- what each exercises is said in tests/test_gpu_spnorm.py
CASES = [(2, 64, 4, 4, 1), (1, 32, 3, 5, 2), (2, 96, 4, 4, 2), (3, 512, 2, 3, 4), (2, 128, 2, 2, 16), (1, 128, 1, 1, 8),
         (1, 64, 1, 2, 32)]
UNSERVED = (2, 48, 3, 4, 2)         # 48 channels in 16 groups: the staged route


def case_id(case) -> str:
    n, c, h, w, r = case
    return f'{n}x{c}x{h}x{w}-r{r}'


def make_inputs(case, seed: int = 0) -> dict:
    """float64 torch tensors on the CPU (NCHW): f = randn + 0.5, M = 1 + 0.5 randn, A = 0.5 randn, gamma = 1 + 0.2 randn,
    beta = 0.2 randn, dy = randn"""
    n, c, h, w, r = case
    g = torch.Generator().manual_seed(1000 + seed + n * 7 + c + h * 13 + w * 17 + r * 31)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)         # noqa: E731
    return dict(f=rnd(n, c, h * r, w * r) + 0.5, M=1.0 + 0.5 * rnd(n, c, h, w), A=0.5 * rnd(n, c, h, w),
                gamma=1.0 + 0.2 * rnd(c), beta=0.2 * rnd(c), dy=rnd(n, c, h * r, w * r))


def _up(t, r):
    return t if r == 1 else np.repeat(np.repeat(t, r, axis=2), r, axis=3)


def _block_sum(t, r):
    n, c, hh, ww = t.shape
    return t.reshape(n, c, hh // r, r, ww // r, r).sum(axis=(3, 5))


def _sigmoid(p):
    return 1.0 / (1.0 + np.exp(-p))


def forward(f, M, A, gamma, beta, groups: int = 32, eps: float = EPS, silu: bool = False) -> dict:
    f, M, A, gamma, beta = (np.asarray(t, dtype=np.float64) for t in (f, M, A, gamma, beta))
    n, c, hh, ww = f.shape
    r = hh // M.shape[2]
    assert (M.shape[2] * r, M.shape[3] * r) == (hh, ww) and M.shape == A.shape == (n, c, hh // r, ww // r)
    fg = f.reshape(n, groups, -1)
    m = fg.shape[2]
    mean = fg.mean(axis=2)
    var = ((fg - mean[:, :, None]) ** 2).sum(axis=2) / (m - 1)              # unbiased
    rstd = 1.0 / np.sqrt(var + eps)
    xh = ((fg - mean[:, :, None]) * rstd[:, :, None]).reshape(f.shape)
    u = xh * gamma.reshape(1, c, 1, 1) + beta.reshape(1, c, 1, 1)
    mup, aup = _up(M, r), _up(A, r)
    p = u * mup + aup
    out = p * _sigmoid(p) if silu else p
    return dict(out=out, mean=mean, rstd=rstd, xh=xh, u=u, p=p, mup=mup, r=r, m=m)


def backward(f, M, A, gamma, beta, dy, groups: int = 32, eps: float = EPS, silu: bool = False) -> dict:
    """out, mean, rstd [N, G] and df, dM, dA, dgamma, dbeta"""
    fw = forward(f, M, A, gamma, beta, groups, eps, silu)
    gamma = np.asarray(gamma, dtype=np.float64).reshape(1, -1, 1, 1)
    dy = np.asarray(dy, dtype=np.float64)
    n, c, hh, ww = dy.shape
    r, m, xh, u, p, mup = fw['r'], fw['m'], fw['xh'], fw['u'], fw['p'], fw['mup']
    if silu:
        sg = _sigmoid(p)
        g = dy * sg * (1.0 + p * (1.0 - sg))
    else:
        g = dy
    dA = _block_sum(g, r)
    dM = _block_sum(g * u, r)
    dgamma = (g * mup * xh).sum(axis=(0, 2, 3))
    dbeta = (g * mup).sum(axis=(0, 2, 3))
    dxh = g * mup * gamma
    s1 = dxh.reshape(n, groups, -1).sum(axis=2)
    s2 = (dxh * xh).reshape(n, groups, -1).sum(axis=2)
    cpg = c // groups
    per = lambda t: np.repeat(t, cpg, axis=1).reshape(n, c, 1, 1)           # noqa: E731  [N, G] -> per channel
    df = per(fw['rstd']) * (dxh - per(s1) / m - xh * per(s2) / (m - 1))     # (m - 1): the variance is unbiased
    return dict(out=fw['out'], mean=fw['mean'], rstd=fw['rstd'], df=df, dM=dM, dA=dA, dgamma=dgamma, dbeta=dbeta)


def reference(inp: dict, silu: bool, groups: int = 32) -> dict:
    """:func:`backward` on a dict of torch tensors (any dtype / device: read as float64), results as float64 torch tensors"""
    a = {k: v.detach().double().cpu().numpy() for k, v in inp.items()}
    out = backward(a['f'], a['M'], a['A'], a['gamma'], a['beta'], a['dy'], groups, EPS, silu)
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def literal(inp: dict, silu: bool, groups: int = 32, conv=None) -> dict:
    """float64 torch autograd of the literal formulation: GroupNorm with ``torch.var``, ``F.interpolate(mode='nearest')`` of the
    tables; ``conv``: (zq, Wy, by, Wb, bb) -- the tables are 1x1 convs of zq evaluated at the latent resolution (inp's M / A are
    ignored) and the gradients of all five are returned as well"""
    F = torch.nn.functional
    f, gamma, beta = (inp[k].double().clone().requires_grad_(True) for k in ('f', 'gamma', 'beta'))
    leaves = None
    if conv is None:
        M, A = (inp[k].double().clone().requires_grad_(True) for k in ('M', 'A'))
    else:
        leaves = [t.double().clone().requires_grad_(True) for t in conv]
        zq, wy, by, wb, bb = leaves
        M, A = F.conv2d(zq, wy, by), F.conv2d(zq, wb, bb)
        M.retain_grad()
        A.retain_grad()
    n, c, hh, ww = f.shape
    r = hh // M.shape[2]
    fg = f.reshape(n, groups, -1)
    mean, var = fg.mean(-1, keepdim=True), fg.var(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    u = ((fg - mean) * rstd).reshape(f.shape) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    p = u * F.interpolate(M, scale_factor=r, mode='nearest') + F.interpolate(A, scale_factor=r, mode='nearest')
    out = F.silu(p) if silu else p
    out.backward(inp['dy'].double())
    res = dict(out=out.detach(), mean=mean.detach().reshape(n, groups), rstd=rstd.detach().reshape(n, groups), df=f.grad, dM=M.grad,
               dA=A.grad, dgamma=gamma.grad, dbeta=beta.grad, M=M.detach(), A=A.detach())
    if leaves is not None:
        res['conv_grads'] = [t.grad for t in leaves]
    return res


def relnorm(a, r) -> float:
    return float((a.double().cpu() - r).norm() / (r.norm() + 1e-300))


def errors(bf16: bool, got: dict, ref: dict) -> dict:
    """the measures of tests/test_gpu_gn_forms.py: fp32 out / df: max |got - ref| / max |ref|; bf16 out / df: the worst element in
    units of one bf16 rounding, 2^-8 * (|ref| + mean |ref|), and the relative norm; dM / dA / dgamma / dbeta: relative norm; mean:
    max |got - ref| * rstd_ref; rstd: max relative error"""
    out = {}
    for k in ('out', 'df'):
        if k not in got:
            continue
        a, r = got[k].double().cpu(), ref[k]
        if not bf16:
            out[k] = float((a - r).abs().max() / r.abs().max())
        else:
            out[k] = float(((a - r).abs() / (BF_EPS * (r.abs() + r.abs().mean()))).max())
            out[k + '_rel'] = relnorm(a, r)
    for k in ('dM', 'dA', 'dgamma', 'dbeta'):
        if k in got:
            out[k] = relnorm(got[k], ref[k])
    if 'stats' in got:
        st = got['stats'].double().cpu().view(ref['mean'].shape + (2,))
        out['mean'] = float(((st[..., 0] - ref['mean']).abs() * ref['rstd']).max())
        out['rstd'] = float(((st[..., 1] - ref['rstd']).abs() / ref['rstd']).max())
    return out
