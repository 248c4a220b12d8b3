"""Float64 reference of the cosine quantizer (include/vqk.h, "cosine quantizer"; no GPU):

    nrm(x) = x / max(|x|, eps), eps = 1e-12;  zn = nrm(z), en = nrm(e);
    idx = argmin_k (|zn|^2 + |en_k|^2) - 2 zn.en_k  (first minimum);  q = en[idx];  sse = sum |q - zn|^2;
    loss = (1 + beta) / (N D) sse  (codebook term |sg(zn) - en|^2 + beta * commitment term |zn - sg(en)|^2);
    g = dq + s cz (zn - q);  dz = (g - zn (zn.g)) inv_z;  de[k] = s ce inv_e[k] sum_{rows: idx = k} (en_k (en_k.zn) - zn),
    cz = 2 beta / (N D), ce = 2 / (N D)  (the straight-through estimator is taken at zn; a clamped row has the Jacobian I / eps).

``forward`` runs free (its own argmin), ``teacher_forced`` / ``check_acceptance`` judge GIVEN indices on the float64-normalised rows,
``gradients`` are the closed forms, ``autograd_gradients`` the same through torch.autograd with the estimator written out.
``staged_f32`` restates the staged formulation (ops.cos_staged and its backward) in fp32 torch for the CPU.
``cases`` / ``make_case`` are the inputs of tests/test_gpu_cos.py, shared with tests/test_cos_cpu.py; results are cached per case."""
import functools

import torch

from tests import rvq_reference

EPS = 1e-12
# (N, K, D) of the GPU tests: one row; a ragged block; two code tiles; several blocks and tiles; the widest served row; many codes in few
# dimensions (near-ties densest)
SHAPES = [(1, 32, 8), (67, 32, 8), (67, 64, 16), (2051, 1024, 32), (67, 2048, 64), (2051, 8192, 8)]
KINDS = ['scale1', 'init', 'collapsed', 'zero']
SEED = 3                # tests/test_cos_cpu.py::test_inputs_are_separated: >= 99 % of the scale-1 rows separated by > 2 eta


def eta(z_norm=1.0, e_norm=1.0):
    """evaluation bound of the exact fp32 ranking at unit norms: rvq_reference.eta(1, 1) = 2^-13 + 2^-20"""
    return rvq_reference.eta(z_norm, e_norm)


@functools.lru_cache(maxsize=None)
def make_case(n: int, k: int, d: int, kind: str):
    """(z [N, D], e [K, D]) fp32 tensors.  scale1 / init: normal codebook of scale 1 / 1/K (the initialisation scale); collapsed: every
    code row a copy of one of 4 distinct rows (exact ties: the smallest index must win); zero: row 3 of e and row 0 of z are the zero
    vector (the clamped branch of the normalisation)."""
    g = torch.Generator().manual_seed(SEED + 7919 * n + 31 * k + d + 1009 * KINDS.index(kind))
    z = torch.randn(n, d, generator=g, dtype=torch.float32)
    e = torch.randn(k, d, generator=g, dtype=torch.float32)
    if kind == 'init':
        e = e / float(k)
    elif kind == 'collapsed':
        e = e[:4][torch.arange(k) % 4].contiguous()
    elif kind == 'zero':
        e[3] = 0.0
        z[0] = 0.0
    elif kind != 'scale1':
        raise ValueError(kind)
    return z, e


def cases():
    return [(n, k, d, kind) for (n, k, d) in SHAPES for kind in KINDS]


def nrm(x):
    """(xn, inv) in the dtype of x"""
    inv = 1.0 / x.norm(dim=1).clamp_min(EPS)
    return x * inv[:, None], inv


def clamped(x):
    """rows the normalisation clamps (|x| < eps)"""
    return x.double().norm(dim=1) < EPS


def _dist64(zn, en):
    return (zn * zn).sum(1, keepdim=True) + (en * en).sum(1)[None, :] - 2.0 * (zn @ en.T)


def _first_of_class(e):
    """per code: the first index among the bitwise-equal rows of e (equal rows normalise to equal rows)"""
    _, inv = torch.unique(e, dim=0, return_inverse=True)
    first_of = torch.full((int(inv.max()) + 1,), e.shape[0], dtype=torch.int64)
    first_of.scatter_reduce_(0, inv, torch.arange(e.shape[0]), reduce='amin')
    return inv, first_of


def forward(z, e):
    """free-running float64 forward: idx [N] (first minimum), zn, en, q, sse"""
    zn, en = nrm(z.double())[0], nrm(e.double())[0]
    d = _dist64(zn, en)
    inv, first_of = _first_of_class(e)
    idx = first_of[inv[d.argmin(1)]]
    q = en[idx]
    return dict(idx=idx, zn=zn, en=en, q=q, sse=((q - zn) ** 2).sum())


def teacher_forced(z, e, idx):
    """every row on the float64-normalised operands: chosen = D64(idx), best = min_k D64, argmin (first of bitwise-equal rows),
    gap = the distance from best to the nearest code that is not a bitwise copy of the best row (inf if none).  All [N]."""
    zn, en = nrm(z.double())[0], nrm(e.double())[0]
    d = _dist64(zn, en)
    inv, first_of = _first_of_class(e)
    best, arg = d.min(1)
    arg = first_of[inv[arg]]
    other = d.masked_fill(inv[None, :] == inv[arg][:, None], float('inf'))
    return dict(chosen=d[torch.arange(z.shape[0]), idx], best=best, argmin=arg, gap=other.min(1).values - best)


def check_acceptance(z, e, idx):
    """the chosen code's float64 distance is within 2 eta of the float64 minimum, and where the runner-up is more than 2 eta away the
    index IS the float64 argmin (first of bitwise-equal rows).  Returns the fraction of separated rows."""
    t = teacher_forced(z, e, idx)
    eta2 = 2.0 * eta()
    excess = t['chosen'] - t['best']
    bad = excess > eta2
    assert not bool(bad.any()), f'{int(bad.sum())} rows beyond 2 eta, worst excess / (2 eta) = {float((excess / eta2).max()):.3g}'
    sep = t['gap'] > eta2
    wrong = sep & (idx != t['argmin'])
    assert not bool(wrong.any()), f'{int(wrong.sum())} separated rows off the float64 argmin'
    return float(sep.double().mean())


def gradients(z, e, idx, dq, beta: float, s: float = 1.0):
    """closed forms on the given indices: (loss, sse, dz [N, D], de [K, D]) in float64; dq may be None"""
    (zn, inv_z), (en, inv_e) = nrm(z.double()), nrm(e.double())
    n, d = z.shape
    q = en[idx]
    sse = ((q - zn) ** 2).sum()
    loss = (1.0 + beta) / (n * d) * sse
    cz, ce = 2.0 * beta / (n * d), 2.0 / (n * d)
    g = s * cz * (zn - q) + (dq.double() if dq is not None else 0.0)
    dz = (g - zn * (zn * g).sum(1, keepdim=True)) * inv_z[:, None]
    rows = q * (q * zn).sum(1, keepdim=True) - zn
    de = torch.zeros(e.shape, dtype=torch.float64).index_add_(0, idx, rows) * (s * ce * inv_e)[:, None]
    return loss, sse, dz, de


def autograd_gradients(z, e, idx, dq, beta: float, s: float = 1.0):
    """the same (dz, de) through torch.autograd on the float64 loss with the straight-through estimator written out:
    q_ste = zn + sg(q - zn);  loss = mean |sg(zn) - q|^2 + beta mean |zn - sg(q)|^2;  objective = sum(q_ste * dq) + s loss"""
    z64 = z.double().clone().requires_grad_(True)
    e64 = e.double().clone().requires_grad_(True)
    zn = z64 / z64.norm(dim=1, keepdim=True).clamp_min(EPS)
    en = e64 / e64.norm(dim=1, keepdim=True).clamp_min(EPS)
    q = en[idx]
    q_ste = zn + (q - zn).detach()
    loss = ((zn.detach() - q) ** 2).mean() + beta * ((zn - q.detach()) ** 2).mean()
    obj = s * loss + ((q_ste * dq.double()).sum() if dq is not None else 0.0)
    dz, de = torch.autograd.grad(obj, [z64, e64])
    return loss.detach(), dz, de


def staged_f32(z, e, dq, beta: float, s: float = 1.0):
    """the staged formulation and its backward in fp32 torch on the CPU: nrm in fp32, d = (|zn|^2 + |en|^2) - 2 zn.en, first minimum,
    gather, and the closed forms of the gradients in fp32.  Same expression sequence as ops.cos_staged up to the summation order inside
    |.|^2, the dot products and the per-code sums."""
    z, e = z.float(), e.float()
    (zn, inv_z), (en, inv_e) = nrm(z), nrm(e)
    n, d = z.shape
    dist = ((zn * zn).sum(1, keepdim=True) + (en * en).sum(1)[None, :]) - 2.0 * (zn @ en.T)
    m = dist.min(1, keepdim=True).values
    idx = torch.argmax((dist == m).to(torch.uint8), dim=1)        # the FIRST minimum
    q = en[idx]
    sse = ((q - zn) ** 2).sum()
    loss = sse * ((1.0 + beta) / (n * d))
    cz, ce = 2.0 * beta / (n * d), 2.0 / (n * d)
    g = (zn - q) * (s * cz)
    if dq is not None:
        g = g + dq.float()
    dz = (g - zn * (zn * g).sum(1, keepdim=True)) * inv_z[:, None]
    ssum = torch.zeros_like(e).index_add_(0, idx, zn)
    de = (en * (en * ssum).sum(1, keepdim=True) - ssum) * (inv_e * (s * ce))[:, None]
    return dict(idx=idx, zn=zn, en=en, q=q, sse=sse, loss=loss, dz=dz, de=de)
