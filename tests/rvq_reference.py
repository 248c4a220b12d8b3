"""Float64 reference of the residual quantizer (include/vqk.h, "residual quantizer"; no GPU):

    r_0 = z;  k_q = argmin_k (|r_{q-1}|^2 + |e_k|^2) - 2 r_{q-1}.e_k  (first minimum);  r_q = r_{q-1} - e[k_q];
    zhat = ((e[k_1] + e[k_2]) + ...) + e[k_Q];  sse[q] = sum_rows |r_q|^2;  loss = (1 + beta) / (N D) sum_q sse[q];
    dz = dq + s cz sum_q r_q,  de[k] = -s ce sum_{(row, q): k_q = k} r_q,  cz = 2 beta / (N D), ce = 2 / (N D).

``forward`` runs free (its own argmins), ``teacher_forced`` evaluates every stage on the residual implied by GIVEN earlier indices,
``gradients`` are the closed forms.  ``staged_f32`` restates the staged formulation (ops.rvq_staged) in fp32 torch for the CPU.
``cases`` / ``make_case`` are the inputs of tests/test_gpu_rvq.py, shared with tests/test_rvq_cpu.py; results are cached per case."""
import functools

import numpy as np
import torch

D = 256
# (N, K, depth) of the GPU tests: one row; one code tile + a ragged block; two tiles; all tiles in the pass-1 registers; tiles beyond
# the first eight per wave; full depth
SHAPES = [(1, 32, 1), (67, 32, 2), (67, 64, 4), (2051, 1024, 4), (67, 2048, 2), (2051, 1024, 8)]
KINDS = ['scale1', 'init', 'collapsed', 'zero']
SEED = 3                # chosen in tests/test_rvq_cpu.py::test_inputs_are_separated: >= 99 % of the scale-1 pairs separated by > 2 eta


@functools.lru_cache(maxsize=None)
def make_case(n: int, k: int, depth: int, kind: str):
    """(z [N, 256], e [K, 256]) fp32 tensors.  scale1 / init: normal codebook of scale 1 / 1/K (the initialisation scale);
    collapsed: every code row a copy of one of 4 distinct rows (thousands of exact ties: the smallest index must win, the candidate
    list overflows); zero: a scale-1/4 codebook whose row 3 is the zero vector (a stage may choose it: r_q = r_{q-1})."""
    g = torch.Generator().manual_seed(SEED + 7919 * n + 31 * k + depth + 1009 * KINDS.index(kind))
    z = torch.randn(n, D, generator=g, dtype=torch.float32)
    e = torch.randn(k, D, generator=g, dtype=torch.float32)
    if kind == 'init':
        e = e / float(k)
    elif kind == 'collapsed':
        e = e[:4][torch.arange(k) % 4].contiguous()
    elif kind == 'zero':
        e = e * 0.25
        e[3] = 0.0
    elif kind != 'scale1':
        raise ValueError(kind)
    return z, e


def cases():
    return [(n, k, depth, kind) for (n, k, depth) in SHAPES for kind in KINDS]


def _dist64(r, e):
    return (r * r).sum(1, keepdim=True) + (e * e).sum(1)[None, :] - 2.0 * (r @ e.T)


def eta(r_norm, e_max_norm):
    """evaluation bound of the exact fp32 path (csrc/vq_filter.hip, file header): 2^-13 |r| max|e| + 2^-21 (|r|^2 + max|e|^2)"""
    return 2.0 ** -13 * r_norm * e_max_norm + 2.0 ** -21 * (r_norm ** 2 + e_max_norm ** 2)


def forward(z, e, depth: int):
    """free-running float64 forward: idx [N, depth], residuals [depth, N, D] (r_1 .. r_Q), zhat [N, D], sse [depth]"""
    z, e = z.double(), e.double()
    r, zhat, idx, res = z, None, [], []
    for _ in range(depth):
        k = torch.argmin(_dist64(r, e), dim=1)                   # first minimum
        q = e[k]
        r = r - q
        zhat = q if zhat is None else zhat + q
        idx.append(k)
        res.append(r)
    res = torch.stack(res)
    return dict(idx=torch.stack(idx, 1), residuals=res, zhat=zhat, sse=(res * res).sum((1, 2)))


def decode(idx, e):
    """the stage-order sum ((e[k_1] + e[k_2]) + ...) + e[k_Q] in the dtype of e"""
    out = e[idx[:, 0]]
    for q in range(1, idx.shape[1]):
        out = out + e[idx[:, q]]
    return out


def residuals(z, e, idx):
    """float64 r_1 .. r_Q [depth, N, D] implied by the given indices"""
    z, e = z.double(), e.double()
    r, res = z, []
    for q in range(idx.shape[1]):
        r = r - e[idx[:, q]]
        res.append(r)
    return torch.stack(res)


def teacher_forced(z, e, idx):
    """Every (row, stage) on the float64 residual implied by the row's EARLIER given indices: chosen = D64(k_q), best = min_k D64,
    argmin (first), gap = the distance from best to the nearest code that is not a bitwise copy of the best row (inf if none), eta2 =
    2 eta at that residual.  All [N, depth]."""
    z64, e64 = z.double(), e.double()
    e_max = float(e64.norm(dim=1).max())
    n, depth = idx.shape
    rows = torch.arange(n)
    # classes of bitwise-equal code rows: the first member represents the class
    _, inv = torch.unique(e, dim=0, return_inverse=True)
    first_of = torch.full((int(inv.max()) + 1,), e.shape[0], dtype=torch.int64)
    first_of.scatter_reduce_(0, inv, torch.arange(e.shape[0]), reduce='amin')
    out = {name: torch.empty(n, depth, dtype=torch.float64) for name in ('chosen', 'best', 'gap', 'eta2')}
    out['argmin'] = torch.empty(n, depth, dtype=torch.int64)
    r = z64
    for q in range(depth):
        d = _dist64(r, e64)
        best, arg = d.min(1)
        arg = first_of[inv[arg]]                                  # torch's min need not return the FIRST of equal minima
        other = d.masked_fill(inv[None, :] == inv[arg][:, None], float('inf'))
        out['chosen'][:, q] = d[rows, idx[:, q]]
        out['best'][:, q] = best
        out['argmin'][:, q] = arg
        out['gap'][:, q] = other.min(1).values - best
        out['eta2'][:, q] = 2.0 * eta(r.norm(dim=1), e_max)
        r = r - e64[idx[:, q]]
    return out


def check_acceptance(z, e, idx):
    """The acceptance rule of the teacher-forced check on EVERY (row, stage): the chosen code's float64 distance is within 2 eta of
    the float64 minimum, and where the runner-up is more than 2 eta away the index IS the float64 argmin (first of bitwise-equal
    rows).  Returns the fraction of separated pairs."""
    t = teacher_forced(z, e, idx)
    excess = t['chosen'] - t['best']
    bad = excess > t['eta2']
    assert not bool(bad.any()), f'{int(bad.sum())} pairs beyond 2 eta, worst excess / (2 eta) = {float((excess / t["eta2"]).max()):.3g}'
    sep = t['gap'] > t['eta2']
    wrong = sep & (idx != t['argmin'])
    assert not bool(wrong.any()), f'{int(wrong.sum())} separated pairs off the float64 argmin'
    return float(sep.double().mean())


def gradients(z, e, idx, dq, beta: float, s: float = 1.0):
    """closed forms on the given indices: (loss, sse [depth], dz [N, D], de [K, D]) in float64; dq may be None"""
    res = residuals(z, e, idx)
    n, d = z.shape
    sse = (res * res).sum((1, 2))
    loss = (1.0 + beta) / (n * d) * sse.sum()
    cz, ce = 2.0 * beta / (n * d), 2.0 / (n * d)
    total = res[0].clone()
    for q in range(1, res.shape[0]):
        total = total + res[q]
    dz = s * cz * total + (dq.double() if dq is not None else 0.0)
    de = torch.zeros(e.shape, dtype=torch.float64)
    for q in range(res.shape[0]):
        de.index_add_(0, idx[:, q], -s * ce * res[q])
    return loss, sse, dz, de


def staged_f32(z, e, depth: int):
    """the staged formulation in fp32 torch on the CPU: per stage d = (|r|^2 + |e|^2) - 2 r.e in fp32, first minimum, r <- r - e[k],
    zhat <- zhat + e[k].  Same expression sequence as ops.rvq_staged up to the summation order inside |.|^2 and the dot product."""
    z, e = z.float(), e.float()
    e2 = (e * e).sum(1)
    r, zhat, idx = z, None, []
    for _ in range(depth):
        d = ((r * r).sum(1, keepdim=True) + e2[None, :]) - 2.0 * (r @ e.T)
        m = d.min(1, keepdim=True).values
        k = torch.argmax((d == m).to(torch.uint8), dim=1)        # the FIRST minimum
        q = e[k]
        r = r - q
        zhat = q if zhat is None else zhat + q
        idx.append(k)
    return torch.stack(idx, 1), zhat
