"""Float64 reference of the grouped quantizer (include/vqk.h, "grouped quantizer"; no GPU):

    z [N, D], D = G d, group g owns columns g d .. (g + 1) d - 1;  e [G K, d], row g K + k = code k of group g;
    idx[r, g] = argmin_k (|z_rg|^2 + |e_gk|^2) - 2 z_rg.e_gk  (first minimum);  q[r, g d:(g + 1) d] = e[g K + idx[r, g]];
    sse = sum |q - z|^2;  loss = (1 + beta) / (N D) sse;  hist[g K + k] = #{r: idx[r, g] = k};
    dz = dq + s cz (z - q);  de[g K + k] = s ce sum_{r: idx[r, g] = k} (e_gk - z_rg),  cz = 2 beta / (N D), ce = 2 / (N D).

``forward`` runs free (its own argmin, the first of bitwise-equal rows), ``teacher_forced`` / ``check_acceptance`` judge GIVEN indices per
(row, group) with eta = rvq_reference.eta(|z_rg|, max_k |e_gk|), ``gradients`` are the closed forms, ``autograd_gradients`` the same
through torch.autograd with the straight-through estimator written out.  ``staged_f32`` restates the definition in fp32 torch for
the CPU.  ``cases`` / ``make_case`` are the inputs of tests/test_gpu_gvq.py, shared with tests/test_gvq_cpu.py; results are cached."""
import functools

import torch

from tests import rvq_reference

# (N, K, d, G) of the GPU tests: one row, one code tile, three idle waves; a ragged last block with pitch != d; an uneven split of 3
# tiles over 4 waves with a non-power-of-two G (D = 48); the widest group (D = 256); many blocks and tiles; the shipped config's shape
# (many codes in few dimensions: near-ties densest)
SHAPES = [(1, 32, 8, 1), (77, 32, 8, 2), (64, 96, 16, 3), (33, 64, 64, 4), (2051, 1024, 32, 2), (256, 4096, 8, 8)]
KINDS = ['scale1', 'init', 'collapsed', 'scaled']
SEED = 4                # chosen so that the float64 reference alone separates >= 99 % of the scale-1 (row, group) pairs of every shape by
                        # more than 2 eta (tests/test_gvq_cpu.py::test_inputs_are_separated; seeds 2 and 3 leave 98.7 - 99.0 % at K = 4096, d = 8)


@functools.lru_cache(maxsize=None)
def make_case(n: int, k: int, d: int, groups: int, kind: str):
    """(z [N, G d], e [G K, d]) fp32 tensors.  scale1 / init: normal codebooks of scale 1 / 1/K (the initialisation scale); collapsed:
    every code of a group a copy of one of 4 distinct rows of that group (exact ties: the smallest index must win); scaled: group g's
    latents and codes multiplied by 4^g (a wrong slab or pitch pairs operands of different scales and cannot pass)."""
    g = torch.Generator().manual_seed(SEED + 7919 * n + 31 * k + d + 104729 * groups + 1009 * KINDS.index(kind))
    z = torch.randn(n, groups * d, generator=g, dtype=torch.float32)
    e = torch.randn(groups * k, d, generator=g, dtype=torch.float32)
    if kind == 'init':
        e = e / float(k)
    elif kind == 'collapsed':
        e = e.view(groups, k, d)[:, :4][:, torch.arange(k) % 4].reshape(groups * k, d).contiguous()
    elif kind == 'scaled':
        scale = 4.0 ** torch.arange(groups, dtype=torch.float32)
        z = (z.view(n, groups, d) * scale[None, :, None]).reshape(n, groups * d).contiguous()
        e = (e.view(groups, k, d) * scale[:, None, None]).reshape(groups * k, d).contiguous()
    elif kind != 'scale1':
        raise ValueError(kind)
    return z, e


def cases():
    return [(n, k, d, g, kind) for (n, k, d, g) in SHAPES for kind in KINDS]


def eta(z_norm, e_max_norm):
    """evaluation bound of the exact fp32 ranking for a slice of norm |z_rg| against a slab whose longest code is max_k |e_gk|"""
    return rvq_reference.eta(z_norm, e_max_norm)


def split(z, e, groups: int):
    """(z as [N, G, d], e as [G, K, d]) views"""
    n = z.shape[0]
    d = e.shape[1]
    return z.view(n, groups, d), e.view(groups, e.shape[0] // groups, d)


def _dist64(zg, eg):
    return (zg * zg).sum(1, keepdim=True) + (eg * eg).sum(1)[None, :] - 2.0 * (zg @ eg.T)


def _first_of_class(eg):
    """per code of one slab: the first index among its bitwise-equal rows"""
    _, inv = torch.unique(eg, dim=0, return_inverse=True)
    first_of = torch.full((int(inv.max()) + 1,), eg.shape[0], dtype=torch.int64)
    first_of.scatter_reduce_(0, inv, torch.arange(eg.shape[0]), reduce='amin')
    return inv, first_of


def global_ids(idx, k: int):
    """idx [N, G] -> g K + idx [N, G]"""
    return idx + torch.arange(idx.shape[1], dtype=torch.int64) * k


def decode(idx, e):
    """q [N, G d] in the dtype of e: the concatenated code rows of the given tokens"""
    groups = idx.shape[1]
    k = e.shape[0] // groups
    return e[global_ids(idx, k)].reshape(idx.shape[0], groups * e.shape[1])


def hist(idx, k: int):
    return torch.bincount(global_ids(idx, k).reshape(-1), minlength=idx.shape[1] * k)


def forward(z, e, groups: int):
    """free-running float64 forward: idx [N, G] (first minimum), q [N, D], sse"""
    z3, e3 = split(z, e, groups)
    idx = []
    for g in range(groups):
        inv, first_of = _first_of_class(e3[g])
        idx.append(first_of[inv[_dist64(z3[:, g].double(), e3[g].double()).argmin(1)]])
    idx = torch.stack(idx, 1)
    q = decode(idx, e.double())
    return dict(idx=idx, q=q, sse=((q - z.double()) ** 2).sum())


def teacher_forced(z, e, idx, groups: int):
    """every (row, group) in float64: chosen = D64(idx), best = min_k D64, argmin (first of bitwise-equal rows), gap = the distance
    from best to the nearest code that is not a bitwise copy of the best row (inf if none), eta2 = 2 eta of that pair.  All [N, G]."""
    z3, e3 = split(z, e, groups)
    n = z.shape[0]
    rows = torch.arange(n)
    out = {name: torch.empty(n, groups, dtype=torch.float64) for name in ('chosen', 'best', 'gap', 'eta2')}
    out['argmin'] = torch.empty(n, groups, dtype=torch.int64)
    for g in range(groups):
        zg, eg = z3[:, g].double(), e3[g].double()
        d = _dist64(zg, eg)
        inv, first_of = _first_of_class(e3[g])
        best, arg = d.min(1)
        arg = first_of[inv[arg]]
        other = d.masked_fill(inv[None, :] == inv[arg][:, None], float('inf'))
        out['chosen'][:, g] = d[rows, idx[:, g]]
        out['best'][:, g] = best
        out['argmin'][:, g] = arg
        out['gap'][:, g] = other.min(1).values - best
        out['eta2'][:, g] = 2.0 * eta(zg.norm(dim=1), float(eg.norm(dim=1).max()))
    return out


def check_acceptance(z, e, idx, groups: int):
    """on EVERY (row, group): the chosen code's float64 distance is within 2 eta of the float64 minimum, and where the runner-up is
    more than 2 eta away the index IS the float64 argmin (first of bitwise-equal rows).  Returns the fraction of separated pairs."""
    t = teacher_forced(z, e, idx, groups)
    excess = t['chosen'] - t['best']
    bad = excess > t['eta2']
    assert not bool(bad.any()), f'{int(bad.sum())} pairs beyond 2 eta, worst excess / (2 eta) = {float((excess / t["eta2"]).max()):.3g}'
    sep = t['gap'] > t['eta2']
    wrong = sep & (idx != t['argmin'])
    assert not bool(wrong.any()), f'{int(wrong.sum())} separated pairs off the float64 argmin'
    return float(sep.double().mean())


def gradients(z, e, idx, dq, beta: float, s: float = 1.0):
    """closed forms on the given indices: (loss, sse, dz [N, D], de [G K, d]) in float64; dq may be None"""
    n, dd = z.shape
    groups = idx.shape[1]
    k, d = e.shape[0] // groups, e.shape[1]
    z64, e64 = z.double(), e.double()
    q = decode(idx, e64)
    sse = ((q - z64) ** 2).sum()
    loss = (1.0 + beta) / (n * dd) * sse
    cz, ce = 2.0 * beta / (n * dd), 2.0 / (n * dd)
    dz = s * cz * (z64 - q) + (dq.double() if dq is not None else 0.0)
    de = torch.zeros(e.shape, dtype=torch.float64).index_add_(0, global_ids(idx, k).reshape(-1), (q - z64).reshape(n * groups, d)) * (s * ce)
    return loss, sse, dz, de


def autograd_gradients(z, e, idx, dq, beta: float, s: float = 1.0):
    """the same (loss, dz, de) through torch.autograd on the float64 loss with the straight-through estimator written out:
    q_ste = z + sg(q - z);  loss = mean |sg(z) - q|^2 + beta mean |z - sg(q)|^2;  objective = sum(q_ste * dq) + s loss"""
    z64 = z.double().clone().requires_grad_(True)
    e64 = e.double().clone().requires_grad_(True)
    q = decode(idx, e64)
    q_ste = z64 + (q - z64).detach()
    loss = ((z64.detach() - q) ** 2).mean() + beta * ((z64 - q.detach()) ** 2).mean()
    obj = s * loss + ((q_ste * dq.double()).sum() if dq is not None else 0.0)
    dz, de = torch.autograd.grad(obj, [z64, e64])
    return loss.detach(), dz, de


def staged_f32(z, e, groups: int, dq, beta: float, s: float = 1.0):
    """the definition and its backward in fp32 torch on the CPU: per group d = (|z_g|^2 + |e_g|^2) - 2 z_g.e_g, first minimum, gather,
    and the closed forms of the gradients in fp32.  Same expression sequence as ops.gvq_staged up to the summation order inside |.|^2,
    the dot products and the per-code sums."""
    z, e = z.float(), e.float()
    n, dd = z.shape
    k, d = e.shape[0] // groups, e.shape[1]
    z3, e3 = split(z, e, groups)
    idx = []
    for g in range(groups):
        zg, eg = z3[:, g], e3[g]
        dist = ((zg * zg).sum(1, keepdim=True) + (eg * eg).sum(1)[None, :]) - 2.0 * (zg @ eg.T)
        m = dist.min(1, keepdim=True).values
        idx.append(torch.argmax((dist == m).to(torch.uint8), dim=1))        # the FIRST minimum
    idx = torch.stack(idx, 1)
    q = decode(idx, e)
    sse = ((q - z) ** 2).sum()
    loss = sse * ((1.0 + beta) / (n * dd))
    cz, ce = 2.0 * beta / (n * dd), 2.0 / (n * dd)
    dz = (z - q) * (s * cz)
    if dq is not None:
        dz = dz + dq.float()
    de = torch.zeros_like(e).index_add_(0, global_ids(idx, k).reshape(-1), (q - z).reshape(n * groups, d)) * (s * ce)
    return dict(idx=idx, q=q, sse=sse, loss=loss, dz=dz, de=de)


@functools.lru_cache(maxsize=None)
def reference(n: int, k: int, d: int, groups: int, kind: str):
    """the free-running float64 forward of a case, computed once and shared (read-only)"""
    z, e = make_case(n, k, d, groups, kind)
    return forward(z, e, groups)
