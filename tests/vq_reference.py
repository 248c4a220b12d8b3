"""Float64 reference of the standard and EMA quantizers (include/vqk.h, "vector quantizer" and the EMA entries; no GPU, nothing of
the product code):

    z [N, D], e [K, D] fp32.  Ranking (vector_quantizers.py:37-44 of the reference project):
        assoc 0:  d_k = (|z|^2 + |e_k|^2) - 2 z.e_k          assoc 1:  d_k = (|z|^2 - 2 z.e_k) + |e_k|^2
        idx = argmin_k d_k, the FIRST minimum; bitwise-equal code rows resolve to the lowest index.
    Forward (:44-56):  q = e[idx];  sse = sum (q - z)^2;  loss = (1 + beta) / (N D) sse (standard), beta / (N D) sse (EMA);
        hist[k] = #{rows on k}.
    Gradients (:52-56 differentiated, s = the loss cotangent):  dz = dq + s cz (z - q),  de[k] = s ce sum_{idx = k} (e_k - z),
        cz = 2 beta / (N D), ce = 2 / (N D) (EMA: no de).
    EMA statistics (:159-166):  counts[k] = #{rows on k},  dw[k] = sum_{idx = k} z   (mags[k] = sum |z|: the bounds' scale).
    EMA update (:161-169):  c' = decay c + (1 - decay) counts;  count = (c' + eps) / (batch + K eps) batch;
        w = decay w + (1 - decay) dw;  codebook = w / count.
        The C-ABI takes decay and eps as fp32 and forms 1.0f - decay from the fp32 value (exact for decay >= 0.5 and for 0): ``ema_update``
        takes exactly those numbers.  The reference project forms 1 - decay in double and hands the product's scalar to an fp32 tensor
        operation, i.e. fp32(1 - decay_double): ``ema_update_project`` is that variant (the two factors differ by about 2^-22 relative at
        decay = 0.95; tests/test_vq_cpu.py records the distance).

``forward`` runs free (its own argmin), ``teacher_forced`` / ``check_acceptance`` judge GIVEN indices as rvq_reference.check_acceptance
does, ``gradients`` are the closed forms, ``autograd_gradients`` the same through torch.autograd in float64 with the straight-through
estimator written out, ``staged_f32`` the forward and gradients in fp32 torch on the CPU (only to measure what an fp32 evaluation costs).

ETA.  rvq_reference.eta(|z|, max|e|) = 2^-13 |z| max|e| + 2^-21 (|z|^2 + max|e|^2) was written for D = 256 (csrc/vq_filter.hip, file
header).  Its leading term pays for the dot product: an fp32 chain of d fused multiply-adds has the first-order bound
|fl(z.e) - z.e| <= d 2^-24 |z| |e| (one rounding per term, Cauchy-Schwarz on sum |z_i e_i|), and the distance holds 2 z.e, so the term
must cover d 2^-23 |z| |e|: it does for d <= 1024 (2^10 2^-23 = 2^-13; at D = 256 with a factor 4 to spare).  The assignment admits
d <= 1264, so for 1024 < d the whole of eta is scaled by d / 1024 (at most 1.235); below, it is the residual quantizer's bound as it
stands.  The second term pays for the two outer roundings and the rounding of |e_k|^2 (the error of |z|^2 is common to every code of a
row and leaves the comparison).

``make_case`` / ``planted`` / ``ema_case`` are the inputs of tests/test_gpu_vq.py, shared with tests/test_vq_cpu.py; cached, read-only."""
import functools

import numpy as np
import torch

from tests import rvq_reference

# (N, K, D) of the assignment tests: a single code (three idle waves); a ragged block and a ragged code tile; ...; the first d whose
# z tile passes 64 KiB of LDS; the largest d admitted; D = 256: one row, K % 32 != 0 (the register kernel alone), many blocks and tiles
ASSIGN_SHAPES = [(1, 1, 8), (33, 40, 8), (77, 100, 24), (64, 160, 264), (33, 96, 512), (33, 64, 1024), (33, 64, 1264),
                 (1, 32, 256), (33, 40, 256), (2051, 1024, 256)]
ASSIGN_KINDS = ['scale1', 'init', 'collapsed']
GATHER_SHAPES = [(5, 16, 4), (77, 100, 12), (300, 16384, 8), (2051, 1024, 256)]
LOOKUP_SHAPES = [(33, 64, 64), (2048, 64, 256)]                 # through ops.VQLookupFn
KINDS = ['scale1', 'init', 'collapsed', 'onecode', 'spread', 'mixed']
SEED = 9                # chosen in tests/test_vq_cpu.py::test_inputs_are_separated: the first seed at which the float64 reference alone
                        # separates >= 99 % of the scale-1 rows of every ASSIGN / LOOKUP shape by more than 2 eta; every shape 100 % but
                        # (2051, 1024, 256): 99.22 % and (2048, 64, 256): 99.61 %.  (Seeds 1 - 8 leave one row of a 33-row shape or of
                        # (77, 100, 24) unseparated: 93.9 - 98.7 %.)


def _gen(n, k, d, kind):
    return torch.Generator().manual_seed(SEED + 7919 * n + 31 * k + d + 1009 * KINDS.index(kind))


@functools.lru_cache(maxsize=None)
def make_case(n: int, k: int, d: int, kind: str):
    """(z [N, D], e [K, D]) fp32.  scale1 / init: normal latents, normal codebook of scale 1 / 1/K; collapsed: every code a copy of one
    of 4 rows (exact ties: the lowest index must win); onecode: every row is code 0 plus noise of 0.05 (all rows on code 0); spread
    (N <= K): row r is code planted[r] plus noise of 0.01, the planted codes pairwise distinct; mixed: row magnitudes 10^-3 .. 10^3
    against a normal codebook."""
    g = _gen(n, k, d, kind)
    z = torch.randn(n, d, generator=g, dtype=torch.float32)
    e = torch.randn(k, d, generator=g, dtype=torch.float32)
    if kind == 'init':
        e = e / float(k)
    elif kind == 'collapsed':
        e = e[:4][torch.arange(k) % 4].contiguous()
    elif kind == 'onecode':
        z = (e[0][None, :] + 0.05 * z).contiguous()
    elif kind == 'spread':
        assert n <= k
        z = (e[torch.randperm(k, generator=g)[:n]] + 0.01 * z).contiguous()
    elif kind == 'mixed':
        z = (z * 10.0 ** torch.randint(-3, 4, (n, 1), generator=g).float()).contiguous()
    elif kind != 'scale1':
        raise ValueError(kind)
    return z, e


@functools.lru_cache(maxsize=None)
def planted(n: int, k: int, d: int, kind: str):
    """the indices a case was built around, int64 [N] (onecode: zeros; spread: the permutation's head) -- tests/test_vq_cpu.py shows on
    the small shapes that they ARE the float64 argmin; every other kind: the free-running float64 forward"""
    if kind == 'onecode':
        return torch.zeros(n, dtype=torch.int64)
    if kind == 'spread':
        g = _gen(n, k, d, kind)
        torch.randn(n, d, generator=g, dtype=torch.float32)
        torch.randn(k, d, generator=g, dtype=torch.float32)
        return torch.randperm(k, generator=g)[:n].clone()
    return reference(n, k, d, kind)['idx']


@functools.lru_cache(maxsize=None)
def ema_case(n: int, k: int, d: int, kind: str):
    """(z [N, D], idx [N]) of the EMA-statistics tests; the kernels take the indices as an input, so ``mixed`` draws them at random
    (code 1 emptied into code 0: an empty and a crowded code); onecode / spread leave K - 1 / K - N codes without rows"""
    z, _ = make_case(n, k, d, kind)
    if kind == 'mixed':
        idx = torch.randint(0, k, (n,), generator=torch.Generator().manual_seed(SEED + n + d))
        idx[idx == 1] = 0
        return z, idx
    return z, planted(n, k, d, kind)


def eta(z_norm, e_max_norm, d: int):
    """evaluation bound of the exact fp32 ranking at width d (see ETA above)"""
    return rvq_reference.eta(z_norm, e_max_norm) * max(1.0, d / 1024.0)


def dist64(z, e, assoc: int = 0):
    z, e = z.double(), e.double()
    z2, e2, ze = (z * z).sum(1, keepdim=True), (e * e).sum(1)[None, :], z @ e.T
    return (z2 + e2) - 2.0 * ze if assoc == 0 else (z2 - 2.0 * ze) + e2


def first_of_class(e):
    """per code: the first index among its bitwise-equal rows"""
    _, inv = torch.unique(e, dim=0, return_inverse=True)
    first_of = torch.full((int(inv.max()) + 1,), e.shape[0], dtype=torch.int64)
    first_of.scatter_reduce_(0, inv, torch.arange(e.shape[0]), reduce='amin')
    return inv, first_of


def hist(idx, k: int):
    return torch.bincount(idx, minlength=k)


def forward(z, e, assoc: int = 0):
    """free-running float64 forward: idx [N] (first minimum, lowest index of bitwise-equal rows), q [N, D], sse, hist [K]"""
    inv, first_of = first_of_class(e)
    idx = first_of[inv[dist64(z, e, assoc).argmin(1)]]
    q = e.double()[idx]
    return dict(idx=idx, q=q, sse=((q - z.double()) ** 2).sum(), hist=hist(idx, e.shape[0]))


@functools.lru_cache(maxsize=None)
def reference(n: int, k: int, d: int, kind: str):
    """the free-running float64 forward (assoc 0) of a case, computed once and shared (read-only)"""
    return forward(*make_case(n, k, d, kind))


def teacher_forced(z, e, idx, assoc: int = 0):
    """every row in float64: chosen = d(idx), best = min_k d, argmin (first of bitwise-equal rows), gap = the distance from best to the
    nearest code that is not a bitwise copy of the best row (inf if none), eta2 = 2 eta of the row.  All [N]."""
    d = dist64(z, e, assoc)
    inv, first_of = first_of_class(e)
    best, arg = d.min(1)
    arg = first_of[inv[arg]]
    other = d.masked_fill(inv[None, :] == inv[arg][:, None], float('inf'))
    eta2 = 2.0 * eta(z.double().norm(dim=1), float(e.double().norm(dim=1).max()), z.shape[1])
    return dict(chosen=d[torch.arange(z.shape[0]), idx], best=best, argmin=arg, gap=other.min(1).values - best, eta2=eta2)


def check_acceptance(z, e, idx, assoc: int = 0):
    """on EVERY row: the chosen code's float64 distance is within 2 eta of the float64 minimum, and where the runner-up is more than
    2 eta away the index IS the float64 argmin (first of bitwise-equal rows).  Returns the fraction of separated rows."""
    assert int(idx.min()) >= 0 and int(idx.max()) < e.shape[0]
    t = teacher_forced(z, e, idx, assoc)
    excess = t['chosen'] - t['best']
    bad = excess > t['eta2']
    assert not bool(bad.any()), f'{int(bad.sum())} rows beyond 2 eta, worst excess / (2 eta) = {float((excess / t["eta2"]).max()):.3g}'
    sep = t['gap'] > t['eta2']
    wrong = sep & (idx != t['argmin'])
    assert not bool(wrong.any()), f'{int(wrong.sum())} separated rows off the float64 argmin'
    return float(sep.double().mean())


def coefficients(n: int, d: int, beta: float):
    """(cz, ce) = (2 beta / (N D), 2 / (N D))"""
    return 2.0 * beta / (n * d), 2.0 / (n * d)


def quantities(z, e, idx, beta: float, ema: bool = False):
    """forward quantities on the given indices in float64: q, sse, loss, hist"""
    q = e.double()[idx]
    sse = ((q - z.double()) ** 2).sum()
    coef = (beta if ema else 1.0 + beta) / (z.shape[0] * z.shape[1])
    return dict(q=q, sse=sse, loss=coef * sse, hist=hist(idx, e.shape[0]))


def code_sums(z, e, idx):
    """(S [K, D] = sum_{idx = k} (e_k - z), M [K, D] = sum_{idx = k} |e_k - z|, n_k [K]) in float64"""
    diff = e.double()[idx] - z.double()
    s = torch.zeros(e.shape, dtype=torch.float64, device=e.device).index_add_(0, idx, diff)
    m = torch.zeros(e.shape, dtype=torch.float64, device=e.device).index_add_(0, idx, diff.abs())
    return s, m, hist(idx, e.shape[0])


def gradients(z, e, idx, dq, cz: float, ce: float, s: float = 1.0):
    """closed forms on the given indices: (dz [N, D], de [K, D]) in float64; dq may be None"""
    z64 = z.double()
    q = e.double()[idx]
    dz = s * cz * (z64 - q) + (dq.double() if dq is not None else 0.0)
    de = torch.zeros(e.shape, dtype=torch.float64, device=e.device).index_add_(0, idx, q - z64) * (s * ce)
    return dz, de


def autograd_gradients(z, e, idx, dq, beta: float, s: float = 1.0, ema: bool = False):
    """(loss, dz, de) through torch.autograd on the float64 loss with the straight-through estimator written out:
    q_ste = z + sg(q - z);  loss = [mean |sg(z) - q|^2 +] beta mean |z - sg(q)|^2;  objective = sum(q_ste * dq) + s loss.
    EMA: the codebook term is absent and de is None."""
    z64 = z.double().clone().requires_grad_(True)
    e64 = e.double().clone().requires_grad_(not ema)
    q = e64[idx]
    q_ste = z64 + (q - z64).detach()
    loss = beta * ((z64 - q.detach()) ** 2).mean()
    if not ema:
        loss = ((z64.detach() - q) ** 2).mean() + loss
    obj = s * loss + ((q_ste * dq.double()).sum() if dq is not None else 0.0)
    if ema:
        return loss.detach(), torch.autograd.grad(obj, [z64])[0], None
    dz, de = torch.autograd.grad(obj, [z64, e64])
    return loss.detach(), dz, de


def grad_bounds(z, e, idx, dz_want, de_want, cz: float, ce: float, s: float, tol, prefill=None, sums=None):
    """THE per-element bounds of dz and de (tests/test_gpu_vq.py and the restatement measure of tests/test_vq_cpu.py).  tol = the
    project's (rtol, atol) pairs for the two quantities (tests/test_rot_cpu.py::TOL).  The gradients are O(1 / (N D)), so the atol is
    scaled by what it stands for, the magnitude the element was summed from:
        dz[r, c]:  rtol |want| + atol s cz |z - q|[r, c]
        de[k, c]:  rtol |want - prefill| + atol s ce M[k, c],   M = sum_{idx = k} |e_k - z|
    Into a pre-filled buffer (want = prefill + gradient) every addition also rounds relative to the running value: at most n_k
    additions touch element (k, c), one per row at the most, so the bound grows by (n_k + 1) 2^-24 (|prefill| + s ce M).
    ``sums``: what code_sums(z, e, idx) returned, when the caller has it.  The tensors may live on any device (torch float64 there)."""
    q = e.double()[idx]
    _, m, nk = sums if sums is not None else code_sums(z, e, idx)
    dz_allowed = tol['dz'][0] * dz_want.abs() + tol['dz'][1] * abs(s * cz) * (z.double() - q).abs()
    if prefill is None:
        return dz_allowed, tol['de'][0] * de_want.abs() + tol['de'][1] * abs(s * ce) * m
    pre = prefill.double()
    de_allowed = tol['de'][0] * (de_want - pre).abs() + tol['de'][1] * abs(s * ce) * m
    return dz_allowed, de_allowed + (nk.double()[:, None] + 1.0) * 2.0 ** -24 * (pre.abs() + abs(s * ce) * m)


def ema_stats(z, idx, k: int):
    """(counts [K], dw [K, D], mags [K, D] = sum_{idx = k} |z|) in float64"""
    z64 = z.double()
    dw = torch.zeros(k, z.shape[1], dtype=torch.float64, device=z.device).index_add_(0, idx, z64)
    mags = torch.zeros(k, z.shape[1], dtype=torch.float64, device=z.device).index_add_(0, idx, z64.abs())
    return hist(idx, k).double(), dw, mags


def _ema_update(c, w, counts, dw, decay: float, one_minus: float, eps: float, batch: float):
    k = c.shape[0]
    c1 = decay * c.double() + one_minus * counts.double()
    count = (c1 + eps) / (batch + k * eps) * batch
    weight = decay * w.double() + one_minus * dw.double()
    return dict(count=count, weight=weight, codebook=weight / count[:, None], wa=(decay * w.double()).abs(), wb=(one_minus * dw.double()).abs())


def ema_update(c, w, counts, dw, decay: float, eps: float, batch: float):
    """float64 update on the numbers the kernel receives: decay and eps rounded to fp32, 1 - decay formed from that fp32 value (in
    fp32, as ``1.0f - decay`` does).  count [K], weight [K, D], codebook [K, D]; wa, wb = |decay w|, |(1 - decay) dw| (the bounds' scale)."""
    d32, e32 = np.float32(decay), np.float32(eps)
    return _ema_update(c, w, counts, dw, float(d32), float(np.float32(1.0) - d32), float(e32), float(np.float32(batch)))


def ema_update_project(c, w, counts, dw, decay: float, eps: float, batch: float):
    """the reference project's variant: 1 - decay in double, that scalar then rounded to fp32 by the tensor operation that takes it"""
    return _ema_update(c, w, counts, dw, float(np.float32(decay)), float(np.float32(1.0 - decay)), float(np.float32(eps)), float(batch))


def staged_f32(z, e, dq, cz: float, ce: float, s: float = 1.0, assoc: int = 0, idx=None):
    """the forward and the gradients in fp32 torch on the CPU: d as ``assoc`` associates it, first minimum, gather, sum (q - z)^2 and the
    closed forms with fp32 coefficients.  ``idx``: skip the ranking and use the given indices."""
    z, e = z.float(), e.float()
    if idx is None:
        z2, e2, ze = (z * z).sum(1, keepdim=True), (e * e).sum(1)[None, :], 2.0 * (z @ e.T)
        dist = (z2 + e2) - ze if assoc == 0 else (z2 - ze) + e2
        m = dist.min(1, keepdim=True).values
        idx = torch.argmax((dist == m).to(torch.uint8), dim=1)             # the FIRST minimum
    q = e[idx]
    sse = ((q - z) ** 2).sum()
    czs, ces = torch.tensor(cz, dtype=torch.float32) * torch.tensor(s, dtype=torch.float32), torch.tensor(ce, dtype=torch.float32) * torch.tensor(s, dtype=torch.float32)
    dz = (z - q) * czs
    if dq is not None:
        dz = dz + dq.float()
    de = torch.zeros_like(e).index_add_(0, idx, q - z) * ces
    return dict(idx=idx, q=q, sse=sse, dz=dz, de=de)
