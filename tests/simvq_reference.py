"""Float64 reference of the SimVQ quantizer (include/vqk.h, "SimVQ quantizer"; no GPU):

    z [N, D] latent rows;  C [K, D] the frozen table;  W [D, D], b [D] the linear layer (nn.Linear orientation);
    E[k, i] = sum_j C[k, j] W[i, j] + b[i];  idx[r] = argmin_k (|z_r|^2 + |E_k|^2) - 2 z_r.E_k  (first minimum);  q_r = E[idx[r]];
    sse = sum |q - z|^2;  loss = (1 + beta) / (N D) sse;  hist[k] = #{r: idx[r] = k};
    dz = dq + s cz (z - q);  g_r = s ce (q_r - z_r);  dW[i, j] = sum_r g_r[i] C[idx_r, j];  db[i] = sum_r g_r[i];  C gets nothing;
    cz = 2 beta / (N D), ce = 2 / (N D).  A token outside [0, K) is a zero code: q = 0 in dz, no term in dW / db.

``effective`` / ``projection_bound`` are the float64 projection and the derived fp32 summation bound of an fp32 evaluation in ANY
order; ``forward`` runs free on the float64 E; ``check_acceptance`` judges GIVEN indices against a GIVEN (device) E with the rule of
tests/gvq_reference.py at one group (eta = rvq_reference.eta); ``gradients`` are the closed forms teacher-forced on a given E and
indices, with the sums of absolute terms the dW / db bounds are stated in; ``autograd_gradients`` is the same through
torch.autograd with the straight-through estimator written out; ``staged_f32`` restates everything in fp32 torch for the CPU.
``SHAPES`` / ``make_case`` are the inputs of tests/test_gpu_simvq.py, shared with tests/test_simvq_cpu.py; results are cached."""
import functools

import torch

from tests import gvq_reference, rvq_reference

# (N, K, D) of the GPU tests: one row in one block; a ragged row block and a code tile (96 of 128 codes) that is no power of two; a
# second chunk of one row at D = 128; one full chunk pair at D = 256; several partial slices with a ragged last range; many code tiles
SHAPES = [(1, 32, 64), (77, 96, 64), (33, 64, 128), (64, 32, 256), (2051, 1024, 256), (256, 4096, 128)]
STAGED_SHAPE = (40, 40, 48)         # served by the staged path alone: D outside {64, 128, 256}, K % 32 != 0
KINDS = ['identity', 'random', 'collapsed', 'nobias']
SEED = 1                # chosen so that the float64 reference alone separates >= 99 % of the rows of every `random` case by more than
                        # 2 eta (tests/test_simvq_cpu.py::test_inputs_are_separated)
U = 2.0 ** -24          # unit roundoff of fp32


@functools.lru_cache(maxsize=None)
def make_case(n: int, k: int, d: int, kind: str):
    """(z [N, D], C [K, D], W [D, D], b [D] or None) fp32.  C ~ N(0, 1 / D) as the module draws it.  identity: W = I, b = 0 (E = C);
    random: W = N(0, 1 / D) entries -- non-symmetric, a transposed W cannot pass -- and b = 0.1 N(0, 1); collapsed: every row of C a copy
    of one of 4 distinct rows (exact ties in E: the smallest index must win) under the random W and b; nobias: the random W, b absent."""
    g = torch.Generator().manual_seed(SEED + 7919 * n + 31 * k + d + 1009 * KINDS.index(kind))
    z = torch.randn(n, d, generator=g, dtype=torch.float32)
    c = torch.randn(k, d, generator=g, dtype=torch.float32) * d ** -0.5
    w = torch.randn(d, d, generator=g, dtype=torch.float32) * d ** -0.5
    b = 0.1 * torch.randn(d, generator=g, dtype=torch.float32)
    if kind == 'identity':
        w, b = torch.eye(d, dtype=torch.float32), torch.zeros(d, dtype=torch.float32)
    elif kind == 'collapsed':
        c = c[:4][torch.arange(k) % 4].contiguous()
    elif kind == 'nobias':
        b = None
    elif kind != 'random':
        raise ValueError(kind)
    # every second row lies near a code, as the latents of a trained encoder do (E[pick] + noise of 0.3 the code scale); the others
    # stay free Gaussians, where near-ties are densest
    e = effective(c, w, b).float()
    pick = torch.randint(0, k, (n,), generator=g)
    near = e[pick] + 0.3 * float(e.std()) * torch.randn(n, d, generator=g, dtype=torch.float32)
    z = torch.where((torch.arange(n) % 2 == 1)[:, None], near, z).contiguous()
    return z, c, w, b


def cases(kinds=KINDS):
    return [(n, k, d, kind) for (n, k, d) in SHAPES for kind in kinds]


def effective(c, w, b):
    """E [K, D] in float64"""
    e = c.double() @ w.double().T
    return e + b.double() if b is not None else e


def projection_bound(c, w, b):
    """|E_fp32 - E_64|[k, i] <= (D + 2) u (sum_j |C_kj W_ij| + |b_i|): D products summed in any order (D - 1 additions), the bias
    addition, first-order rounding with the (1 + u)^n slack taken by the two spare units"""
    d = c.shape[1]
    t = c.double().abs() @ w.double().abs().T
    if b is not None:
        t = t + b.double().abs()
    return (d + 2) * U * t


def forward(z, c, w, b):
    """free-running float64 forward on the float64 E: idx [N] (first minimum), q [N, D], sse, E"""
    e = effective(c, w, b)
    f = gvq_reference.forward(z.double(), e, 1)
    return dict(idx=f['idx'][:, 0], q=f['q'], sse=f['sse'], e=e)


def check_acceptance(z, e, idx):
    """on EVERY row, against the GIVEN E (fp32, as the device wrote it): the chosen code's float64 distance is within 2 eta of the
    float64 minimum, and where the runner-up is more than 2 eta away the index IS the float64 argmin (first of bitwise-equal rows).
    Returns the fraction of separated rows."""
    return gvq_reference.check_acceptance(z, e, idx.view(-1, 1), 1)


def separated_fraction(z, e):
    """fraction of rows whose float64 runner-up distance exceeds the float64 winner's by more than 2 eta, on the given E"""
    idx = gvq_reference.forward(z, e, 1)['idx']
    t = gvq_reference.teacher_forced(z, e, idx, 1)
    return float((t['gap'] > t['eta2']).double().mean())


def hist(idx, k: int):
    ok = (idx >= 0) & (idx < k)
    return torch.bincount(idx[ok], minlength=k)


def gradients(z, e, c, idx, dq, beta: float, s: float = 1.0):
    """closed forms teacher-forced on the given E and indices, float64: dict(loss, sse, dz [N, D], dw [D, D], db [D], dw_terms, db_terms)
    with dw_terms[i, j] = sum_r |g_r[i] C[idx_r, j]| and db_terms[i] = sum_r |g_r[i]|; dq may be None; tokens outside [0, K) are zero
    codes without a term"""
    n, d = z.shape
    k = e.shape[0]
    z64, e64, c64 = z.double(), e.double(), c.double()
    ok = (idx >= 0) & (idx < k)
    safe = idx.clamp(0, k - 1)
    q = e64[safe] * ok[:, None]
    cg = c64[safe] * ok[:, None]
    sse = ((q - z64) ** 2).sum()
    loss = (1.0 + beta) / (n * d) * sse
    cz, ce = 2.0 * beta / (n * d), 2.0 / (n * d)
    dz = s * cz * (z64 - q) + (dq.double() if dq is not None else 0.0)
    g = s * ce * (q - z64) * ok[:, None]
    return dict(loss=loss, sse=sse, dz=dz, dw=g.T @ cg, db=g.sum(0), dw_terms=g.abs().T @ cg.abs(), db_terms=g.abs().sum(0))


def gradient_bounds(ref, n: int):
    """(N + 8) u term_sum for dW and db: N - 1 additions in any order plus the roundings of forming a term in fp32 -- ce as an fp32
    number, s ce, q - z, the product -- and the final old + sum"""
    return (n + 8) * U * ref['dw_terms'], (n + 8) * U * ref['db_terms']


def autograd_gradients(z, c, w, b, idx, dq, beta: float, s: float = 1.0):
    """(loss, dz, dW, db, dC) through torch.autograd on the float64 loss with the straight-through estimator written out:
    E = C W^T + b;  q = E[idx];  q_ste = z + sg(q - z);  loss = mean |sg(z) - q|^2 + beta mean |z - sg(q)|^2;
    objective = sum(q_ste * dq) + s loss.  dC is what a learned table WOULD receive (the module freezes it)."""
    z64 = z.double().clone().requires_grad_(True)
    c64 = c.double().clone().requires_grad_(True)
    w64 = w.double().clone().requires_grad_(True)
    b64 = b.double().clone().requires_grad_(True) if b is not None else None
    e = c64 @ w64.T
    if b64 is not None:
        e = e + b64
    q = e[idx]
    q_ste = z64 + (q - z64).detach()
    loss = ((z64.detach() - q) ** 2).mean() + beta * ((z64 - q.detach()) ** 2).mean()
    obj = s * loss + ((q_ste * dq.double()).sum() if dq is not None else 0.0)
    grads = torch.autograd.grad(obj, [z64, w64, c64] + ([b64] if b64 is not None else []))
    return loss.detach(), grads[0], grads[1], (grads[3] if b64 is not None else None), grads[2]


def staged_f32(z, c, w, b, dq, beta: float, s: float = 1.0):
    """the definition and its backward in fp32 torch on the CPU: E by addmm, d = (|z|^2 + |E|^2) - 2 z.E, first minimum, gather, the
    closed forms in fp32 with the [K, D] scatter target and the D x K x D product of ops.simvq_staged.  Same expression sequence as the
    kernels up to the summation orders."""
    z, c, w = z.float(), c.float(), w.float()
    n, d = z.shape
    k = c.shape[0]
    e = torch.addmm(b.float(), c, w.T) if b is not None else c @ w.T
    dist = ((z * z).sum(1, keepdim=True) + (e * e).sum(1)[None, :]) - 2.0 * (z @ e.T)
    m = dist.min(1, keepdim=True).values
    idx = torch.argmax((dist == m).to(torch.uint8), dim=1)            # the FIRST minimum
    q = e[idx]
    sse = ((q - z) ** 2).sum()
    loss = sse * ((1.0 + beta) / (n * d))
    cz, ce = 2.0 * beta / (n * d), 2.0 / (n * d)
    dz = (z - q) * (s * cz)
    if dq is not None:
        dz = dz + dq.float()
    de = torch.zeros_like(e).index_add_(0, idx, q - z) * (s * ce)
    return dict(e=e, idx=idx, q=q, sse=sse, loss=loss, dz=dz, dw=de.T @ c, db=de.sum(0))


@functools.lru_cache(maxsize=None)
def reference(n: int, k: int, d: int, kind: str):
    """the free-running float64 forward of a case, computed once and shared (read-only)"""
    return forward(*make_case(n, k, d, kind))
