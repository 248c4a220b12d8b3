"""Inputs, float64 closed forms and the CPU restatement for the index-backpropagation (IBQ) quantizer tests (test_ibq_cpu.py,
test_gpu_ibq.py).  Conventions of attn_reference.py / simvq_reference.py.

Definition (include/vqk.h, "IBQ quantizer"), z [N, D], E [K, D], temperature T, commitment weight beta, loss cotangent s, decoder
gradient g on the output rows, c2 = 2 / (N D):
    S = z E^T / T, P = softmax_j S, lse, ebar = P E, idx = argmax_j S (the smallest index wins a tie), q = E[idx],
    loss = (2 + beta) / (N D) sum |q - z|^2,
    G = g + s c2 (q - z), delta = rowsum(G ebar), dS = P (G E^T - delta),
    dz = -2 s c2 (q - z) + dS E / T,   dE = scatter_idx(G + s beta c2 (q - z)) + dS^T z / T.
``literal`` states the published formulation for torch.autograd (Ind = hard - sg[P] + P, three loss terms); ``closed_form`` the
formulas above in float64 on given tokens (teacher forcing) -- on any device, so the GPU tests evaluate the large shapes there.

Tolerances are MEASURED: ``restate`` repeats the kernels' arithmetic on the CPU in fp32 -- every product a fixed k-ordered chain of
elementwise operations (attn_reference._chain_mm), index-ordered sums, the online softmax in the kernels' order of 64-code tiles with
the argmax carried beside the running maximum, exp / log through float64 -- and TABLE holds its distance to float64 per (kind, quantity)
in the metric max|got - want| / max|want|, the worst over TABLE_CASES, rounded up to two digits.  test_ibq_cpu.py re-measures the table;
the GPU tests allow 4x an entry (the kernels make the same roundings in another order).  Quantities that are mathematically zero are
measured against a neighbour's magnitude (``figures``)."""
import numpy as np
import torch

from tests.attn_reference import _chain_mm, _exp32, _log32, _row_sum, distance, one_thread

KINDS = ('normal', 'init', 'peaked', 'shifted', 'collapsed', 'scaled')
QUANTS = ('lse', 'ebar', 'dz', 'de')
SMALL_SHAPES = [(1, 64, 64), (65, 96, 64), (100, 40, 128), (64, 64, 256), (130, 200, 256)]
LARGE_SHAPES = [(2051, 1024, 256), (4096, 4096, 256)]
SHAPES = SMALL_SHAPES + LARGE_SHAPES            # (N, K, D) of the GPU tests
TEMPS = (1.0, 0.5)
STAGED_SHAPE = (40, 40, 48)                     # a D the fused kernels do not serve
MARGIN_KINDS = ('normal', 'init', 'scaled')     # the kinds whose rows must be separated (test_ibq_cpu.py checks the 99 % condition)
SEED_SALT = 1                                   # chosen so that the float64 reference alone meets the margin condition (test_ibq_cpu.py)
BETA = 0.25
SCALE = 0.7                                     # the loss cotangent s of the raw backward calls
# the cases the table is measured on: every kind at every small shape and both temperatures, and the 1024-code shape for 'normal'
# (the sums over 1024 codes and 2051 rows: the error of a longer sum, which the larger GPU shapes are held to as well)
TABLE_CASES = [(s, kind, t) for s in SMALL_SHAPES for kind in KINDS for t in TEMPS] + [((2051, 1024, 256), 'normal', 1.0)]

# worst restatement-vs-float64 figure over TABLE_CASES (test_ibq_cpu.py::test_table_bounds_restatement prints and checks every one)
TABLE = {
    ('normal', 'lse'): 2.9e-07,
    ('normal', 'ebar'): 1.6e-06,
    ('normal', 'dz'): 2e-06,
    ('normal', 'de'): 1.1e-06,
    ('init', 'lse'): 1.3e-07,
    ('init', 'ebar'): 4.7e-07,
    ('init', 'dz'): 5.7e-07,
    ('init', 'de'): 1.6e-07,
    ('peaked', 'lse'): 5.5e-07,
    ('peaked', 'ebar'): 1.4e-05,
    ('peaked', 'dz'): 0.00026,
    ('peaked', 'de'): 5.7e-05,
    ('shifted', 'lse'): 4.3e-07,
    ('shifted', 'ebar'): 1.6e-05,
    ('shifted', 'dz'): 9.7e-05,
    ('shifted', 'de'): 2.9e-05,
    ('collapsed', 'lse'): 3.1e-07,
    ('collapsed', 'ebar'): 9.8e-07,
    ('collapsed', 'dz'): 2.3e-06,
    ('collapsed', 'de'): 2.3e-07,
    ('scaled', 'lse'): 4.7e-07,
    ('scaled', 'ebar'): 1.8e-06,
    ('scaled', 'dz'): 2.3e-06,
    ('scaled', 'de'): 2.3e-06,
}


def shape_id(c):
    return f'N{c[0]}-K{c[1]}-D{c[2]}' + (f'-{c[3]}' if len(c) > 3 else '')


def make_case(n: int, k: int, d: int, kind: str):
    """(z [N, D], e [K, D], g [N, D]) as float64 tensors that are exact in fp32, from a seed of the shape and kind alone"""
    gen = torch.Generator().manual_seed(100003 * n + 101 * k + d + 7 * KINDS.index(kind) + SEED_SALT)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)       # noqa: E731
    z, e, g = rn(n, d), rn(k, d), rn(n, d)
    if kind == 'normal':                         # logits O(1)
        e = e / d ** 0.5
    elif kind == 'init':                         # the module's start: +- 1 / K, a near-uniform softmax
        e = (2.0 * torch.rand(k, d, generator=gen, dtype=torch.float64) - 1.0) / k
    elif kind == 'peaked':                       # logits to about +- 190: P is nearly hard
        sc = (50.0 / d ** 0.5) ** 0.5
        z, e = sc * z, sc * e
    elif kind == 'shifted':                      # a common offset on every code: every logit of a row moves by 0.5 sum(z_i) ~ D / 2
        e = e / d ** 0.5 + 0.5
        z = z + 1.0
    elif kind == 'collapsed':                    # 4 distinct codes repeated: the smallest index wins, P splits evenly
        e = (e[:4] / d ** 0.5)[torch.arange(k) % 4]
    elif kind == 'scaled':                       # code j times a slowly growing factor: a wrong tile pitch cannot pass
        e = e / d ** 0.5 * (1.0 + 0.5 * torch.arange(k, dtype=torch.float64) / k)[:, None]
    else:
        raise ValueError(kind)
    f32 = lambda t: t.to(torch.float32).to(torch.float64).contiguous()        # noqa: E731
    return f32(z), f32(e), f32(g)


def logits64(z, e, temperature: float = 1.0):
    return (z.double() @ e.double().t()) * (1.0 / temperature)


def eta(z, e, temperature: float = 1.0):
    """[N] the fp32 error bound of one logit of row i: a dot product of length D summed in any order, then one scaling --
    (D + 1) 2^-24 |z_i| max_j |e_j| / T  (rvq_reference.eta adapted from distances to logits)"""
    d = z.shape[1]
    return (d + 1) * 2.0 ** -24 * z.double().norm(dim=1) * float(e.double().norm(dim=1).max()) / temperature


def margins(z, e, temperature: float = 1.0):
    """float64: (S, best [N], argmax [N] (first), gap between the top two logits [N], 2 eta [N])"""
    s = logits64(z, e, temperature)
    top = torch.topk(s, min(2, s.shape[1]), dim=1).values
    best = top[:, 0]
    gap = top[:, 0] - top[:, 1] if s.shape[1] > 1 else torch.full_like(best, float('inf'))
    first = (s == best[:, None]).to(torch.int8).argmax(dim=1)
    return s, best, first, gap, 2.0 * eta(z, e, temperature).to(s.device)


def check_acceptance(z, e, idx, temperature: float = 1.0) -> float:
    """every token is accepted by float64 (its logit is within 2 eta of the maximum) and on rows whose top two logits are more than
    2 eta apart it IS the float64 argmax.  Returns the fraction of separated rows."""
    s, best, first, gap, eta2 = margins(z, e, temperature)
    chosen = s.gather(1, idx.view(-1, 1).to(s.device))[:, 0]
    bad = best - chosen > eta2
    assert not bool(bad.any()), f'{int(bad.sum())} tokens beyond 2 eta, worst excess / (2 eta) = {float(((best - chosen) / eta2).max()):.3g}'
    sep = gap > eta2
    wrong = sep & (idx.to(s.device) != first)
    assert not bool(wrong.any()), f'{int(wrong.sum())} separated rows off the float64 argmax'
    return float(sep.double().mean())


def closed_form(z, e, idx=None, g=None, s=None, beta: float = BETA, temperature: float = 1.0) -> dict:
    """the float64 oracle on the tokens ``idx`` (None: the float64 argmax, first maximum): idx, lse, ebar, q, loss, dz, de.  g / s None
    = absent.  A token outside [0, K) has no hard terms (q - z counts as zero everywhere)."""
    z, e = z.double(), e.double()
    n, d = z.shape
    k = e.shape[0]
    inv_t = 1.0 / temperature
    sl = (z @ e.t()) * inv_t
    if idx is None:
        idx = (sl == sl.max(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)
    idx = idx.to(z.device)
    lse = torch.logsumexp(sl, dim=1)
    p = torch.exp(sl - lse[:, None])
    ebar = p @ e
    ok = (idx >= 0) & (idx < k)
    q = e[idx.clamp(0, k - 1)]
    diff = torch.where(ok[:, None], q - z, torch.zeros_like(z))
    loss = (2.0 + beta) / (n * d) * (diff * diff).sum()
    sc2 = (0.0 if s is None else float(s)) * 2.0 / (n * d)
    gg = diff * sc2 + (g.double().to(z.device) if g is not None else 0.0)
    delta = (gg * ebar).sum(1, keepdim=True)
    ds = p * (gg @ e.t() - delta)
    dz = -2.0 * sc2 * diff + (ds @ e) * inv_t
    hard = torch.where(ok[:, None], gg + beta * sc2 * diff, torch.zeros_like(z))
    de = torch.zeros_like(e).index_add_(0, idx.clamp(0, k - 1), hard) + (ds.t() @ z) * inv_t
    return dict(idx=idx, lse=lse, ebar=ebar, q=q, loss=loss, dz=dz, de=de)


def literal(z, e, g, s: float, beta: float = BETA, temperature: float = 1.0) -> dict:
    """the published formulation, differentiated by torch.autograd in float64: Ind = hard - sg[P] + P, the output Ind E (its value is
    q), the three loss terms.  Returns loss, dz, de for the cotangents g on the output and s on the loss."""
    z = z.double().clone().requires_grad_(True)
    e = e.double().clone().requires_grad_(True)
    sl = (z @ e.t()) / temperature
    p = torch.softmax(sl, dim=1)
    idx = (sl == sl.max(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)
    hard = torch.nn.functional.one_hot(idx, e.shape[0]).to(torch.float64)
    ind = hard - p.detach() + p
    zq = ind @ e
    q = e[idx]
    loss = ((zq - z) ** 2).mean() + ((q.detach() - z) ** 2).mean() + beta * ((q - z.detach()) ** 2).mean()
    dz, de = torch.autograd.grad([zq, loss], [z, e], [g.double(), torch.tensor(float(s), dtype=torch.float64)])
    return dict(idx=idx, loss=loss.detach(), dz=dz, de=de)


def restate(z, e, g, s, beta: float = BETA, temperature: float = 1.0, tile: int = 64) -> dict:
    """the kernels' arithmetic on the CPU in fp32 (see the module docstring); results as float64 tensors (idx int64)"""
    with one_thread():
        z, e = z.to(torch.float32).contiguous(), e.to(torch.float32).contiguous()
        n, d = z.shape
        k = e.shape[0]
        inv_t = np.float32(1.0 / temperature)
        sl = _chain_mm(z, e.t().contiguous(), 1) * inv_t
        m = torch.full((n, 1), float('-inf'), dtype=torch.float32)
        l = torch.zeros((n, 1), dtype=torch.float32)
        acc = torch.zeros((n, d), dtype=torch.float32)
        idx = torch.zeros(n, dtype=torch.int64)
        for k0 in range(0, k, tile):                              # ascending tiles, strict >: the first maximum stays
            st = sl[:, k0:k0 + tile]
            mx = st.max(dim=1, keepdim=True).values
            first = torch.from_numpy(np.argmax(st.numpy(), axis=1)) + k0
            idx = torch.where((mx > m)[:, 0], first, idx)
            mn = torch.maximum(m, mx)
            alpha = _exp32(m - mn)
            p = _exp32(st - mn)
            l = l * alpha + _row_sum(p)
            acc = acc * alpha + _chain_mm(p, e[k0:k0 + tile].contiguous(), 1)
            m = mn
        lse = m + _log32(l)
        ebar = acc * (1.0 / l)
        q = e[idx]
        diff = q - z
        sse = _row_sum((diff * diff).reshape(1, -1))[0, 0]
        loss = sse * np.float32((2.0 + beta) / (n * d))
        ce = np.float32((0.0 if s is None else s) * 2.0 / (n * d))
        cz = np.float32((0.0 if s is None else s) * 2.0 * beta / (n * d))
        gg = diff * ce + (g.to(torch.float32) if g is not None else 0.0)
        hh = gg + diff * cz
        delta = _row_sum(gg * ebar)
        p = _exp32(sl - lse)
        ds = p * (_chain_mm(gg, e.t().contiguous(), 1) - delta)
        dz = diff * (np.float32(-2.0) * ce) + _chain_mm(ds, e, 1) * inv_t
        hard = torch.zeros((k, d), dtype=torch.float32)
        for i in range(n):                                        # the hard term in row order
            hard[idx[i]] += hh[i]
        de = _chain_mm(ds.t().contiguous(), z, 1) * inv_t + hard
    out = dict(lse=lse[:, 0], ebar=ebar, loss=loss, dz=dz, de=de)
    out = {name: t.to(torch.float64) for name, t in out.items()}
    out['idx'] = idx
    return out


def figures(got: dict, ref: dict, kind: str = '') -> dict:
    """figure per quantity of ``got`` against the float64 ``ref``: max|got - want| / max|want|.  A quantity that is mathematically zero
    (dz with one code and no loss cotangent: a constant softmax) is held to its neighbour's magnitude max|de|, an absolute check."""
    out = {}
    for name in QUANTS:
        if name not in got:
            continue
        norm = float(ref[name].abs().max())
        if norm < 1e-30:
            norm = float(ref['de'].abs().max())
        out[name] = distance(got[name], ref[name], norm)
    return out


def measure(case) -> dict:
    """the restatement's figures for one of TABLE_CASES, teacher-forced on the restatement's own tokens: the worse of the decoder's
    gradient present and absent (the small shapes; the large one is measured with it)"""
    (n, k, d), kind, t = case
    z, e, g = make_case(n, k, d, kind)
    out = {}
    for gg in ((g, None) if (n, k, d) in SMALL_SHAPES else (g,)):
        r = restate(z, e, gg, SCALE, BETA, t)
        ref = closed_form(z, e, r['idx'], gg, SCALE, BETA, t)
        for name, fig in figures(r, ref, kind).items():
            out[name] = max(out.get(name, 0.0), fig)
    return out


def bound(kind: str, quant: str) -> float:
    return TABLE[(kind, quant)]


def roundup(x: float) -> float:
    """x rounded up to two significant digits"""
    if x <= 0.0:
        return 0.0
    e = int(np.floor(np.log10(x))) - 1
    return float(np.ceil(x / 10.0 ** e) * 10.0 ** e)


def hist(idx, k: int):
    return torch.bincount(idx.view(-1).cpu(), minlength=k)
