"""Inputs, float64 closed forms and CPU restatements for the self-attention tests (test_attn_cpu.py, test_gpu_attn.py).

The oracle is the float64 closed form below (the project this one was modelled on has no attention):
    S = scale q k^T, lse = logsumexp_j S, P = exp(S - lse), o = P v,
    delta = rowsum(do * o), dv = P^T do, dS = P * (do v^T - delta), dq = scale dS k, dk = scale dS^T q.

Tolerances are MEASURED: ``restate`` repeats the kernels' arithmetic on the CPU -- every product as a fixed k-ordered chain of
elementwise fp32 operations (``_chain_mm``: no GEMM, so the figures do not depend on the host's BLAS or thread count), on one intra-op
thread, exp / log / sqrt evaluated in float64 and rounded once (the vectorised fp32 routines differ between CPU instruction sets);
the AttnBlock restatement (``block_forward``) is built the same way, its backward included (``_ChainMM``, ``_OrderedSum``, ``_Bcast``:
autograd never runs a GEMM or a reduction of its own).  fp32: fp32 throughout; bf16: bf16-rounded inputs, fp32 logits and statistics, P (and dS) rounded to bf16 only as matrix operands, fp32 accumulation, outputs rounded to bf16 once, delta
from the rounded o -- and its distance to float64 (on the same, for bf16 the rounded, inputs) in the metric max|got - want| / max|want|
is what TABLE / BLOCK_TABLE hold, the worst over the shapes per (kind, quantity, dtype), rounded up to two digits.  test_attn_cpu.py
asserts that the tables still bound what it measures (they cannot drift from the code); the GPU tests allow 4x an entry: the kernels
make the same roundings in another order (tile walk, MFMA accumulation order, online rescaling, the device's exp).
``constant`` dq is mathematically zero (reference ~1e-16): its figure is max|dq| / max|dk|, an absolute value, not a relative error.
The lse entry uses the same metric (max|lse| is 3 to 330)."""
import numpy as np
import torch

# (B, H, W, heads, d)
SHAPES = [(3, 1, 1, 1, 64), (2, 8, 8, 1, 64), (2, 5, 13, 1, 64), (2, 10, 10, 2, 64), (1, 16, 16, 1, 512), (1, 33, 32, 1, 128),
          (1, 16, 16, 4, 128)]
STAGED_SHAPES = [(2, 6, 7, 2, 32), (1, 9, 8, 1, 96)]          # head dims the fused kernels do not serve
KINDS = ('scale1', 'peaked', 'shifted', 'constant')
QUANTS = ('o', 'lse', 'dq', 'dk', 'dv')
DTYPES = ('fp32', 'bf16')

# worst restatement-vs-float64 figure over SHAPES (test_attn_cpu.py::test_table_bounds_restatement prints and checks every one).
# Some bf16 entries are wide once multiplied by 4 -- ``shifted`` dq 0.071 (28 % of max|dq|: the common offset of 330 makes dS a
# difference of rounded terms), the block's q.weight 0.032 (13 %) -- and would let a wrong tile of THAT case through; the same code path
# (one template, the storage type changes only the MFMA and the roundings) is held to 1e-6 ... 4e-5 by the fp32 rows of the same cases,
# and the bf16 figures measured on the device sit at the restatement's own value (a quarter of the bound).
TABLE = {
    ('scale1', 'o', 'fp32'): 1.6e-06,
    ('scale1', 'lse', 'fp32'): 2.3e-07,
    ('scale1', 'dq', 'fp32'): 1.5e-06,
    ('scale1', 'dk', 'fp32'): 1.5e-06,
    ('scale1', 'dv', 'fp32'): 1.8e-06,
    ('peaked', 'o', 'fp32'): 2.1e-05,
    ('peaked', 'lse', 'fp32'): 6.8e-07,
    ('peaked', 'dq', 'fp32'): 3.7e-05,
    ('peaked', 'dk', 'fp32'): 3.8e-05,
    ('peaked', 'dv', 'fp32'): 1e-05,
    ('shifted', 'o', 'fp32'): 3.5e-05,
    ('shifted', 'lse', 'fp32'): 4.1e-07,
    ('shifted', 'dq', 'fp32'): 4.4e-05,
    ('shifted', 'dk', 'fp32'): 2.4e-05,
    ('shifted', 'dv', 'fp32'): 2.2e-05,
    ('constant', 'o', 'fp32'): 5.6e-07,
    ('constant', 'lse', 'fp32'): 1.8e-07,
    ('constant', 'dq', 'fp32'): 2.2e-06,
    ('constant', 'dk', 'fp32'): 1.2e-06,
    ('constant', 'dv', 'fp32'): 8e-07,
    ('scale1', 'o', 'bf16'): 0.0032,
    ('scale1', 'lse', 'bf16'): 2.3e-07,
    ('scale1', 'dq', 'bf16'): 0.0036,
    ('scale1', 'dk', 'bf16'): 0.0039,
    ('scale1', 'dv', 'bf16'): 0.0039,
    ('peaked', 'o', 'bf16'): 0.0023,
    ('peaked', 'lse', 'bf16'): 3.2e-07,
    ('peaked', 'dq', 'bf16'): 0.0081,
    ('peaked', 'dk', 'bf16'): 0.0084,
    ('peaked', 'dv', 'bf16'): 0.0033,
    ('shifted', 'o', 'bf16'): 0.0033,
    ('shifted', 'lse', 'bf16'): 8.4e-08,
    ('shifted', 'dq', 'bf16'): 0.071,
    ('shifted', 'dk', 'bf16'): 0.0058,
    ('shifted', 'dv', 'bf16'): 0.0037,
    ('constant', 'o', 'bf16'): 0.003,
    ('constant', 'lse', 'bf16'): 9.5e-08,
    ('constant', 'dq', 'bf16'): 0.006,
    ('constant', 'dk', 'bf16'): 0.0035,
    ('constant', 'dv', 'bf16'): 0.0028,
}
# AttnBlock: (dtype, quantity) -> worst figure over BLOCK_CASES
BLOCK_CASES = [(2, 64, 8, 8, 1), (2, 128, 10, 10, 2)]         # (B, C, H, W, heads)
BLOCK_PARAMS = ('norm.weight', 'norm.bias', 'q.weight', 'q.bias', 'k.weight', 'k.bias', 'v.weight', 'v.bias', 'proj_out.weight',
                'proj_out.bias')
BLOCK_TABLE = {
    ('fp32', 'out'): 1.4e-06,
    ('fp32', 'dx'): 1.9e-06,
    ('fp32', 'norm.weight'): 2.1e-06,
    ('fp32', 'norm.bias'): 1.9e-06,
    ('fp32', 'q.weight'): 2.1e-06,
    ('fp32', 'q.bias'): 2e-06,
    ('fp32', 'k.weight'): 1.5e-06,
    ('fp32', 'k.bias'): 9.7e-07,
    ('fp32', 'v.weight'): 1.2e-06,
    ('fp32', 'v.bias'): 5.7e-07,
    ('fp32', 'proj_out.weight'): 1.4e-06,
    ('fp32', 'proj_out.bias'): 3.1e-08,
    ('bf16', 'out'): 0.0094,
    ('bf16', 'dx'): 0.02,
    ('bf16', 'norm.weight'): 0.015,
    ('bf16', 'norm.bias'): 0.019,
    ('bf16', 'q.weight'): 0.032,
    ('bf16', 'q.bias'): 0.012,
    ('bf16', 'k.weight'): 0.018,
    ('bf16', 'k.bias'): 0.0056,
    ('bf16', 'v.weight'): 0.0071,
    ('bf16', 'v.bias'): 0.0034,
    ('bf16', 'proj_out.weight'): 0.0088,
    ('bf16', 'proj_out.bias'): 3.1e-08,
}


def shape_id(s):
    return 'B%d-%dx%d-h%d-d%d' % s


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def make_inputs(shape, kind: str, dtype: str = 'fp32') -> dict:
    """q, k, v, do as float64 [B, N, heads * d] tensors (exact in ``dtype``), computed from a seed of the shape alone"""
    b, h, w, heads, d = shape
    n, c = h * w, heads * d
    g = torch.Generator().manual_seed(1000 * n + 10 * c + b)
    q, k, v, do = (torch.randn(b, n, c, generator=g, dtype=torch.float64) for _ in range(4))
    if kind == 'peaked':
        q, k = 6.0 * q, 6.0 * k
    elif kind == 'shifted':
        k = k + 40.0 * torch.sign(q.mean(dim=1, keepdim=True))
        q = q + 3.0
    elif kind == 'constant':
        k = k[:, :1].expand(b, n, c).clone()
    elif kind != 'scale1':
        raise ValueError(kind)
    out = dict(q=q, k=k, v=v, do=do)
    rnd = bf16_round if dtype == 'bf16' else (lambda t: t.to(torch.float32).to(torch.float64))
    return {name: rnd(t).contiguous() for name, t in out.items()}


def _heads(t, heads):
    b, n, c = t.shape
    return t.reshape(b, n, heads, c // heads).permute(0, 2, 1, 3)


def _rows(t):
    b, h, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, n, h * d)


def closed_form(q, k, v, do, heads: int, scale=None) -> dict:
    """the float64 oracle: o, lse [B, heads, N], dq, dk, dv"""
    q, k, v, do = (_heads(t.to(torch.float64), heads) for t in (q, k, v, do))
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    s = scale * (q @ k.transpose(-1, -2))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    delta = (do * o).sum(-1, keepdim=True)
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - delta)
    dq = scale * (ds @ k)
    dk = scale * (ds.transpose(-1, -2) @ q)
    return dict(o=_rows(o), lse=lse, dq=_rows(dq), dk=_rows(dk), dv=_rows(dv))


class one_thread:
    """the measurement runs on ONE intra-op thread: torch's CPU reductions and GEMMs split their sums by the thread count, and a table
    entry must not depend on the host's"""

    def __enter__(self):
        self.prev = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.prev)


def _chain_mm(a, b, step: int):
    """a [.., M, K] @ b [.., K, N] in fp32 as a FIXED chain of elementwise operations, no GEMM: the products of ``step`` consecutive k
    are added in k order and that group is added to the accumulator -- the chain an MFMA accumulator runs (fp32: one product per
    v_mfma_f32_32x32x2_f32 step; bf16: the 16 products of one 32x32x16 instruction), every product and every sum rounded once.  The
    same bits on every host and thread count, which a blocked CPU GEMM does not give."""
    kk = a.shape[-1]
    acc = torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=torch.float32)
    part, tmp = torch.empty_like(acc), torch.empty_like(acc)
    for c0 in range(0, kk, step):
        torch.mul(a[..., c0:c0 + 1], b[..., c0:c0 + 1, :], out=part)
        for c in range(c0 + 1, min(c0 + step, kk)):
            torch.mul(a[..., c:c + 1], b[..., c:c + 1, :], out=tmp)
            part.add_(tmp)
        acc.add_(part)
    return acc


def _exp32(t):
    """exp / log evaluated in float64 and rounded once to fp32: the vectorised fp32 routines differ in the last bit between CPU
    instruction sets, the rounded float64 value does not"""
    return torch.exp(t.to(torch.float64)).to(torch.float32)


def _log32(t):
    return torch.log(t.to(torch.float64)).to(torch.float32)


def _row_sum(t):
    """sum over the last dim in index order (elementwise adds: no host-dependent reduction tree)"""
    acc = t[..., 0:1].clone()
    for c in range(1, t.shape[-1]):
        acc.add_(t[..., c:c + 1])
    return acc


def restate(q, k, v, do, heads: int, dtype: str, scale=None) -> dict:
    """the kernels' arithmetic on the CPU (see the module docstring); results as float64 tensors"""
    lo = dtype == 'bf16'
    step = 16 if lo else 1
    r = (lambda t: t.to(torch.bfloat16).to(torch.float32)) if lo else (lambda t: t)
    with one_thread():
        q, k, v, do = (_heads(t.to(torch.float32), heads).contiguous() for t in (q, k, v, do))
        scale = q.shape[-1] ** -0.5 if scale is None else scale
        tr = lambda t: t.transpose(-1, -2).contiguous()           # noqa: E731
        s = _chain_mm(q, tr(k), step) * scale                     # fp32 products and sums of the (bf16-exact) inputs: never a bf16 matmul
        m = s.max(dim=-1, keepdim=True).values
        e = _exp32(s - m)
        l = _row_sum(e)
        o = r(_chain_mm(r(e), v, step) / l)
        lse = (m + _log32(l))
        p = _exp32(s - lse)
        delta = _row_sum(do * o)
        dv = r(_chain_mm(tr(r(p)), do, step))
        ds = p * (_chain_mm(do, tr(v), step) - delta)
        dq = r(scale * _chain_mm(r(ds), k, step))
        dk = r(scale * _chain_mm(tr(r(ds)), q, step))
    return {name: t.to(torch.float64) for name, t in dict(o=_rows(o), lse=lse[..., 0], dq=_rows(dq), dk=_rows(dk), dv=_rows(dv)).items()}


def distance(got, want, norm=None) -> float:
    got, want = torch.as_tensor(got).to(torch.float64), torch.as_tensor(want).to(torch.float64)
    norm = float(want.abs().max()) if norm is None else float(norm)
    return float((got - want).abs().max()) / max(norm, 1e-300)


def figures(got: dict, ref: dict, kind: str) -> dict:
    """figure per quantity of ``got`` against the float64 ``ref``.  Quantities that are mathematically zero (reference ~1e-16) are held
    to a neighbour's magnitude, an absolute check: ``constant`` dq to max|dk|; with one key (N = 1) dq and dk to max|dv|"""
    out = {}
    one_key = ref['lse'].shape[-1] == 1
    for name in QUANTS:
        if name not in got:
            continue
        norm = None
        if one_key and name in ('dq', 'dk'):
            norm = float(ref['dv'].abs().max())
        elif kind == 'constant' and name == 'dq':
            norm = float(ref['dk'].abs().max())
        out[name] = distance(got[name], ref[name], norm)
    return out


def block_figures(got: dict, ref: dict) -> dict:
    """the same for the block; the gradient of k.bias is mathematically zero (a constant added to every logit of a row): held to
    max|d q.bias|"""
    return {k: distance(got[k], ref[k], float(ref['q.bias'].abs().max()) if k == 'k.bias' else None) for k in ref if k in got}


def bound(kind: str, quant: str, dtype: str) -> float:
    return TABLE[(kind, quant, dtype)]


# ---------------------------------------------------------------------------------------------- AttnBlock
class _RoundBoth(torch.autograd.Function):
    """bf16 storage of an activation: the value is rounded on the way forward, its gradient on the way back"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class _RoundFwd(torch.autograd.Function):
    """a parameter packed to bf16 for the matrix pipe: its gradient stays fp32"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def _ordered_sum_to(g, shape):
    """g summed down to ``shape`` (same rank, ones where it was broadcast) by index-ordered elementwise adds"""
    for d, n in enumerate(shape):
        if n == 1 and g.shape[d] > 1:
            acc = g.narrow(d, 0, 1).clone()
            for i in range(1, g.shape[d]):
                acc.add_(g.narrow(d, i, 1))
            g = acc
    return g


class _ChainMM(torch.autograd.Function):
    """a @ b and its two gradient products as ``_chain_mm`` chains: no GEMM on the way forward or back"""

    @staticmethod
    def forward(ctx, a, b, step):
        ctx.save_for_backward(a, b)
        ctx.step = step
        return _chain_mm(a, b, step)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return _chain_mm(g, b.transpose(-1, -2), ctx.step), _chain_mm(a.transpose(-1, -2), g, ctx.step), None


class _OrderedSum(torch.autograd.Function):
    """sum over the last dim (kept) in index order"""

    @staticmethod
    def forward(ctx, t):
        ctx.n = t.shape[-1]
        return _row_sum(t)

    @staticmethod
    def backward(ctx, g):
        return g.expand(*g.shape[:-1], ctx.n).clone()


class _Bcast(torch.autograd.Function):
    """explicit broadcast: autograd never reduces a gradient with a host-dependent sum, the way back is ``_ordered_sum_to``"""

    @staticmethod
    def forward(ctx, t, shape):
        ctx.shape = t.shape
        return t.expand(shape).clone()

    @staticmethod
    def backward(ctx, g):
        return _ordered_sum_to(g, ctx.shape), None


class _Exp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        y = _exp32(t)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


def make_block(case) -> dict:
    """x, dy [B, C, H, W] and the ten parameters of an AttnBlock as float64 tensors, exact in bf16 (so one set serves both dtypes)"""
    b, c, h, w, heads = case
    g = torch.Generator().manual_seed(7 * c + h)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)       # noqa: E731
    p = {'x': rn(b, c, h, w), 'dy': rn(b, c, h, w), 'norm.weight': 1.0 + 0.2 * rn(1, c, 1, 1), 'norm.bias': 0.2 * rn(1, c, 1, 1)}
    for name in ('q', 'k', 'v', 'proj_out'):
        p[name + '.weight'] = rn(c, c, 1, 1) * (2.0 if name in ('q', 'k') else 1.0) / c ** 0.5
        p[name + '.bias'] = 0.1 * rn(c)
    return {k: bf16_round(t) for k, t in p.items()}


def block_forward(x, p: dict, heads: int, mode: str):
    """AttnBlock in torch: x + proj_out(attention(q(h), k(h), v(h))), h = GroupNorm(32, eps 1e-6, unbiased variance)(x).
    mode 'f64': plain torch (the oracle).  'fp32' / 'bf16': the restatement -- every product a ``_chain_mm`` chain forward and back,
    every reduction and every reduced gradient an index-ordered sum, exp through float64, so that no figure depends on the host's
    BLAS, thread count or vector instruction set; 'bf16' adds bf16 storage between the operators and bf16 matrix operands."""
    b, c, hh, ww = x.shape
    n = hh * ww
    scale = (c // heads) ** -0.5
    if mode == 'f64':
        xg = x.reshape(b, 32, -1)
        mean, var = xg.mean(-1, keepdim=True), xg.var(-1, keepdim=True)
        hn = ((xg - mean) / torch.sqrt(var + 1e-6)).reshape(b, c, hh, ww) * p['norm.weight'] + p['norm.bias']
        rows = hn.permute(0, 2, 3, 1).reshape(b, n, c)
        lin = lambda t, name: t @ p[name + '.weight'].reshape(c, c).t() + p[name + '.bias']       # noqa: E731
        q, k, v = (_heads(lin(rows, name), heads) for name in ('q', 'k', 'v'))
        a = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v
        y = lin(_rows(a), 'proj_out') + x.permute(0, 2, 3, 1).reshape(b, n, c)
        return y.reshape(b, hh, ww, c).permute(0, 3, 1, 2)
    lo = mode == 'bf16'
    step = 16 if lo else 1
    act = _RoundBoth.apply if lo else (lambda t: t)
    par = _RoundFwd.apply if lo else (lambda t: t)
    bc = _Bcast.apply
    xg = x.reshape(b, 32, -1)
    cnt = xg.shape[-1]
    xc = xg - bc(_OrderedSum.apply(xg) / cnt, xg.shape)
    var = _OrderedSum.apply(xc * xc) / (cnt - 1)
    rstd = 1.0 / torch.sqrt((var + 1e-6).to(torch.float64)).to(torch.float32)      # (sqrt through float64, like exp)
    xn = (xc * bc(rstd, xg.shape)).reshape(b, c, hh, ww)
    hn = act(xn * bc(p['norm.weight'], x.shape) + bc(p['norm.bias'], x.shape))
    rows = hn.permute(0, 2, 3, 1).reshape(b * n, c)

    def lin(t, name):
        w = par(p[name + '.weight']).reshape(c, c).t()
        return _ChainMM.apply(t, w, step) + bc(p[name + '.bias'].reshape(1, c), (b * n, c))
    q, k, v = (_heads(act(lin(rows, name)).reshape(b, n, c), heads) for name in ('q', 'k', 'v'))
    s = _ChainMM.apply(q, k.transpose(-1, -2), step) * scale
    e = _Exp.apply(s - s.max(dim=-1, keepdim=True).values.detach())
    a = act(_ChainMM.apply(act(e), v, step) / bc(_OrderedSum.apply(e), v.shape))
    y = act(lin(_rows(a).reshape(b * n, c), 'proj_out') + x.permute(0, 2, 3, 1).reshape(b * n, c))
    return y.reshape(b, hh, ww, c).permute(0, 3, 1, 2)


def block_eval(case, mode: str) -> dict:
    """out, dx and the ten parameter gradients of the block of ``case`` in ``mode``, as float64 tensors"""
    heads = case[4]
    dt = torch.float64 if mode == 'f64' else torch.float32
    p = {k: t.to(dt).requires_grad_(k != 'dy') for k, t in make_block(case).items()}
    with one_thread():
        y = block_forward(p['x'], p, heads, mode)
        y.backward(p['dy'])
    out = {'out': y.detach(), 'dx': p['x'].grad}
    out.update({k: p[k].grad for k in BLOCK_PARAMS})
    return {k: t.to(torch.float64) for k, t in out.items()}


def np64(t):
    return np.asarray(t.detach().cpu().to(torch.float64))
