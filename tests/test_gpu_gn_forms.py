"""Every code path of the GroupNorm(+SiLU) kernels (csrc/norm.hip) against float64, at both sides of each dispatch guard.

The library picks a form from the map shape, the dtype, the workspace size, four tuning slots and the deterministic switch:
  forward   single-kernel small form (gn_small_fwd_kernel, 1 / 2 / 4 / 8 / 16 pixels per thread: gn_small_ppt)
            or statistics + finalize-and-apply (gn_stats_kernel, gn_apply_fin_kernel; deterministic: block partials)
  backward  small form (gn_small_bwd_kernel, <= 8 pixels per thread; deterministic: per-sample channel partials)
            or cluster form (gn_cluster_bwd_kernel, 64- / 32-channel slices, hw <= GN_CLUSTER_MAX_HW)
            or reduce + apply (gn_bwd_reduce_kernel, gn_bwd_apply_kernel; NT loads at >= GN_NT_MB MiB; addend none / same
            resolution / half resolution; dx column sums; deterministic: group and channel partials)
  plus the separate entry points (vqk_gn_stats, vqk_gn_apply) and the presummed forwards (vqk_gn_forward_presummed[_parts]).
Each case forces its form through the tuning slots (``_CFG``), mirrors the host's choice in Python (``_forms``: the case id
names the form that ran) and checks y, the returned (mean, rstd), dx, dW, dB (accumulated onto non-zero values: a kernel that
stores instead of adding fails) and the stream's GroupNorm workspace (zero on exit).  The reference restates
vqvae/modules/autoencoder.py:25-39: per-(sample, group) mean, UNBIASED torch.var, eps 1e-6, affine, optional SiLU, differentiated
by float64 autograd on the inputs as the kernel sees them (bf16 mode: the bf16-rounded x, dy and addend), on the device.

Error measures (``_errors``): fp32 y / dx: max |got - ref| / max |ref|; bf16 y / dx: the worst element in units of one bf16 rounding
(tests/test_gpu_conv_edges.py::_check_bf16: 2^-8 * (|ref| + mean |ref|)) and the relative norm; dW / dB / dx column sums:
relative norm; mean: max |got - ref| * rstd_ref (units of the group's standard deviation); rstd: max relative error.

Measured worst errors over all cases of this file on MI355X, and the bounds (_BOUNDS: about 10x the worst; the bf16 per-element
rule is fixed at one rounding):
            measure    small1/2/4/8/16   cluster   two-kernel   NT        worst    bound
  fp32      y          1.0e-7 .. 1.5e-7  -         1.9e-7       -         1.9e-7   2e-6
            dx         1.8e-7 .. 2.6e-7  3.0e-7    4.6e-7       4.6e-7    4.6e-7   5e-6
            dW / dB    0.9e-7 .. 1.5e-7  1.9e-7    4.8e-7       4.3e-7    4.9e-7   5e-6   (dx column sums 4.7e-7, 5e-6)
            mean/rstd                                                     1.1e-7 / 1.9e-7   1e-6 / 2e-6
  bf16      y, dx      0.83 .. 0.90      0.90      0.94         0.91      0.94     1 rounding (relative norm 1.8e-3, 3e-3)
            dW / dB    1.0e-7 .. 2.0e-7  1.9e-7    7.0e-7       7.1e-7    7.1e-7   7e-6 / 5e-6   (column sums 4.8e-7, 5e-6)
            mean/rstd                                                     2.3e-8 / 5.6e-7   3e-7 / 6e-6
Deterministic forms, the presummed forwards and the separate entry points fall inside the same ranges.
Large mean (fp32, 32 x 128 @ 256^2, 512 pixels per thread in fp32): the statistics are raw moments, the variance error grows
like (mu / sigma)^2 -- measured about 1.1e-7 * (mu / sigma)^2 relative.  mu / sigma = 8: rstd 3.5e-6, y 2.3e-6, dx 2.3e-6
(bound 1e-5, fp32 grade); mu / sigma = 140: rstd 1.2e-3, y 7.6e-4, dx 7.1e-4, dW 3.0e-4 (bound 2e-3, as
test_gpu_ops.py::test_group_norm_large_mean_fp32).  The same conditioning shows on groups of two elements (a 1 x 1 map with
2 channels per group): two close values lose the fp32 sum of squares (rstd off by up to 3e-2), so the 1 x 1 cases use
8 channels per group.
"""
import contextlib
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
native = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd._native')
DEV, F32, BF, CL = 'cuda:0', torch.float32, torch.bfloat16, torch.channels_last
EPS = 1e-6
BF_EPS = 2.0 ** -8
GN_DEPTH = 5                                    # csrc/norm.hip: loads in flight per tensor in the streaming passes

# tuning slots that force one form (include/vqk.h: vqk_set_tuning)
_CFG = {
    'default': {},
    'cluster': {'GN_NO_SMALL': 1, 'GN_CLUSTER_MAX_HW': 1 << 20},
    'two': {'GN_NO_SMALL': 1, 'GN_CLUSTER_MAX_HW': 0, 'GN_NT_MB': 1 << 20},
    'nt': {'GN_NO_SMALL': 1, 'GN_CLUSTER_MAX_HW': 0, 'GN_NT_MB': 0},
}

# error bounds per dtype and measure (module docstring)
_BOUNDS = {
    F32: dict(y=2e-6, dx=5e-6, dw=5e-6, db=5e-6, colsum=5e-6, mean=1e-6, rstd=2e-6),
    BF: dict(y=1.0, y_rel=3e-3, dx=1.0, dx_rel=3e-3, dw=7e-6, db=5e-6, colsum=5e-6, mean=3e-7, rstd=6e-6),
}


def _check(what, err, bound):
    assert err < bound, (what, err, bound)


@contextlib.contextmanager
def _tuned(slots):
    lib = native.lib()
    try:
        for k, v in slots.items():
            native.check(lib.vqk_set_tuning(k.encode(), int(v)), 'set_tuning')
        yield
    finally:
        lib.vqk_reset_tuning()


@contextlib.contextmanager
def _deterministic(on):
    if not on:
        yield
        return
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------ the host's choice, restated
def _small_ppt(dt, hw, c, groups, max_ppt, slots):
    """csrc/norm.hip: gn_small_ppt"""
    if slots.get('GN_NO_SMALL', 0) or c % 32 or 32 % (c // groups):
        return 0
    rows = 32 if dt == F32 else 64
    if hw % rows:
        return 0
    ppt = hw // rows
    return ppt if ppt in (1, 2, 4, 8, 16) and ppt <= max_ppt else 0


def _forms(dt, n, c, h, w, groups, slots, det=False, mode='plain', colsum=False):
    """(forward form, backward form) that vqk_gn_forward / gn_backward_impl take for this problem"""
    hw, cpg = h * w, c // groups
    p = _small_ppt(dt, hw, c, groups, 16, slots)
    fwd = f'small{p}' if p else 'two'
    p = 0 if (mode == 'pooled' or colsum) else _small_ppt(dt, hw, c, groups, 8, slots)
    if p:
        return fwd, f'small{p}'
    v = 4 if dt == F32 else 8
    sl = 64 if (c % 64 == 0 and 64 % cpg == 0) else 32
    rows = 256 // (sl // v)
    if (not det and not colsum and hw <= slots.get('GN_CLUSTER_MAX_HW', 1024) and c % sl == 0 and sl % cpg == 0
            and hw % (8 * rows) == 0 and (mode != 'pooled' or w % 2 == 0)):
        return fwd, f'cluster{sl}'
    nt = n * hw * c * (4 if dt == F32 else 2) >= (slots.get('GN_NT_MB', 192) << 20)
    return fwd, 'nt' if nt else 'two'


def _pick_ppb(n, hw, total):
    """csrc/norm.hip: pick_ppb with the block total given"""
    bps = (total + n - 1) // n
    return max(64, (hw + bps - 1) // bps)


# ------------------------------------------------------------------------------------------ data, reference, kernels
def _data(dt, n, c, h, w, mode, seed, mu=0.0, sigma=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    x = (rnd(n, c, h, w) * sigma + mu).to(dt).contiguous(memory_format=CL)
    dy = rnd(n, c, h, w).to(dt).contiguous(memory_format=CL)
    wt, bs = rnd(c) * 0.5 + 1.0, rnd(c) * 0.5
    add = None
    if mode in ('add', 'acc'):
        add = rnd(n, c, h, w).to(dt).contiguous(memory_format=CL)
    elif mode == 'pooled':
        add = rnd(n, c, h // 2, w // 2).to(dt).contiguous(memory_format=CL)
    return x, dy, wt, bs, add


def _ref(x, dy, wt, bs, add, groups, silu, mode='plain'):
    """float64 restatement of autoencoder.py:25-39 (+ SiLU) and its autograd: y, mean, rstd [N, G], dx (+ addend), dW, dB"""
    n, c, h, w = x.shape
    xd = x.double().requires_grad_(True)
    wd, bd = wt.double().requires_grad_(True), bs.double().requires_grad_(True)
    xg = xd.reshape(n, groups, -1)
    mean, var = xg.mean(-1, keepdim=True), xg.var(-1, keepdim=True)           # torch.var: unbiased (autoencoder.py:33)
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = ((xg - mean) * rstd).reshape(n, c, h, w) * wd.view(1, -1, 1, 1) + bd.view(1, -1, 1, 1)
    if silu:
        y = torch.nn.functional.silu(y)
    y.backward(dy.double())
    dx = xd.grad
    if mode in ('add', 'acc'):
        dx = dx + add.double()
    elif mode == 'pooled':
        dx = dx + 0.25 * add.double().repeat_interleave(2, 2).repeat_interleave(2, 3)
    return dict(y=y.detach(), mean=mean.detach().reshape(n, groups), rstd=rstd.detach().reshape(n, groups), dx=dx,
                dw=wd.grad, db=bd.grad)


def _prefill(c, seed):
    return torch.randn(c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _ws_zero(what):
    ws = ops._gn_ws(torch.device(DEV), 0)
    torch.cuda.synchronize()
    nz = int((ws != 0).sum())
    assert nz == 0, (what, nz)


def _run(x, dy, wt, bs, add, groups, silu, mode='plain', colsum=False):
    """vqk_gn_forward, then the backward entry point of `mode`; dW / dB / column sums accumulate onto non-zero values"""
    n, c, h, w = x.shape
    ops._gn_ws(x.device, ops._gn_ws_doubles(n, c, groups))        # (sized before the first call: one buffer for all of them)
    _ws_zero('workspace dirty on entry')
    y, st = ops.raw_gn_forward(x, wt, bs, groups, EPS, silu)
    dw0, db0, cs0 = _prefill(c, 1), _prefill(c, 2), _prefill(c, 3)
    dw, db, cs = dw0.clone(), db0.clone(), cs0.clone()
    if mode == 'pooled':
        dx = ops.raw_gn_backward_pooled_add(x, st, wt, bs, dy, groups, silu, dw, db, add, 0.25, cluster_ok=True)
    elif mode == 'acc':                                            # accumulate = 1, no addend: dx += result
        dx = add.clone()
        red = ops._gn_ws(x.device, 0)
        native.check(native.lib().vqk_gn_backward_ws(ops.dcode(x.dtype), x.data_ptr(), st.data_ptr(), wt.data_ptr(), bs.data_ptr(),
                                                     dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), red.data_ptr(),
                                                     red.numel(), n, h, w, c, groups, int(silu), 1, None, None, 1.0,
                                                     ops._stream()), 'gn_backward_ws')
    else:
        dx, _, _ = ops.raw_gn_backward(x, st, wt, bs, dy, groups, silu, dw, db, add=add if mode == 'add' else None,
                                       dx_colsum=cs if colsum else None, cluster_ok=True)
    _ws_zero('workspace not zero after the backward')
    out = dict(y=y, stats=st, dx=dx, dw=dw.double() - dw0.double(), db=db.double() - db0.double())
    if colsum:
        out['colsum'] = cs.double() - cs0.double()
    return out


def _relnorm(a, r):
    return float((a.double() - r).norm() / (r.norm() + 1e-300))


def _errors(dt, got, ref):
    out = {}
    for k in ('y', 'dx'):
        a, r = got[k].double(), ref[k]
        if dt == F32:
            out[k] = float((a - r).abs().max() / r.abs().max())
        else:
            out[k] = float(((a - r).abs() / (BF_EPS * (r.abs() + r.abs().mean()))).max())
            out[k + '_rel'] = _relnorm(a, r)
    for k in ('dw', 'db'):
        out[k] = _relnorm(got[k], ref[k])
    if 'colsum' in got:
        out['colsum'] = _relnorm(got['colsum'], ref['dx'].sum((0, 2, 3)))
    st = got['stats'].view(ref['mean'].shape + (2,)).double()
    out['mean'] = float(((st[..., 0] - ref['mean']).abs() * ref['rstd']).max())
    out['rstd'] = float(((st[..., 1] - ref['rstd']).abs() / ref['rstd']).max())
    return out


def _check_all(dt, got, ref, bounds=None, what=''):
    b = dict(_BOUNDS[dt], **(bounds or {}))
    for k, e in _errors(dt, got, ref).items():
        _check(f'{what}{k}', e, b[k])


def _same_bits(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------ the case table
def _shapes():
    """(dtype, n, c, h, w, groups, mode, silu, slots-extra)"""
    s = []
    for dt, rows in ((F32, 32), (BF, 64)):
        # small form: hw = rows * ppt; backward small up to 8, cluster / two-kernel at 16; 12 and 32 are not small at all
        for ppt, (h, w) in zip((1, 2, 4, 8, 16, 12, 32), ((4, 8), (8, 8), (8, 16), (16, 16), (16, 32), (16, 24), (32, 32)) if dt == F32
                               else ((8, 8), (8, 16), (16, 16), (16, 32), (32, 32), (24, 32), (32, 64))):
            assert h * w == rows * ppt
            s.append((dt, 3, 64, h, w, 32, 'plain', True, None))
            s.append((dt, 2, 32, w, h, 16, 'add', False, None))       # (32 channels: the cluster form's 32-channel slices)
        s.append((dt, 2, 64, 8, 16, 32, 'acc', True, None))
        # channels per group 1 ... 32 and more, c from the smallest check_gn accepts to 256 vector slots
        for c in ((4, 8, 32, 64, 128, 256, 512, 1024) if dt == F32 else (8, 16, 32, 64, 128, 256, 512, 1024, 2048)):
            for groups in sorted({1, 32, c}):
                if c % groups == 0:
                    s.append((dt, 2, c, 8, 16, groups, 'plain', True, None))
                    s.append((dt, 2, c, 9, 13, groups, 'plain', groups != 1, None))
        # cluster form: non-square maps at the 1024-pixel default, 64- and 32-channel slices, with and without the addend
        for h, w in ((16, 64), (32, 32), (64, 16), (8, 128)):
            for c, groups in ((128, 32), (32, 16), (32, 32)):
                s.append((dt, 2, c, h, w, groups, 'plain', True, None))
            s.append((dt, 2, 128, h, w, 32, 'add', True, None))
        s.append((dt, 3, 128, 16, 64, 32, 'acc', True, None))
        # the pooled addend on non-square even maps above 1024 pixels (cluster forced / two-kernel / NT)
        for c, groups in ((128, 32), (32, 16)):
            s.append((dt, 2, c, 48, 80, groups, 'pooled', True, None))
        s.append((dt, 1, 64, 34, 66, 32, 'pooled', True, None))
        # two-kernel passes: ragged and tiny maps, maps below one row step of a block, n from 1 to 33
        for n, c, h, w, groups in ((33, 64, 1, 1, 8), (5, 64, 3, 5, 32), (4, 16, 3, 5, 8), (1, 128, 17, 25, 32),
                                   (2, 128, 17, 241, 32), (1, 128, 136, 200, 32), (7, 32, 5, 3, 16)):
            s.append((dt, n, c, h, w, groups, 'plain', True, None))
            s.append((dt, n, c, h, w, groups, 'add', True, None))
        s.append((dt, 2, 128, 17, 25, 32, 'acc', True, None))
        # last block short by less than / more than GN_DEPTH row steps (GN_BLOCKS_REDUCE / GN_BLOCKS_APPLY)
        for c in ((128, 512) if dt == F32 else (256, 1024)):         # 8 and 2 pixels per row step
            pstep = 256 // (c // (4 if dt == F32 else 8))
            for short in ((1, GN_DEPTH - 1), (GN_DEPTH + 2, 10 ** 6)):
                tot = _blocks_with_short_tail(2, 17 * 241, pstep, short)
                s.append((dt, 2, c, 17, 241, 32, 'plain', True, {'GN_BLOCKS_REDUCE': tot, 'GN_BLOCKS_APPLY': tot}))
    return s


def _blocks_with_short_tail(n, hw, pstep, short):
    """a block total whose last block per sample is short by `short[0]` ... `short[1]` row steps (and is not the only block)"""
    for tot in range(2 * n, 256 * n):
        ppb = _pick_ppb(n, hw, tot)
        nb = (hw + ppb - 1) // ppb
        steps = (ppb - (hw - (nb - 1) * ppb)) / pstep
        if nb > 1 and short[0] <= steps <= short[1]:
            return tot
    raise AssertionError(('no block total', hw, pstep, short))


def _cases():
    out = []
    for dt, n, c, h, w, groups, mode, silu, extra in _shapes():
        seen = set()
        for cfg in ('default', 'cluster', 'two', 'nt'):
            slots = dict(_CFG[cfg], **(extra or {}))
            if mode == 'pooled' and h * w <= 1024:
                continue
            f = _forms(dt, n, c, h, w, groups, slots, mode=mode)
            if f in seen:
                continue
            seen.add(f)
            tag = 'f32' if dt == F32 else 'bf16'
            tail = '' if not extra else '-blocks%d' % extra['GN_BLOCKS_REDUCE']
            out.append(pytest.param(dt, n, c, h, w, groups, mode, silu, slots,
                                    id=f'{tag}-{n}x{c}x{h}x{w}-g{groups}-{mode}-{"silu" if silu else "id"}-{f[0]}-{f[1]}{tail}'))
    return out


@pytest.mark.parametrize('dt,n,c,h,w,groups,mode,silu,slots', _cases())
def test_form_matches_fp64(dt, n, c, h, w, groups, mode, silu, slots):
    x, dy, wt, bs, add = _data(dt, n, c, h, w, mode, seed=n * 1000 + c + h * 7 + w)
    with _tuned(slots):
        got = _run(x, dy, wt, bs, add, groups, silu, mode)
    _check_all(dt, got, _ref(x, dy, wt, bs, add, groups, silu, mode))


# ------------------------------------------------------------------------------------------ dx column sums (conv bias gradient)
@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('n,c,h,w,groups', [(2, 128, 40, 48, 32), (1, 128, 136, 200, 32), (3, 64, 33, 35, 16)])
@pytest.mark.parametrize('mode', ['plain', 'add'])
@pytest.mark.parametrize('nt', [False, True])
def test_backward_colsum_matches_fp64(dt, n, c, h, w, groups, mode, nt):
    assert _forms(dt, n, c, h, w, groups, {}, colsum=True)[1] == 'two'
    x, dy, wt, bs, add = _data(dt, n, c, h, w, mode, seed=c + h)
    with _tuned({'GN_NT_MB': 0 if nt else 1 << 20}):
        got = _run(x, dy, wt, bs, add, groups, True, mode, colsum=True)
    _check_all(dt, got, _ref(x, dy, wt, bs, add, groups, True, mode))


def test_backward_colsum_refuses_deterministic_mode():
    x, dy, wt, bs, _ = _data(BF, 2, 64, 40, 40, 'plain', seed=5)
    _, st = ops.raw_gn_forward(x, wt, bs, 32, EPS, True)
    cs = torch.zeros(64, device=DEV)
    with _deterministic(True), pytest.raises(RuntimeError, match='gn_backward_colsum'):
        ops.raw_gn_backward(x, st, wt, bs, dy, 32, True, dx_colsum=cs)
    torch.cuda.synchronize()
    assert float(cs.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ deterministic mode
def _det_cases():
    s = []
    for dt, rows in ((F32, 32), (BF, 64)):
        for ppt in (1, 2, 4, 8, 16):
            s.append((dt, 3, 64, rows * ppt // 8, 8, 32, 'plain', 'default'))
        s += [(dt, 33, 64, 1, 1, 8, 'plain', 'default'), (dt, 2, 128, 17, 25, 32, 'add', 'default'),
              (dt, 2, 128, 16, 64, 32, 'plain', 'default'), (dt, 1, 128, 136, 200, 32, 'add', 'default'),
              (dt, 2, 32, 48, 80, 16, 'pooled', 'default'), (dt, 2, 128, 17, 25, 32, 'plain', 'nt'),
              (dt, 2, 64, 48, 80, 32, 'pooled', 'nt'), (dt, 3, 64, 16, 16, 32, 'plain', 'two')]
    # more groups than threads per block (csrc/norm.hip: gn_bwd_apply_kernel's per-group factors)
    s += [(F32, 2, 512, 12, 12, 512, 'plain', 'default'), (F32, 2, 1024, 9, 13, 1024, 'add', 'default'),
          (BF, 2, 2048, 6, 10, 1024, 'plain', 'default'), (BF, 2, 2048, 9, 13, 2048, 'plain', 'nt')]
    out = []
    for dt, n, c, h, w, groups, mode, cfg in s:
        f = _forms(dt, n, c, h, w, groups, _CFG[cfg], det=True, mode=mode)
        tag = 'f32' if dt == F32 else 'bf16'
        out.append(pytest.param(dt, n, c, h, w, groups, mode, cfg, id=f'{tag}-{n}x{c}x{h}x{w}-g{groups}-{mode}-{f[0]}-{f[1]}'))
    return out


@pytest.mark.parametrize('dt,n,c,h,w,groups,mode,cfg', _det_cases())
def test_deterministic_form_matches_fp64_and_repeats_bitwise(dt, n, c, h, w, groups, mode, cfg):
    x, dy, wt, bs, add = _data(dt, n, c, h, w, mode, seed=c * 3 + h * w)
    with _tuned(_CFG[cfg]), _deterministic(True):
        got = _run(x, dy, wt, bs, add, groups, True, mode)
        again = _run(x, dy, wt, bs, add, groups, True, mode)
    _same_bits(got, again)
    _check_all(dt, got, _ref(x, dy, wt, bs, add, groups, True, mode))


# ------------------------------------------------------------------------------------------ presummed forwards
def _group_sums(x, groups, nblk):
    """float64 (sum, sum of squares) of x as stored, per (sample, group, 256-pixel tile): [N, G, nblk, 2]"""
    n, c, h, w = x.shape
    xd = x.double().permute(0, 2, 3, 1).reshape(n, nblk, h * w // nblk, groups, c // groups)
    return torch.stack([xd.sum((2, 4)), (xd * xd).sum((2, 4))], -1).permute(0, 2, 1, 3).contiguous()


@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('n,c,h,w,groups', [(2, 128, 64, 64, 32), (1, 128, 128, 160, 32), (3, 64, 16, 16, 64)])
@pytest.mark.parametrize('parts', [False, True])
def test_presummed_forward_matches_fp64(dt, n, c, h, w, groups, parts):
    """vqk_gn_forward_presummed on float64 sums placed in the workspace (zero protocol), and vqk_gn_forward_presummed_parts on
    one slot per 256-pixel tile (deterministic mode: ordered, bit-identical on repeat)"""
    x, dy, wt, bs, _ = _data(dt, n, c, h, w, 'plain', seed=h + w + c)
    lib, hw = native.lib(), h * w
    nblk = hw // 256
    sums = _group_sums(x, groups, nblk)

    def run():
        y = torch.empty_like(x)
        st = torch.empty(n * groups * 2, device=DEV)
        if parts:
            slots = sums.reshape(-1).clone()
            scratch = torch.full((n * groups * 2,), float('nan'), dtype=torch.float64, device=DEV)
            native.check(lib.vqk_gn_forward_presummed_parts(ops.dcode(dt), x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(),
                                                            st.data_ptr(), slots.data_ptr(), nblk, scratch.data_ptr(), n, hw, c,
                                                            groups, EPS, 1, ops._stream()), 'gn_forward_presummed_parts')
        else:
            ws = ops._gn_ws(x.device, n * groups * 2 + n)
            _ws_zero('workspace dirty on entry')
            ws[:n * groups * 2].copy_(sums.sum(2).reshape(-1))
            native.check(lib.vqk_gn_forward_presummed(ops.dcode(dt), x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(),
                                                      st.data_ptr(), ws.data_ptr(), n, hw, c, groups, EPS, 1, ops._stream()),
                         'gn_forward_presummed')
            _ws_zero('workspace not zero after the presummed forward')
        torch.cuda.synchronize()
        return dict(y=y, stats=st)

    with _deterministic(parts):
        got = run()
        if parts:
            _same_bits(got, run())
    ref = _ref(x, dy, wt, bs, None, groups, True)
    err = _errors(dt, dict(got, dx=ref['dx'], dw=ref['dw'], db=ref['db']), ref)
    for k in ('y', 'mean', 'rstd') + (('y_rel',) if dt == BF else ()):
        _check(k, err[k], _BOUNDS[dt][k])


# ------------------------------------------------------------------------------------------ separate entry points
@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('n,c,h,w,groups', [(2, 64, 8, 8, 32), (33, 64, 1, 1, 8), (3, 128, 17, 25, 32), (1, 128, 136, 200, 32),
                                            (2, 512, 9, 13, 512), (2, 32, 40, 40, 1)])
@pytest.mark.parametrize('silu', [False, True])
def test_stats_and_apply_entry_points_match_fp64(dt, n, c, h, w, groups, silu):
    x, dy, wt, bs, _ = _data(dt, n, c, h, w, 'plain', seed=n + c + h + w)
    st = ops.raw_gn_stats(x, groups, EPS)
    y = ops.raw_gn_apply(x, st, wt, bs, groups, silu)
    torch.cuda.synchronize()
    ref = _ref(x, dy, wt, bs, None, groups, silu)
    err = _errors(dt, dict(y=y, stats=st, dx=ref['dx'], dw=ref['dw'], db=ref['db']), ref)
    for k in ('y', 'mean', 'rstd') + (('y_rel',) if dt == BF else ()):
        _check(k, err[k], _BOUNDS[dt][k])


# ------------------------------------------------------------------------------------------ chained calls on one stream
def test_chained_calls_leave_no_state_behind():
    """GroupNorm calls of different shapes, forms and dtypes back to back on one stream, no synchronisation in between; the last
    call still matches float64 (a workspace slot left non-zero by any of them would shift its statistics)"""
    seq = [(BF, 2, 128, 17, 25, 32, 'add', 'two'), (F32, 3, 64, 16, 64, 32, 'plain', 'cluster'),
           (BF, 2, 32, 48, 80, 16, 'pooled', 'nt'), (F32, 2, 64, 8, 16, 32, 'plain', 'default'),
           (BF, 2, 128, 32, 32, 32, 'plain', 'default'), (F32, 33, 64, 1, 1, 8, 'add', 'two'),
           (F32, 2, 128, 17, 25, 32, 'plain', 'two')]
    data = [_data(dt, n, c, h, w, mode, seed=i) for i, (dt, n, c, h, w, _g, mode, _cfg) in enumerate(seq)]
    ops._gn_ws(torch.device(DEV), 1 << 16)
    _ws_zero('workspace dirty on entry')
    for (dt, n, c, h, w, groups, mode, cfg), (x, dy, wt, bs, add) in zip(seq, data):
        with _tuned(_CFG[cfg]):
            y, st = ops.raw_gn_forward(x, wt, bs, groups, EPS, True)
            dw, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
            if mode == 'pooled':
                dx = ops.raw_gn_backward_pooled_add(x, st, wt, bs, dy, groups, True, dw, db, add, 0.25, cluster_ok=True)
            else:
                dx, _, _ = ops.raw_gn_backward(x, st, wt, bs, dy, groups, True, dw, db, add=add, cluster_ok=True)
    _ws_zero('workspace not zero after the chain')
    got = dict(y=y, stats=st, dx=dx, dw=dw.double(), db=db.double())
    _check_all(seq[-1][0], got, _ref(x, dy, wt, bs, add, seq[-1][5], True, seq[-1][6]))


# ------------------------------------------------------------------------------------------ large tensors
@pytest.mark.parametrize('dt,n', [(BF, 16), (F32, 8)])
def test_nt_form_at_full_size(dt, n):
    """the form of the headline bs-32 step: 128 channels at 256^2, >= 192 MiB (non-temporal loads), reference on the device"""
    c, h, w, groups = 128, 256, 256, 32
    assert _forms(dt, n, c, h, w, groups, {})[1] == 'nt'
    x, dy, wt, bs, add = _data(dt, n, c, h, w, 'add', seed=11)
    got = _run(x, dy, wt, bs, add, groups, True, 'add')
    ref = _ref(x, dy, wt, bs, add, groups, True, 'add')
    del x, dy, add
    _check_all(dt, got, ref)


@pytest.mark.parametrize('ratio', [8.0, 140.0])
def test_large_mean_fp32_longest_runs(ratio):
    """x = mu + sigma * N(0, 1) on the fp32 shape with the longest per-thread runs (32 x 128 @ 256^2: 16 reduce blocks per sample,
    512 pixels per thread summed in fp32 before the fp64 fold).  The statistics are raw moments: their error grows like
    (mu / sigma)^2 -- fp32 grade at mu / sigma = 8, the 2e-3 of test_gpu_ops.py::test_group_norm_large_mean_fp32 at 140"""
    n, c, h, w, groups = 32, 128, 256, 256, 32
    assert _pick_ppb(n, h * w, 512) // (256 // (c // 4)) == 512
    x, dy, wt, bs, _ = _data(F32, n, c, h, w, 'plain', seed=int(ratio), mu=ratio * 0.5, sigma=0.5)
    got = _run(x, dy, wt, bs, None, groups, False)
    ref = _ref(x, dy, wt, bs, None, groups, False)
    del x, dy
    _check_all(F32, got, ref, {k: 1e-5 if ratio < 100 else 2e-3 for k in ('y', 'dx', 'dw', 'db', 'mean', 'rstd')})
