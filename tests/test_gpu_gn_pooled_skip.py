"""The GroupNorm apply pass that also stores the 2x2 average of its input (vqk_gn_forward_presummed_pooled, csrc/norm.hip:
gn_apply_fin_kernel<T, SILU, true>) against the pair of launches it replaces, vqk_gn_forward_presummed + vqk_pool2x2, on the same
inputs: y, stats and the pooled tensor are equal BIT FOR BIT (the pooled value is formed from the raw loaded x with pool2x2_kernel's
association, y by the same arithmetic per element), the workspace is left zero, an odd side is refused, and a pooling ResBlock
computes the same outputs and gradients with the form switched on and off.

Shapes: one quad; a width that is no power of two with a short last block; > 1024 pixels whose row pairs do not divide the
default block size (several blocks per sample); the 64 x 64 map the headline's smallest pooling block runs at.
"""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
native = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd._native')
DEV, F32, BF, CL = 'cuda:0', torch.float32, torch.bfloat16, torch.channels_last
EPS, GROUPS = 1e-6, 32
SHAPES = [(1, 64, 2, 2), (3, 128, 6, 10), (2, 256, 34, 36), (2, 128, 64, 64)]


def _data(dt, n, c, h, w, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(n, c, h, w, device=DEV, generator=g) * 1.5 + 0.25).to(dt).contiguous(memory_format=CL)
    wt = torch.randn(c, device=DEV, generator=g) * 0.5 + 1.0
    bs = torch.randn(c, device=DEV, generator=g) * 0.5
    return x, wt, bs


def _sums(x, groups):
    """float64 (sum, sum of squares) of x as stored, per (sample, group): [N, G, 2]"""
    n, c, h, w = x.shape
    xd = x.double().permute(0, 2, 3, 1).reshape(n, h * w, groups, c // groups)
    return torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], -1).contiguous()


def _ws(x, groups):
    n = x.shape[0]
    ws = ops._gn_ws(x.device, n * groups * 2 + n)
    torch.cuda.synchronize()
    assert int((ws != 0).sum()) == 0, 'workspace dirty on entry'
    return ws


def _ws_is_zero(what):
    ws = ops._gn_ws(torch.device(DEV), 0)
    torch.cuda.synchronize()
    nz = int((ws != 0).sum())
    assert nz == 0, (what, nz)


def _pair(x, wt, bs, sums, silu, scale):
    """the two launches: vqk_gn_forward_presummed, vqk_pool2x2"""
    n, c, h, w = x.shape
    lib, dc = native.lib(), ops.dcode(x.dtype)
    y, st = torch.empty_like(x), torch.empty(n * GROUPS * 2, device=DEV)
    pooled = ops.empty_nhwc(n, c, h // 2, w // 2, x.dtype, x.device)
    ws = _ws(x, GROUPS)
    ws[:n * GROUPS * 2].copy_(sums.reshape(-1))
    native.check(lib.vqk_gn_forward_presummed(dc, x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(), st.data_ptr(),
                                              ws.data_ptr(), n, h * w, c, GROUPS, EPS, int(silu), ops._stream()), 'gn_forward_presummed')
    native.check(lib.vqk_pool2x2(dc, x.data_ptr(), pooled.data_ptr(), n, h, w, c, scale, ops._stream()), 'pool2x2')
    torch.cuda.synchronize()
    return y, st, pooled


def _fused(x, wt, bs, sums, silu, scale):
    n, c, h, w = x.shape
    lib, dc = native.lib(), ops.dcode(x.dtype)
    y, st = torch.full_like(x, float('nan')), torch.empty(n * GROUPS * 2, device=DEV)
    pooled = torch.full_like(ops.empty_nhwc(n, c, h // 2, w // 2, x.dtype, x.device), float('nan'))
    ws = _ws(x, GROUPS)
    ws[:n * GROUPS * 2].copy_(sums.reshape(-1))
    native.check(lib.vqk_gn_forward_presummed_pooled(dc, x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(), st.data_ptr(),
                                                     ws.data_ptr(), n, h, w, c, GROUPS, EPS, int(silu), pooled.data_ptr(), scale,
                                                     ops._stream()), 'gn_forward_presummed_pooled')
    _ws_is_zero('workspace not zero after the pooled forward')
    return y, st, pooled


@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('n,c,h,w', SHAPES)
@pytest.mark.parametrize('silu', [True, False])
def test_pooled_forward_equals_the_two_launches(dt, n, c, h, w, silu):
    x, wt, bs = _data(dt, n, c, h, w, seed=1000 * h + w + c)
    sums = _sums(x, GROUPS)
    y0, st0, p0 = _pair(x, wt, bs, sums, silu, 0.25)
    y1, st1, p1 = _fused(x, wt, bs, sums, silu, 0.25)
    assert torch.equal(st1, st0)
    assert torch.equal(y1, y0)
    assert torch.equal(p1, p0)
    assert bool(torch.isfinite(p1.float()).all()) and bool(torch.isfinite(y1.float()).all())


@pytest.mark.parametrize('dt', [BF, F32])
def test_pooled_parts_entry_equals_the_two_launches(dt):
    """deterministic mode's entry (one slot per 256-pixel tile, added in a fixed order) on the several-blocks case"""
    n, c, h, w = 2, 128, 64, 64
    x, wt, bs = _data(dt, n, c, h, w, seed=7)
    lib, dc, nblk = native.lib(), ops.dcode(dt), h * w // 256
    xd = x.double().permute(0, 2, 3, 1).reshape(n, nblk, 256, GROUPS, c // GROUPS)
    slots = torch.stack([xd.sum((2, 4)), (xd * xd).sum((2, 4))], -1).permute(0, 2, 1, 3).contiguous().reshape(-1)

    def run(pool):
        y, st = torch.full_like(x, float('nan')), torch.empty(n * GROUPS * 2, device=DEV)
        pooled = torch.full_like(ops.empty_nhwc(n, c, h // 2, w // 2, dt, x.device), float('nan'))
        scratch = torch.full((n * GROUPS * 2,), float('nan'), dtype=torch.float64, device=DEV)
        if pool:
            native.check(lib.vqk_gn_forward_presummed_parts_pooled(dc, x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(),
                                                                   st.data_ptr(), slots.data_ptr(), nblk, scratch.data_ptr(), n, h, w,
                                                                   c, GROUPS, EPS, 1, pooled.data_ptr(), 0.25, ops._stream()),
                         'gn_forward_presummed_parts_pooled')
        else:
            native.check(lib.vqk_gn_forward_presummed_parts(dc, x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(),
                                                            st.data_ptr(), slots.data_ptr(), nblk, scratch.data_ptr(), n, h * w, c,
                                                            GROUPS, EPS, 1, ops._stream()), 'gn_forward_presummed_parts')
            native.check(lib.vqk_pool2x2(dc, x.data_ptr(), pooled.data_ptr(), n, h, w, c, 0.25, ops._stream()), 'pool2x2')
        torch.cuda.synchronize()
        return y, st, pooled

    ops.set_deterministic(True)
    try:
        ref, got = run(False), run(True)
    finally:
        ops.set_deterministic(False)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_odd_sides_are_refused():
    x, wt, bs = _data(BF, 1, 64, 6, 6, seed=3)
    lib, y, st = native.lib(), torch.empty(1, 64, 6, 6, device=DEV, dtype=BF), torch.empty(64, device=DEV)
    pooled = torch.empty(1, 64, 3, 3, device=DEV, dtype=BF)
    ws = _ws(x, GROUPS)
    for h, w in ((5, 6), (6, 5)):
        rc = lib.vqk_gn_forward_presummed_pooled(ops.dcode(BF), x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(), st.data_ptr(),
                                                 ws.data_ptr(), 1, h, w, 64, GROUPS, EPS, 1, pooled.data_ptr(), 0.25, ops._stream())
        assert rc == native.ERR_SHAPE, (h, w, rc)
        rc = lib.vqk_gn_forward_presummed_parts_pooled(ops.dcode(BF), x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(),
                                                       st.data_ptr(), ws.data_ptr(), 1, ws.data_ptr(), 1, h, w, 64, GROUPS, EPS, 1,
                                                       pooled.data_ptr(), 0.25, ops._stream())
        assert rc == native.ERR_SHAPE, (h, w, rc)


def test_raw_gn_forward_falls_back_to_the_pool_pass():
    """not presummed (nothing left the sums of x in the workspace): the ordinary forward, then raw_pool -- same three tensors"""
    x, wt, bs = _data(BF, 2, 128, 64, 64, seed=11)
    y0, st0 = ops.raw_gn_forward(x, wt, bs, GROUPS, EPS, True)
    y1, st1, p1 = ops.raw_gn_forward(x, wt, bs, GROUPS, EPS, True, pooled_scale=0.25)
    assert torch.equal(y1, y0) and torch.equal(st1, st0) and torch.equal(p1, ops.raw_pool(x, 0.25))
    _ws_is_zero('workspace not zero after raw_gn_forward')


def test_pooling_resblock_is_unchanged_bit_for_bit(monkeypatch):
    """two ResBlocks at (2, 128, 64, 64) in bf16, deterministic mode: the first leaves the GroupNorm sums of its output for the
    second, which pools (pooled-forward phase form, skip = its input).  With the form on the skip comes out of norm1's apply pass
    (no raw_pool call in the forward), with it off out of raw_pool: outputs and every gradient are equal bit for bit."""
    n, c, h, w = 2, 128, 64, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    x0 = rnd(n, c, h, w).to(BF).contiguous(memory_format=CL)
    dout = rnd(n, c, h // 2, w // 2).to(BF).contiguous(memory_format=CL)
    names = ('n1w', 'n1b', 'c1w', 'n2w', 'n2b', 'c2w')
    init = []
    for _ in range(2):
        init.append(dict(n1w=rnd(c) * 0.2 + 1.0, n1b=rnd(c) * 0.2, c1w=(rnd(c, c, 3, 3) * 0.03).contiguous(memory_format=CL),
                         n2w=rnd(c) * 0.2 + 1.0, n2b=rnd(c) * 0.2, c2w=(rnd(c, c, 3, 3) * 0.03).contiguous(memory_format=CL)))
    pools = []
    real_pool = ops.raw_pool
    monkeypatch.setattr(ops, 'raw_pool', lambda t, s: (pools.append(tuple(t.shape)), real_pool(t, s))[1])

    def run(on):
        monkeypatch.setattr(ops, 'GN_POOLED_SKIP', on)
        x = x0.clone().requires_grad_(True)
        params = [{k: v.clone().requires_grad_(True) for k, v in blk.items()} for blk in init]
        pools.clear()
        a = ops.res_block(x, *[params[0][k] for k in names], None, GROUPS, EPS, False, GROUPS)
        out = ops.res_block(a, *[params[1][k] for k in names], None, GROUPS, EPS, True, 0)
        torch.cuda.synchronize()
        fwd_pools = list(pools)
        grads = torch.autograd.grad(out, [x] + [blk[k] for blk in params for k in names], dout)
        torch.cuda.synchronize()
        return out.detach(), grads, fwd_pools

    ops.set_deterministic(True)
    try:
        out_off, grads_off, pools_off = run(False)
        out_on, grads_on, pools_on = run(True)
    finally:
        ops.set_deterministic(False)
    assert pools_off == [(n, c, h, w)] and pools_on == []          # the form was taken, and only where it should be
    assert torch.equal(out_on, out_off)
    for a, b in zip(grads_on, grads_off):
        assert torch.equal(a, b)
