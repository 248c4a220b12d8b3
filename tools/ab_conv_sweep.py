"""A/B sweep of the forward / data-gradient conv launchers under the library named by VQK_LIB (run through tools/ab_oldlib.py for a
library that lacks newer symbols).  Problems: the launchable rows of tests/conv_plan_rows.py plus every raw forward-conv call of one
eager train step of the flagship model (forward and data gradient), each replayed alone on seeded operands, in default and in
deterministic mode; writes {problem: sha256 of the output bytes} to the JSON named on the command line.
usage: [VQK_LIB=old.so python tools/ab_oldlib.py] tools/ab_conv_sweep.py OUT.json; then tools/ab_conv_compare.py"""
import hashlib
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
from tests import conv_plan_rows as T  # noqa: E402

DEV, CL = 'cuda:0', torch.channels_last
DT = {T.F32: torch.float32, T.BF16: torch.bfloat16}
NAME = {torch.float32: 'f32', torch.bfloat16: 'bf16'}
problems = {}                                                    # key -> spec (insertion order = launch order)


def note(kind, x, cout, ksize, ups, act, out_dtype, wlayout, bias, res, extra=()):
    n, cin, h, w = x.shape
    key = (kind, NAME[x.dtype], NAME[out_dtype], n, h, w, cin, cout, ksize, int(bool(ups)), act, wlayout, int(bias is not None),
           int(res is not None)) + tuple(extra)
    problems.setdefault('/'.join(map(str, key)), key)


def record_model_step():
    """one eager forward + backward of the flagship autoencoder at batch 2: every raw forward-conv call is noted, then runs as usual"""
    real = (ops.raw_conv_fprop, ops.raw_conv_fprop_pooled, ops.raw_conv_fprop_gnstats)

    def fprop(x, wq, bias, residual, ksize, ups, act, out_dtype, cout, wlayout=0, out=None):
        note('fprop', x, cout, ksize, ups, act, out_dtype, wlayout, bias, residual)
        return real[0](x, wq, bias, residual, ksize, ups, act, out_dtype, cout, wlayout, out)

    def pooled(x, wq, bias, residual, ksize, ups, cout, pool_scale):
        note('pooled', x, cout, ksize, ups, 0, x.dtype, 1, bias, residual)
        return real[1](x, wq, bias, residual, ksize, ups, cout, pool_scale)

    def gnstats(x, wq, bias, residual, ups, cout, groups, pool=False, pool_scale=0.25, wlayout=1):
        if wlayout == 1:
            note('gnstats', x, cout, 3, ups, 0, x.dtype, 1, bias, residual, (groups, int(pool)))
        return real[2](x, wq, bias, residual, ups, cout, groups, pool, pool_scale, wlayout)

    ops.raw_conv_fprop, ops.raw_conv_fprop_pooled, ops.raw_conv_fprop_gnstats = fprop, pooled, gnstats
    try:
        model_mod = importlib.import_module(PKG + '.model')
        torch.manual_seed(0)
        ae = dict(channels=128, num_res_blocks=2, channel_multipliers=(1, 2, 2, 4))
        qc = dict(num_embeddings=1024, embedding_dim=256, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
        tc = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
        for dtype in (torch.bfloat16, torch.float32):
            model = model_mod.VQVAE(256, ae, qc, None, tc, compute_dtype=dtype).to(DEV).train()
            loss = model.training_step(torch.rand(2, 3, 256, 256, device=DEV), 0)
            loss.backward()
            torch.cuda.synchronize()
            del model, loss
    finally:
        ops.raw_conv_fprop, ops.raw_conv_fprop_pooled, ops.raw_conv_fprop_gnstats = real


def table_rows():
    for r in T.ROWS:
        if r.form < 0 or r.flags & (T.GNSTATS | T.GENERAL) or r.variant != -1 or r.tuning:
            continue
        x = torch.empty(r.n, r.cin, r.h, r.w, dtype=DT[r.dtype], device='meta')
        res = x if r.flags & T.RESIDUAL else None
        note('pooled' if r.flags & T.POOL else 'fprop', x, r.cout, r.ksize, r.ups, r.act, DT[r.out_dtype], r.wlayout, None, res)


def replay(key):
    kind, dt, odt, n, h, w, cin, cout, ksize, ups, act, wlayout, has_bias, has_res = key[:14]
    dt = torch.float32 if dt == 'f32' else torch.bfloat16
    odt = torch.float32 if odt == 'f32' else torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(n + 3 * h + 5 * w + 7 * cin + 11 * cout + ksize + ups)
    s = 1 << ups
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).to(dt).contiguous(memory_format=CL)
    wmem = (torch.randn(cout, ksize, ksize, cin, device=DEV, generator=g) / (ksize * cin ** 0.5)).reshape(-1)
    bias = torch.randn(cout, device=DEV, generator=g) if has_bias else None
    wq = ops.pack_weights(wmem, dt, cout, cin, ksize, False, wlayout)
    if kind == 'fprop':
        res = torch.randn(n, cout, h * s, w * s, device=DEV, generator=g).to(odt).contiguous(memory_format=CL) if has_res else None
        y = ops.raw_conv_fprop(x, wq, bias, res, ksize, bool(ups), act, odt, cout, wlayout)
    elif kind == 'pooled':
        res = torch.randn(n, cout, h * s, w * s, device=DEV, generator=g).to(odt).contiguous(memory_format=CL) if has_res else None
        y = ops.raw_conv_fprop_pooled(x, wq, bias, res, ksize, bool(ups), cout, 0.25)
    else:
        groups, pool = key[14], key[15]
        res = torch.randn(n, cout, h * s, w * s, device=DEV, generator=g).to(odt).contiguous(memory_format=CL) if has_res else None
        y = ops.raw_conv_fprop_gnstats(x, wq, bias, res, bool(ups), cout, groups, bool(pool))
        if ops._HANDOFF.gn is not None:
            ops._claim_presummed(x, -1)                           # the sums nobody reads here
    torch.cuda.synchronize()
    if y is None:
        return 'not served'
    return hashlib.sha256(y.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def main():
    out = sys.argv[1]
    table_rows()
    record_model_step()
    result = {'lib': native.library_path(), 'problems': len(problems), 'default': {}, 'deterministic': {}}
    for mode in ('default', 'deterministic'):
        ops.set_deterministic(mode == 'deterministic')
        for name, key in problems.items():
            result[mode][name] = replay(key)
    ops.set_deterministic(False)
    os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
    json.dump(result, open(out, 'w'), indent=0)
    print(f'[ab_conv_sweep] {native.library_path()}: {len(problems)} problems x 2 modes -> {out}', flush=True)


if __name__ == '__main__':
    main()
