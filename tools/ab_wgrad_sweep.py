"""A/B sweep of the one-layer and grouped weight-gradient launchers under the library named by VQK_LIB (run through
tools/ab_oldlib.py for a library that lacks newer symbols).
  rows      every launchable row of tests/wgrad_plan_rows.py through its own entry point, under the row's tuning slots, variant,
            block cap and deterministic workspace (operands, entry points and float64 reference of tests/test_gpu_wgrad_plan.py)
  problems  the default-state rows that the host routing reaches plus every raw weight-gradient call (plain, pooled-dy,
            split-product, edge) of one eager train step of the flagship model in bf16, fp32 and fp32 with split products at
            batch 2, each replayed alone on seeded operands through ops.py, plus one grouped launch of the step's small-map layers
Deterministic mode (and the rows that carry a deterministic workspace): one run, sha256 of dw.  Default mode: six runs -- three
to compare with, three more so that a library can be held against ITSELF under the same rule; when their bytes differ (fp32
atomics), or when the problem is named in the JSON given as second argument (a previous sweep's "split" list), also
max |dw - dw64| of each run against a float64 reference.  "split" lists what has several blocks adding to one dW element: >= 2
splits, the phases of a phase form, the row blocks of the fp32 thin forms (problems: asked of the plan query where the library has
it; rows: read off the table).
usage: [VQK_LIB=old.so python tools/ab_oldlib.py] tools/ab_wgrad_sweep.py OUT.json [SPLITS.json]; then tools/ab_wgrad_compare.py"""
import ctypes
import hashlib
import importlib
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
from tests import wgrad_plan_rows as T  # noqa: E402
from tests import test_gpu_wgrad_plan as G  # noqa: E402

DEV, CL = 'cuda:0', torch.channels_last
NAME = {torch.float32: 'f32', torch.bfloat16: 'bf16'}
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
HAS_PLAN = hasattr(ctypes.CDLL(native.library_path()), 'vqk_conv_wgrad_plan')
RUNS = 6
if not HAS_PLAN:                                                 # an older library: the edge rule as ops.py spelt it before the query
    ops.edge_wgrad_served = lambda x, dy, k, ups: (
        x.dtype == torch.bfloat16 and k == 3 and not ups and (x.shape[1], dy.shape[1]) in ((8, 128), (128, 8))
        and (x.shape[2] * x.shape[3]) % 128 == 0 and (x.shape[3] % 128 == 0 or 128 % x.shape[3] == 0))
problems = {}                                                    # key -> spec (insertion order = launch order)


def note(kind, x, dy, ksize, ups, x3, thin_true=8, has_db=False):
    n, cin, h, w = x.shape
    key = (kind, NAME[x.dtype], n, h, w, cin, dy.shape[1], ksize, int(ups), int(bool(x3)), int(thin_true), int(has_db))
    problems.setdefault('/'.join(map(str, key)), key)


def record_model_step():
    """one eager forward + backward of the flagship autoencoder at batch 2 per mode: every raw weight-gradient call is noted"""
    real = (ops.raw_conv_wgrad, ops.raw_conv_wgrad_pooled_dy, ops.raw_conv_wgrad_pooled_x3)

    def wgrad(x, dy, ksize, ups, out=None, thin_true=8, x3=False, db=None):
        note('wgrad', x, dy, ksize, ups, x3, thin_true, db is not None)
        return real[0](x, dy, ksize, ups, out=out, thin_true=thin_true, x3=x3, db=db)

    def pooled_dy(x, dyp, scale, out):
        note('pooled_dy', x, dyp, 3, 0, False)
        return real[1](x, dyp, scale, out)

    def pooled_x3(x, dyp, scale, out):
        note('pooled_x3', x, dyp, 3, 2, True)
        return real[2](x, dyp, scale, out)

    ops.raw_conv_wgrad, ops.raw_conv_wgrad_pooled_dy, ops.raw_conv_wgrad_pooled_x3 = wgrad, pooled_dy, pooled_x3
    try:
        model_mod = importlib.import_module(PKG + '.model')
        torch.manual_seed(0)
        ae = dict(channels=128, num_res_blocks=2, channel_multipliers=(1, 2, 2, 4))
        qc = dict(num_embeddings=1024, embedding_dim=256, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
        tc = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
        for dtype, products in ((torch.bfloat16, 'fp32'), (torch.float32, 'fp32'), (torch.float32, 'bf16x3')):
            ops.set_conv_products(products)
            model = model_mod.VQVAE(256, ae, qc, None, tc, compute_dtype=dtype).to(DEV).train()
            loss = model.training_step(torch.rand(2, 3, 256, 256, device=DEV), 0)
            loss.backward()
            torch.cuda.synchronize()
            del model, loss
    finally:
        ops.set_conv_products('fp32')
        ops.raw_conv_wgrad, ops.raw_conv_wgrad_pooled_dy, ops.raw_conv_wgrad_pooled_x3 = real


def table_rows():
    """rows of the default state that the host routing reaches with these arguments (the others: tests/test_gpu_wgrad_plan.py)"""
    for r in T.ROWS:
        if r.form < 0 or r.variant != -1 or r.tuning or r.det is not None or r.cap or r.stride != 1 or r.op == T.FOLD:
            continue
        dt = T.F32 if r.op == T.X3_OP else r.dtype
        x = torch.empty(r.n, r.cin, r.h << (r.op == T.POOLED_DY_PHASE), r.w << (r.op == T.POOLED_DY_PHASE), dtype=DT['f32' if dt == T.F32 else 'bf16'],
                        device='meta')
        if r.op in (T.POOLED_DY, T.POOLED_DY_PHASE) or (r.op == T.X3_OP and r.ups == 2):
            dy = torch.empty(r.n, r.cout, x.shape[2] // 2, x.shape[3] // 2, device='meta')
            note('pooled_x3' if r.op == T.X3_OP else 'pooled_dy', x, dy, 3, 2 if r.op == T.X3_OP else 0, r.op == T.X3_OP)
        else:
            ups = r.op == T.UPS_PHASE or r.ups == 1
            note('wgrad', x, torch.empty(r.n, r.cout, 1, 1, device='meta'), r.ksize, ups, r.op == T.X3_OP)


def operands(key):
    kind, dt, n, h, w, cin, cout, ksize, ups, x3, thin_true, has_db = key
    g = torch.Generator(device=DEV).manual_seed(n + 3 * h + 5 * w + 7 * cin + 11 * cout + ksize + ups)
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).to(DT[dt]).contiguous(memory_format=CL)
    hy, wy = (h // 2, w // 2) if kind != 'wgrad' else (h << ups, w << ups)
    dy = torch.randn(n, cout, hy, wy, device=DEV, generator=g).to(DT[dt]).contiguous(memory_format=CL)
    return x, dy


def launch(key, x, dy):
    """(dw, extra) of one run of the problem through the host routing, dw pre-zeroed"""
    kind, dt, n, h, w, cin, cout, ksize, ups, x3, thin_true, has_db = key
    co, ci = (thin_true if cout == 8 and thin_true != 8 else cout), (thin_true if cin == 8 and thin_true != 8 else cin)
    dw = torch.zeros((co, ksize, ksize, ci), dtype=torch.float32, device=DEV).permute(0, 3, 1, 2)
    db = torch.zeros(thin_true, device=DEV) if has_db else None
    if kind == 'wgrad':
        ops.raw_conv_wgrad(x, dy, ksize, bool(ups), out=dw, thin_true=thin_true, x3=bool(x3), db=db)
    elif kind == 'pooled_dy':
        if not ops.raw_conv_wgrad_pooled_dy(x, dy, 0.25, dw):
            return None, None
    elif not ops.raw_conv_wgrad_pooled_x3(x, dy, 0.25, dw):
        return None, None
    torch.cuda.synchronize()
    return dw, db


def reference(key, x, dy):
    """float64 dw of the problem (the thin side's padded channels dropped like the kernel drops them)"""
    kind, dt, n, h, w, cin, cout, ksize, ups, x3, thin_true, has_db = key
    xin = x.double()
    if kind == 'wgrad' and ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode='nearest')
    dyf = dy.double() if kind == 'wgrad' else 0.25 * F.interpolate(dy.double(), scale_factor=2.0, mode='nearest')
    wd = torch.zeros(cout, cin, ksize, ksize, device=DEV, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xin, wd, None, padding=ksize >> 1) * dyf).sum().backward()
    ref = wd.grad
    if thin_true != 8:
        ref = ref[:thin_true] if cout == 8 else ref[:, :thin_true]
    return ref


def sha(*ts):
    m = hashlib.sha256()
    for t in ts:
        if t is not None:
            m.update(t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    return m.hexdigest()


def plan_splits(key):
    """blocks that add to one dW element in the plan of the entry point that served the problem: its splits, at least 2 for the
    four phases of a phase form and the row blocks of the fp32 thin forms; None where the library cannot be asked"""
    if not HAS_PLAN:
        return None
    took, real = [], ops._run_wgrad

    def spy(what, call, *event, **kw):
        ok = real(what, call, *event, **kw)
        if ok:
            took.append(event)
        return ok

    ops._run_wgrad = spy
    try:
        launch(key, *operands(key))
    finally:
        ops._run_wgrad = real
    if not took:
        return None                                              # the edge kernels: ordered workspace sums, no plan
    op, xx, cout, h, w, ksize, ups = took[-1][:7]
    details = (ctypes.c_int * 5)()
    form = native.lib().vqk_conv_wgrad_plan(op, ops.dcode(xx.dtype), xx.shape[0], h, w, xx.shape[1], cout, ksize, 1, ksize >> 1, ups,
                                            h << (ups == 1), w << (ups == 1), details)
    if form < 0:
        return None
    return max(details[1], 2) if form in (2, 3, 14, 15) or details[4] else details[1]      # (phases / thin row blocks add like splits)


def group_problem():
    """the step's small-map layers as ONE grouped call: per item sha and float64 error, `own` items (one split) are plain adds"""
    items, keys = [], []
    for name, key in problems.items():
        kind, dt, n, h, w, cin, cout, ksize, ups, x3, thin_true, has_db = key
        if kind == 'wgrad' and dt == 'bf16' and ksize == 3 and not ups and h * w <= ops.WGRAD_GROUP_MAX_HW and h % 8 == 0 and w % 16 == 0 \
                and cin % 64 == 0 and cout % 64 == 0:
            x, dy = operands(key)
            items.append((x, dy, torch.zeros((cout, 3, 3, cin), dtype=torch.float32, device=DEV).permute(0, 3, 1, 2)))
            keys.append((name, key))
    return items, keys


def run_row(r):
    """the row's entry point under the row's state: sha256 of dw and max |dw - dw64| per run"""
    lib = native.lib()
    x, dy, _ = G._operands(r)
    ref = G._reference(r, x, dy)
    ops._stream()
    ws = torch.empty(max(r.det or 0, 16) // 4, device=DEV) if r.det is not None else None
    for slot, val in r.tuning.items():
        native.check(lib.vqk_set_tuning(slot.encode(), val), 'set_tuning')
    lib.vqk_conv_set_variant(r.variant)
    lib.vqk_conv_set_block_caps(0, r.cap)
    if ws is not None:
        native.check(lib.vqk_set_deterministic(1, ws.data_ptr(), r.det), 'set_deterministic')
    shas, errs = [], []
    try:
        for _ in range(1 if ws is not None else RUNS):
            dw = torch.zeros(r.cout, r.ksize, r.ksize, r.cin, device=DEV)
            if r.stride == 1:
                what, call = G._entry(lib, r, x, dy, dw)
                st = call()
            else:
                st = lib.vqk_conv2d_wgrad_general(r.dtype, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), r.n, r.h, r.w, r.cin, r.cout, r.ksize,
                                                  r.stride, r.pad, r.ups, r.h_out, r.w_out, ops.zero_page(x.device).data_ptr(), ops._stream())
            torch.cuda.synchronize()
            native.check(st, r.name)
            shas.append(sha(dw))
            errs.append(float((dw.permute(0, 3, 1, 2).double() - ref).abs().max()))
    finally:
        lib.vqk_conv_set_block_caps(0, 0)
        lib.vqk_conv_set_variant(-1)
        if r.tuning:
            lib.vqk_reset_tuning()
            native.apply_env_tuning(lib)
        ops.rearm_workspaces()
    atomic = ws is None and (r.splits >= 2 or r.launches == 4 or r.form in (T.MX_UPS_PHASE, T.MX_POOLED_DY_PHASE, T.X3_UPS_PHASE,
                                                                             T.X3_POOLED_PHASE, T.THIN_CIN4, T.THIN_COUT4))
    return dict(sha=shas, errors=errs, atomic=atomic)


def main():
    out = sys.argv[1]
    force = set(json.load(open(sys.argv[2]))['split']) if len(sys.argv) > 2 else set()
    table_rows()
    record_model_step()
    result = {'lib': native.library_path(), 'problems': len(problems), 'default': {}, 'deterministic': {}, 'split': [], 'errors': {}}
    for name, key in problems.items():
        s = plan_splits(key)
        if s is not None and s >= 2:
            result['split'].append(name)
    for mode in ('default', 'deterministic'):
        ops.set_deterministic(mode == 'deterministic')
        for name, key in problems.items():
            x, dy = operands(key)
            runs = [launch(key, x, dy) for _ in range(RUNS if mode == 'default' else 1)]
            if runs[0][0] is None:
                result[mode][name] = ['not served']
                continue
            result[mode][name] = [sha(*r) for r in runs]
            if mode == 'default' and (len(set(result[mode][name])) > 1 or name in force or name in result['split']):
                ref = reference(key, x, dy)
                result['errors'][name] = [float((r[0].double() - ref).abs().max()) for r in runs]
        if mode == 'default':                                    # the grouped launch (refused in deterministic mode)
            items, keys = group_problem()
            for run in range(RUNS if items else 0):
                for x, dy, dw in items:
                    dw.zero_()
                st, splits, launches = ops.raw_conv_wgrad_group(items)
                torch.cuda.synchronize()
                assert st == 0, st
                for (name, key), (x, dy, dw), s in zip(keys, items, splits):
                    gname = 'group:' + name
                    result[mode].setdefault(gname, []).append(sha(dw))
                    if s >= 2:
                        if run == 0:
                            result['split'].append(gname)
                        result['errors'].setdefault(gname, []).append(float((dw.double() - reference(key, x, dy)).abs().max()))
                result['group'] = dict(items=len(items), launches=launches, splits=list(splits))
    ops.set_deterministic(False)
    result['rows'] = {r.name: run_row(r) for r in T.ROWS if r.form >= 0}
    os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
    json.dump(result, open(out, 'w'), indent=0)
    print(f'[ab_wgrad_sweep] {native.library_path()}: {len(problems)} problems x 2 modes, {len(result["split"])} split, '
          f'{len(result["errors"])} with float64 errors, {len(result["rows"])} table rows -> {out}', flush=True)


if __name__ == '__main__':
    main()
