"""The weight-gradient launch plan (vqk_conv_wgrad_plan: csrc/conv_wgrad.hip::plan_wgrad behind the C-ABI) on the CPU: it names
the kernel form, the grid and the split for every row of tests/wgrad_plan_rows.py -- a table derived by reading the launcher's
cascade, not by running the plan -- and it never refuses the entry point that the routing of ops.py tries first."""
import ctypes
import importlib
import itertools

import pytest
import torch

from tests import wgrad_plan_rows as T

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
native = importlib.import_module(PKG + '._native')
FAKE_WS = 0x40000                                                 # aligned, never dereferenced: a plan launches nothing
DT = {T.F32: torch.float32, T.BF16: torch.bfloat16}


@pytest.fixture(scope='module')
def lib():
    native.build()
    return native.lib()


def plan(lib, r):
    """(form or status, details) of a table row under its variant, tuning, block cap and deterministic state, all put back after"""
    details = (ctypes.c_int * 5)()
    for slot, val in r.tuning.items():
        assert lib.vqk_set_tuning(slot.encode(), val) == 0
    assert lib.vqk_conv_set_variant(r.variant) == 0
    assert lib.vqk_conv_set_block_caps(0, r.cap) == 0
    if r.det is not None:
        assert lib.vqk_set_deterministic(1, FAKE_WS, r.det) == 0
    try:
        form = lib.vqk_conv_wgrad_plan(r.op, r.dtype, r.n, r.h, r.w, r.cin, r.cout, r.ksize, r.stride, r.pad, r.ups, r.h_out, r.w_out,
                                       details)
    finally:
        lib.vqk_set_deterministic(0, None, 0)
        lib.vqk_conv_set_block_caps(0, 0)
        lib.vqk_conv_set_variant(-1)
        if r.tuning:
            lib.vqk_reset_tuning()
            native.apply_env_tuning(lib)
    return form, list(details)


def test_table_covers_what_the_dispatch_can_do():
    rows = T.ROWS
    assert len({r.name for r in rows}) == len(rows)
    assert {r.form for r in rows} >= set(range(16)) | {T.ERR_SHAPE, T.ERR_ARG, T.ERR_DTYPE}
    for form in set(range(16)) - {T.THIN_CIN4, T.THIN_COUT4}:                          # every form that can split: once each way
        assert {r.splits >= 2 for r in rows if r.form == form} == {False, True}, form
    det = [r for r in rows if r.det is not None]
    assert any(r.form == T.MX and r.ordered for r in det) and any(r.form == T.MX and r.splits == 1 and not r.ordered for r in det)
    assert any(r.form in (T.GENERAL_F32, T.GENERAL_BF16, T.GENERAL_DB) and r.ordered for r in det)
    assert {r.op for r in det if r.form == T.ERR_SHAPE} == {T.UPS_PHASE, T.POOLED_DY_PHASE, T.FOLD, T.X3_OP}
    assert any(r.variant == 0 for r in rows)
    slots = [r.tuning for r in rows]
    assert all(any(t.get(s, d) != d for t in slots)
               for s, d in (('WGMX', 1), ('WGRAD_BLOCKS', 0), ('WGRAD_NO_PW16', 0), ('WGRAD_NO_P16K', 0), ('UPS_MERGE', 1), ('X3_WGRAD_PHASE', 1)))
    small = [r for r in rows if not r.name.startswith('thin-cin4-w4')]                  # (the fp32 thin form's LDS bound needs w >= 408)
    assert len(small) == len(rows) - 2
    assert all(r.n <= 2 and r.cin <= 256 and r.cout <= 256 and max(r.h, r.h_out) <= 64 and max(r.w, r.w_out) <= 64 for r in small)


@pytest.mark.parametrize('r', T.ROWS, ids=[r.name for r in T.ROWS])
def test_plan_row(lib, r):
    form, (tiles, splits, pps, launches, membound) = plan(lib, r)
    assert form == r.form, (form, lib.vqk_conv_wgrad_form_name(form, r.dtype))
    if form < 0:
        return
    assert (tiles, splits, pps, launches) == (r.tiles, r.splits, r.pps, r.launches)
    assert (launches == 2) == bool(r.ordered) and (launches == 4) == (r.tuning.get('UPS_MERGE') == 0)
    name = lib.vqk_conv_wgrad_form_name(form, r.dtype if r.dtype in DT else T.BF16).decode()
    assert name == T.NAMES[form] and name.endswith(' (HBM)') == bool(membound) == (form in (T.THIN_CIN4, T.THIN_COUT4))


def test_plan_argument_checks(lib):
    d = (ctypes.c_int * 5)()
    ok = (T.PLAIN, T.BF16, 2, 16, 32, 64, 64, 3, 1, 1, 0, 16, 32)
    assert lib.vqk_conv_wgrad_plan(*ok, d) == T.MX and lib.vqk_conv_wgrad_plan(*ok, None) == T.MX       # details are optional
    assert lib.vqk_conv_wgrad_plan(6, *ok[1:], d) == T.ERR_ARG and lib.vqk_conv_wgrad_plan(-1, *ok[1:], d) == T.ERR_ARG
    bad = {2: (0, -1), 3: (0, -1), 5: (0, -1), 6: (-8, -1), 8: (0, -5), 9: (-1, -5)}                  # arg index: (value, status)
    for i, (val, status) in bad.items():
        args = list(ok)
        args[i] = val
        assert lib.vqk_conv_wgrad_plan(*args, d) == status, i
    # ops 1-5 take the map from (h_in, w_in) alone; 4 and 5 bring their own dtype
    assert lib.vqk_conv_wgrad_plan(T.POOLED_DY, T.BF16, 2, 16, 32, 64, 64, 1, 2, 7, 1, 3, 3, d) == T.MX_POOLED_DY
    assert lib.vqk_conv_wgrad_plan(T.X3_OP, T.BF16, 2, 16, 32, 64, 64, 3, 1, 1, 0, 0, 0, d) == T.X3
    assert lib.vqk_conv_wgrad_form_name(99, 0) == b'?' and lib.vqk_conv_wgrad_form_name(-1, 1) == b'?'
    assert lib.vqk_conv_wgrad_form_name(0, 7) == b'?'


def test_edge_served_rule(lib):
    """vqk_conv2d_wgrad_edge_serves: bf16, (8, 128) or (128, 8) channels, 128-pixel patches inside a row or over whole rows"""
    serves = lib.vqk_conv2d_wgrad_edge_serves
    assert serves(T.BF16, 2, 16, 16, 8, 128) == 1 and serves(T.BF16, 2, 4, 256, 128, 8) == 1
    assert serves(T.F32, 2, 16, 16, 8, 128) == 0 and serves(T.BF16, 2, 16, 16, 8, 64) == 0 and serves(T.BF16, 2, 16, 16, 128, 128) == 0
    assert serves(T.BF16, 2, 8, 8, 8, 128) == 0 and serves(T.BF16, 2, 2, 192, 8, 128) == 0 and serves(T.BF16, 0, 16, 16, 8, 128) == 0
    ops = importlib.import_module(PKG + '.ops')
    x = torch.empty(2, 8, 16, 16, dtype=torch.bfloat16, device='meta')
    dy = torch.empty(2, 128, 16, 16, dtype=torch.bfloat16, device='meta')
    assert ops.edge_wgrad_served(x, dy, 3, False) and not ops.edge_wgrad_served(x, dy, 3, True) and not ops.edge_wgrad_served(x, dy, 1, False)
    assert not ops.edge_wgrad_served(x.float(), dy.float(), 3, False)


def test_label_matches_the_plan(lib):
    """ops._wgrad_event: label, FLOPs, executed FLOPs, launches and bytes from the library's plan; a memory-bound form has bytes and
    no FLOPs, a phase form executes 4/9, a split-product form x 3; None for a problem the plan refuses"""
    ops = importlib.import_module(PKG + '.ops')
    xb = torch.empty(2, 64, 16, 32, dtype=torch.bfloat16, device='meta')
    xf = torch.empty(2, 64, 16, 32, device='meta')
    mx, x3 = 'conv3x3_wgrad_mx_kernel<bf16>', 'conv3x3_wgrad_x3_kernel<f32 as 3 x bf16>'
    def ev(*a):                                                  # (FLOP figures to float rounding)
        r = ops._wgrad_event(*a)
        assert r is None or (r[4] > 0) == r[0].endswith(' (HBM)')      # bytes for the memory-bound forms only
        return r if r is None else (r[0], pytest.approx(r[1]), pytest.approx(r[2]), r[3])
    assert ev(T.PLAIN, xb, 64, 16, 32, 3, 0, 9.0) == (mx, 9.0, 9.0, 1)
    assert ev(T.PLAIN, xb, 64, 16, 32, 1, 0, 9.0) == ('conv_wgrad_db_kernel<bf16>', 9.0, 9.0, 1)
    assert ev(T.PLAIN, xb[:, :, :, :24], 64, 16, 24, 3, 0, 9.0) == ('conv3x3_wgrad_halo_kernel<bf16>', 9.0, 9.0, 1)
    assert ev(T.PLAIN, xb[:, :, :12], 64, 12, 32, 3, 0, 9.0) == ('conv_wgrad_kernel<bf16>', 9.0, 9.0, 1)
    assert ev(T.PLAIN, xf, 64, 16, 32, 3, 0, 9.0) == ('conv_wgrad_kernel<f32>', 9.0, 9.0, 1)
    assert ev(T.PLAIN, xf[:, :4], 64, 16, 32, 3, 0, 9.0) == ('conv3x3_wgrad_thin_f32_kernel (HBM)', 0.0, 0.0, 1)
    assert ops._wgrad_event(T.PLAIN, xf[:, :4], 64, 16, 32, 3, 0, 9.0)[4] == 4 * 2 * 16 * 32 * (4 + 64)        # x and dy, fp32
    assert ev(T.POOLED_DY, xb, 64, 16, 32, 3, 0, 9.0) == (mx, 9.0, 9.0, 1)
    assert ev(T.UPS_PHASE, xb, 64, 16, 32, 3, 0, 9.0) == (mx, 9.0, 4.0, 1)
    assert ev(T.POOLED_DY_PHASE, xb, 128, 16, 32, 3, 0, 9.0) == (mx, 9.0, 4.0, 1)
    assert ev(T.FOLD, xf, 64, 16, 32, 3, 0, 9.0) == ('conv3x3_wgrad_mx_kernel<f32 as 3 x bf16>', 9.0, 27.0, 1)
    assert ev(T.X3_OP, xf, 64, 16, 32, 3, 0, 9.0) == (x3, 9.0, 27.0, 1)
    assert ev(T.X3_OP, xf, 64, 16, 32, 3, 1, 9.0) == (x3, 9.0, 12.0, 1) and ev(T.X3_OP, xf, 64, 16, 32, 3, 2, 9.0) == (x3, 9.0, 12.0, 1)
    assert ev(T.POOLED_DY, xf, 64, 16, 32, 3, 0, 9.0) is None and ev(T.UPS_PHASE, xb[:, :, :, :24], 64, 16, 24, 3, 0, 9.0) is None
    lib.vqk_set_tuning(b'WGMX', 0)                               # the label follows the library's slot, not the host's environment
    lib.vqk_set_tuning(b'UPS_MERGE', 0)
    try:
        assert ev(T.PLAIN, xb, 64, 16, 32, 3, 0, 9.0) == ('conv3x3_wgrad_p16_kernel<bf16>', 9.0, 9.0, 1)
        lib.vqk_set_tuning(b'WGMX', 1)
        assert ev(T.UPS_PHASE, xb, 64, 16, 32, 3, 0, 9.0) == (mx, 9.0, 4.0, 4)
    finally:
        lib.vqk_reset_tuning()
        native.apply_env_tuning(lib)
    # the event is asked only while events are recorded, and a refused call records none
    assert ops.KERNEL_EVENTS is None
    asked = []
    real, ops._wgrad_event = ops._wgrad_event, lambda *a: asked.append(a)
    try:
        assert ops._run_wgrad('probe', lambda: 0, T.PLAIN, xb, 64, 16, 32, 3, 0, 9.0, '') is True and not asked
        assert ops._run_wgrad('probe', lambda: native.ERR_SHAPE, T.PLAIN, xb, 64, 16, 32, 3, 0, 9.0, '') is False and not asked
        with pytest.raises(RuntimeError):
            ops._run_wgrad('probe', lambda: -5, T.PLAIN, xb, 64, 16, 32, 3, 0, 9.0, '')
        with pytest.raises(RuntimeError):                        # the last resort of the routing may not refuse
            ops._run_wgrad('probe', lambda: native.ERR_SHAPE, T.PLAIN, xb, 64, 16, 32, 3, 0, 9.0, '', must=True)
        ops.KERNEL_EVENTS = []
        assert ops._run_wgrad('probe', lambda: native.ERR_SHAPE, T.POOLED_DY, xf, 64, 16, 32, 3, 0, 9.0, '') is False
        assert len(asked) == 1 and ops.KERNEL_EVENTS == []
    finally:
        ops._wgrad_event, ops.KERNEL_EVENTS = real, None


# ---------------------------------------------------------------------------------------------------------------------------------
# the sweep: the entry point the routing of ops.py tries FIRST for a problem is one the plan serves.  Problems where the launcher
# before the plan function already refused the routing's first choice would be listed here as (function, dtype, ksize, ups, x3,
# cin, cout, h, w, deterministic); none was found.
KNOWN_REFUSALS = set()


def test_routing_is_never_refused(lib, monkeypatch):
    ops = importlib.import_module(PKG + '.ops')
    chans = (4, 8, 32, 64, 96, 128, 256)
    maps = ((4, 4), (8, 32), (16, 16), (16, 48), (24, 24), (12, 32), (32, 32), (64, 64), (8, 200), (136, 16))
    tried = []

    def first_try(what, launch, op, x, cout, h, w, ksize, ups, flops, tag, must=False):
        tried.append((op, lib.vqk_conv_wgrad_plan(op, ops.dcode(x.dtype), x.shape[0], h, w, x.shape[1], cout, ksize, 1, ksize >> 1, ups,
                                                  h << (ups == 1), w << (ups == 1), None)))
        return True                                              # (nothing is launched; the routing stops at its first choice)

    monkeypatch.setattr(ops, '_run_wgrad', first_try)
    monkeypatch.setattr(ops, 'raw_split_pair', lambda t: t)
    monkeypatch.setattr(ops, 'POOLED_WGRAD_PHASE', True)         # (off by default: with it the pooled-dy routing has two first choices)
    seen, refused = set(), []
    for det in (False, True):
        monkeypatch.setattr(ops, 'DETERMINISTIC', det)
        assert lib.vqk_set_deterministic(int(det), FAKE_WS if det else None, T.WS if det else 0) == 0
        try:
            for dt, k, ups, x3, cin, cout, (h, w) in itertools.product((T.F32, T.BF16), (1, 3), (0, 1), (False, True), chans, chans, maps):
                if cin % (4 if dt == T.F32 else 8) or cout % (4 if dt == T.F32 else 8):
                    continue
                x = torch.empty(2, cin, h, w, dtype=DT[dt], device='meta')
                dy = torch.empty(2, cout, h << ups, w << ups, dtype=DT[dt], device='meta')
                dw = torch.empty(cout, cin, k, k, device='meta')
                calls = []
                if not ops.edge_wgrad_served(x, dy, k, bool(ups)):     # (the edge kernels have their own entry points and checks)
                    calls.append(('wgrad', lambda: ops.raw_conv_wgrad(x, dy, k, bool(ups), out=dw, x3=x3)))
                if k == 3 and not ups and h % 2 == 0 and w % 2 == 0:
                    dyp = torch.empty(2, cout, h // 2, w // 2, dtype=DT[dt], device='meta')
                    calls.append(('pooled_dy', lambda: ops.raw_conv_wgrad_pooled_dy(x, dyp, 0.25, dw)))
                    if x3:
                        calls.append(('pooled_x3', lambda: ops.raw_conv_wgrad_pooled_x3(x, dyp, 0.25, dw)))
                for fn, call in calls:
                    del tried[:]
                    call()
                    for op, form in tried[:1]:
                        seen.add(op)
                        if form < 0 and (fn, dt, k, ups, x3, cin, cout, h, w, det) not in KNOWN_REFUSALS:
                            refused.append((fn, dt, k, ups, x3, cin, cout, h, w, det, op, form))
                if ops.wgrad_group_deferrable(x, dy, dw, x3, k, bool(ups)):
                    seen.add('group')
                    item = native.WgradItem(FAKE_WS, FAKE_WS, FAKE_WS, dt, 2, h, w, cin, cout, 3, 0, 1.0, 0)
                    splits, launches = ctypes.c_int(0), ctypes.c_int(0)
                    st = lib.vqk_conv3x3_wgrad_group_plan(ctypes.addressof(item), 1, ctypes.addressof(splits), ctypes.addressof(launches))
                    if st != 0:
                        refused.append(('group', dt, k, ups, x3, cin, cout, h, w, det, st))
        finally:
            lib.vqk_set_deterministic(0, None, 0)
    assert seen == {T.PLAIN, T.POOLED_DY, T.UPS_PHASE, T.POOLED_DY_PHASE, T.X3_OP, 'group'}     # (FOLD: the VQK_X3_WGRAD_FOLD switch)
    assert not refused, refused[:20]
