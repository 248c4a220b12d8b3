"""The forward-conv launch plan (vqk_conv_fprop_plan: csrc/conv.hip::plan_fprop behind the C-ABI) on the CPU: it names the kernel
form for every row of tests/conv_plan_rows.py -- a table derived by reading the launcher's cascade, not by running the plan --
and it never refuses the operand layout that ops.weight_layout tells the packer to build.

One anchor row of the issue that introduced the plan ("128 -> 128 @128x128, layout 1, variant 4 -> stream, full tiles") does not
hold for the launcher it was derived from: variant 4 only removes the stream kernel's half-tile form, the matrix/auxiliary-wave
kernel is tested first and serves that problem (whole 128-cout tile, cin >= 64).  The table keeps the problem and the variant
twice: at the default tuning, where the form is the matrix/auxiliary-wave kernel, and with the MX slot off, where the row's
expectation holds."""
import ctypes
import importlib
import itertools

import pytest
import torch

from tests import conv_plan_rows as T

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
native = importlib.import_module(PKG + '._native')
FAKE_SCRATCH = 0x40000                                            # aligned, never dereferenced: a plan launches nothing


@pytest.fixture(scope='module')
def lib():
    native.build()
    return native.lib()


def plan(lib, r):
    """(form or status, details) of a table row under its variant, tuning and scratch; the thread's state is put back"""
    details = (ctypes.c_int * 5)()
    for slot, val in r.tuning.items():
        assert lib.vqk_set_tuning(slot.encode(), val) == 0
    assert lib.vqk_conv_set_variant(r.variant) == 0
    if r.scratch:
        assert lib.vqk_set_scratch(FAKE_SCRATCH, r.scratch) == 0
    try:
        form = lib.vqk_conv_fprop_plan(r.dtype, r.out_dtype, r.n, r.h, r.w, r.cin, r.cout, r.ksize, r.ups, r.act, r.wlayout,
                                       r.flags, details)
    finally:
        lib.vqk_set_scratch(0, 0)
        lib.vqk_conv_set_variant(-1)
        if r.tuning:
            lib.vqk_reset_tuning()
            native.apply_env_tuning(lib)
    return form, list(details)


def test_table_covers_every_form_and_refusal():
    forms = {r.form for r in T.ROWS}
    assert set(range(14)) <= forms and {T.ERR_SHAPE, T.ERR_ARG} <= forms
    assert len({r.name for r in T.ROWS}) == len(T.ROWS)
    assert all(r.n <= 2 and r.cin <= 256 and r.cout <= 256 and (r.h << r.ups) <= 256 and (r.w << r.ups) <= 256 for r in T.ROWS)


@pytest.mark.parametrize('r', T.ROWS, ids=[r.name for r in T.ROWS])
def test_plan_row(lib, r):
    form, (tw, blocks, splits, launches, membound) = plan(lib, r)
    assert form == r.form, (form, lib.vqk_conv_fprop_form_name(form, r.dtype))
    if form < 0:
        return
    assert (tw, splits, launches) == (r.tw, r.splits, r.launches)
    name = lib.vqk_conv_fprop_form_name(form, r.dtype).decode()
    assert name != '?' and name.endswith(' (HBM)') == bool(membound)
    assert bool(membound) == (form in (T.THIN_OUT_F32, T.THIN_IN_F32, T.MX_1X1, T.THIN_IN_BF16, T.X3_1X1))
    # the grid, where conv.hip itself sizes it (same reading of the cascade: persistent stream grid of at most STREAM_BLOCKS = 512)
    tiles = r.n * ((r.h << r.ups) // (256 >> tw)) * ((r.w << r.ups) >> tw) * -(-r.cout // 128) if tw else 0
    m = r.n * (r.h << r.ups) * (r.w << r.ups)
    want = {T.STREAM_THIN: min(tiles, 512), T.STREAM_FULL: min(tiles, 512), T.STREAM_HALF: min(2 * tiles, 512),
            T.HALO_BREG: tiles, T.HALO_LDS: tiles, T.IM2COL: -(-m // 128) * -(-r.cout // 128),
            T.IM2COL_SPLITK: -(-m // 128) * -(-r.cout // 128),
            T.THIN_IN_BF16: min(-(-(r.n * r.h * (r.w >> 5)) // 4), 1024)}.get(form, 0)
    assert blocks == want


def test_plan_argument_checks(lib):
    d = (ctypes.c_int * 5)()
    ok = (T.BF16, T.BF16, 1, 32, 32, 128, 128, 3, 0, 0, 1, 0)
    assert lib.vqk_conv_fprop_plan(*ok, d) == T.MX and lib.vqk_conv_fprop_plan(*ok, None) == T.MX     # details are optional
    bad = {0: (7, -2), 1: (7, -2), 8: (2, -5), 9: (4, -5), 10: (3, -5), 11: (16, -5), 5: (12, -1)}    # arg index: (value, status)
    for i, (val, status) in bad.items():
        args = list(ok)
        args[i] = val
        assert lib.vqk_conv_fprop_plan(*args, d) == status, i
    assert lib.vqk_conv_fprop_plan(T.F32, T.BF16, 1, 32, 32, 64, 64, 3, 0, 0, 0, 0, d) == -2          # fp32 -> bf16 has no kernel
    assert lib.vqk_conv_fprop_form_name(99, 0) == b'?' and lib.vqk_conv_fprop_form_name(-1, 1) == b'?'


def test_label_matches_the_plan(lib):
    """ops._fprop_event asks the library only while events are recorded, and reports a memory-bound form with 0 FLOPs"""
    ops = importlib.import_module(PKG + '.ops')
    x = torch.empty(1, 256, 64, 64, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert ops.KERNEL_EVENTS is None and ops._fprop_event(x, torch.bfloat16, 128, 1, False, 0, 1, 5.0) == ('', 5.0)
    ops.KERNEL_EVENTS = []
    try:
        assert ops._fprop_event(x, torch.bfloat16, 128, 1, False, 0, 1, 5.0) == ('conv1x1_mx_kernel<bf16> (HBM)', 0.0)
        assert ops._fprop_event(x, torch.bfloat16, 128, 3, False, 0, 1, 5.0) == ('conv3x3_mx_kernel<bf16>', 5.0)
        assert ops._fprop_event(x, torch.float32, 128, 3, False, 0, 1, 5.0) == ('conv3x3_stream_kernel<bf16>', 5.0)
        assert ops._fprop_event(x, torch.bfloat16, 128, 3, False, 0, 0, 5.0, 8) == ('conv_fprop_kernel<bf16>', 5.0)
        xf = torch.empty(1, 64, 32, 32).contiguous(memory_format=torch.channels_last)
        assert ops._fprop_event(xf, torch.float32, 64, 3, False, 0, 0, 5.0) == ('conv3x3_halo_kernel<f32>', 5.0)
        assert ops._fprop_event(xf, torch.float32, 4, 3, False, 0, 0, 5.0) == ('conv3x3_thin_out_f32_kernel (HBM)', 0.0)
    finally:
        ops.KERNEL_EVENTS = None


# ---------------------------------------------------------------------------------------------------------------------------------
# the sweep: the layout ops.weight_layout names is one the plan serves.  Shapes where the launcher before the plan function already
# refused the layout its own query named would be listed here as (dtype, out_dtype, ksize, ups, cin, cout, h, w); none was found.
KNOWN_REFUSALS = set()
DT = {T.F32: torch.float32, T.BF16: torch.bfloat16}


def test_weight_layout_is_never_refused(lib):
    ops = importlib.import_module(PKG + '.ops')
    chans = (4, 8, 32, 64, 96, 128, 256)
    maps = ((4, 4), (8, 32), (16, 16), (16, 48), (24, 24), (12, 32), (32, 32), (64, 64), (8, 200), (136, 16))
    seen, refused = set(), []
    for (dt, odt), k, ups, cin, cout, (h, w), x3 in itertools.product(
            ((T.F32, T.F32), (T.BF16, T.BF16), (T.BF16, T.F32)), (1, 3), (0, 1), chans, chans, maps, (False, True)):
        if cin % (4 if dt == T.F32 else 8):
            continue
        for variant in (-1, 2, 5):
            lib.vqk_conv_set_variant(variant)
            try:
                layout = ops.weight_layout(DT[dt], 2, h, w, cin, cout, k, bool(ups), DT[odt], x3=x3)
                form = lib.vqk_conv_fprop_plan(dt, odt, 2, h, w, cin, cout, k, ups, 0, layout, 0, None)
            finally:
                lib.vqk_conv_set_variant(-1)
            seen.add(layout)
            if form < 0 and (dt, odt, k, ups, cin, cout, h, w) not in KNOWN_REFUSALS:
                refused.append((dt, odt, k, ups, cin, cout, h, w, variant, layout, form))
    assert seen == {0, 1, 5}
    assert not refused, refused[:20]
