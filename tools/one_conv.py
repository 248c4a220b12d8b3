#!/usr/bin/env python
"""Run ONE conv shape repeatedly (for rocprofv3 --pmc runs).  args: cin cout hw k ups which(fprop|wgrad|phase-...) iters
which = phase-fwd | phase-dgrad | pooled-fprop | pooled-dgrad: the 2x2-tap phase forms, hw = the FULL-resolution side
VQK_ONE_CONV_MODE=x3: fp32 tensors, split products on the bf16 pipe (csrc/conv_x3.hip); f32: the exact-fp32 kernels"""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
cin, cout, hw, k, ups = (int(a) for a in sys.argv[1:6])
which, iters = sys.argv[6], int(sys.argv[7])
mode = os.environ.get('VQK_ONE_CONV_MODE', 'bf16')
dt = torch.bfloat16 if mode == 'bf16' else torch.float32
if mode == 'x3':
    ops.set_conv_products('bf16x3')
n, hin = 32, hw >> ups
x = torch.randn(n, cin, hin, hin, device='cuda').to(dt).contiguous(memory_format=torch.channels_last)
w = (torch.randn(cout, k, k, cin, device='cuda') * 0.05).to(dt)
dy = torch.randn(n, cout, hw, hw, device='cuda').to(dt).contiguous(memory_format=torch.channels_last)
layout = ops.weight_layout(dt, n, hin, hin, cin, cout, k, bool(ups))
wq = ops.pack_weights(w.float().reshape(-1), dt, cout, cin, k, False, layout)
wt = (torch.randn(cout, cin, 3, 3, device='cuda') * 0.05).contiguous(memory_format=torch.channels_last)
half = lambda c: torch.randn(n, c, hw // 2, hw // 2, device='cuda').to(dt).contiguous(memory_format=torch.channels_last)
if which in ('phase-fwd', 'phase-dgrad'):
    xs = half(cin) if which == 'phase-fwd' else dy
    w4 = ops.pack_weights(wt.permute(0, 2, 3, 1).reshape(-1), dt, cout, cin, 3, which == 'phase-dgrad', 2)
elif which == 'pooled-dgrad':
    xs = half(cout)
for _ in range(iters):
    if which == 'phase-fwd':
        assert ops.raw_conv_ups_phase(xs, w4, None, cout, False) is not None
    elif which == 'phase-dgrad':
        assert ops.raw_conv_ups_phase(xs, w4, None, cin, True) is not None
    elif which == 'pooled-fprop':
        assert ops.raw_conv_pooled_fprop_phase(x, wt, None, 0.25) is not None
    elif which == 'pooled-dgrad':
        assert ops.raw_conv_pooled_dgrad_phase(xs, wt, 0.25) is not None
    elif which == 'fprop':
        ops.raw_conv_fprop(x, wq, None, None, k, bool(ups), 0, dt, cout, layout)
    else:
        ops.raw_conv_wgrad(x, dy, k, bool(ups), x3=ops.X3)
torch.cuda.synchronize()
