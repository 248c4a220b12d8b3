#!/usr/bin/env python
"""Grouped 3x3 weight-gradient launch (vqk_conv3x3_wgrad_group) against the per-layer launches it replaces, on the headline step's
own list of <= 32x32 layers at batch 32 (profiles/round6_per_shape.txt: 21 launches of conv3x3_wgrad_mx_kernel<bf16> k3).

    python tools/wgrad_group_bench.py [--reps 30] [--out profiles/wgrad_group_bench.txt]

Both forms run back to back on one stream, HIP events around ``--reps`` repetitions of the whole list after warm-up; the grouped
form in the two launches the step issues (16 layers, then 5) and with each stage's layers alone.  Then the partition thresholds
(tuning slots WGRAD_GROUP_LOAD_PCT, WGRAD_GROUP_MIN_PPS) are swept.  Operands are random (MFMA power depends on them: DESIGN.md §3)."""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd.ops')
native = importlib.import_module('vqvae-vqgan-pytorch-lightning_amd._native')

BATCH = 32
# (cin, cout, h = w, count) in the order the backward meets them: the decoder's deep levels, then the encoder's
DECODER = [(512, 512, 32, 3), (256, 512, 32, 1), (512, 512, 16, 4), (256, 512, 16, 1)]
ENCODER = [(512, 256, 16, 1), (512, 512, 16, 4), (256, 256, 16, 3), (256, 256, 32, 4)]


def layers(spec):
    out = []
    for cin, cout, hw, count in spec:
        for _ in range(count):
            x = torch.randn(BATCH, cin, hw, hw, device='cuda').to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            dy = torch.randn(BATCH, cout, hw, hw, device='cuda').to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            dw = torch.zeros(cout, 3, 3, cin, device='cuda').permute(0, 3, 1, 2)
            out.append((x, dy, dw))
    return out


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def grouped(items):
    for i in range(0, len(items), 16):
        st, _, _ = ops.raw_conv_wgrad_group(items[i:i + 16])
        native.check(st, 'conv3x3_wgrad_group')


def per_layer(items):
    for x, dy, dw in items:
        ops.raw_conv_wgrad(x, dy, 3, False, out=dw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lib = native.lib()
    dec, enc = layers(DECODER), layers(ENCODER)
    every = dec + enc
    flops = sum(2.0 * x.shape[0] * x.shape[2] * x.shape[3] * x.shape[1] * dy.shape[1] * 9 for x, dy, _ in every)
    lines = [f'# tools/wgrad_group_bench.py --reps {args.reps}: {len(every)} layers, {flops / 1e12:.3f} TFLOP, batch {BATCH}, bf16; ms per pass over the list']

    def row(tag, ms):
        lines.append(f'{tag:<58s} {ms:7.3f} ms  {flops / ms / 1e9:7.1f} TFLOP/s')
        print(lines[-1], flush=True)

    row('per-layer launches (vqk_conv2d_wgrad x 21, one stream)', timed(lambda: per_layer(every), args.reps))
    _, splits, launches = ops.raw_conv_wgrad_group(every, plan_only=True)
    row(f'grouped, as the step issues them (16 + 5): {launches} launches', timed(lambda: grouped(every), args.reps))
    lines.append(f'#   splits per layer: {splits}')
    ms_d, ms_e = timed(lambda: grouped(dec), args.reps), timed(lambda: grouped(enc), args.reps)
    lines.append(f'grouped, the decoder\'s {len(dec)} / the encoder\'s {len(enc)} layers alone: {ms_d:.3f} + {ms_e:.3f} = {ms_d + ms_e:.3f} ms')
    print(lines[-1], flush=True)
    row('per-layer launches again (drift check)', timed(lambda: per_layer(every), args.reps))
    lines.append('# sweep of the partition thresholds (grouped, 16 + 5)')
    for pct in (50, 75, 100, 150, 200, 100000):
        for min_pps in (4, 16):
            if min_pps == 16 and pct != 100:
                continue
            native.check(lib.vqk_set_tuning(b'WGRAD_GROUP_LOAD_PCT', pct), 'set_tuning')
            native.check(lib.vqk_set_tuning(b'WGRAD_GROUP_MIN_PPS', min_pps), 'set_tuning')
            _, splits, _ = ops.raw_conv_wgrad_group(every, plan_only=True)
            row(f'LOAD_PCT {pct:6d} MIN_PPS {min_pps:2d} (split layers {sum(s > 1 for s in splits):2d}, max split {max(splits)})',
                timed(lambda: grouped(every), args.reps))
    lib.vqk_reset_tuning()
    native.apply_env_tuning(lib)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
