"""Measurements of the optimizer step guard; one JSON line.

    python tools/stepguard_bench.py [--part kernel|step|gan|all] [--steps 40] [--out FILE]

Every timed window starts after warm-up and is closed by a device synchronise; reported is the median of 3 (5 for the kernels)
with min / max, the variants alternating inside one process.
  kernel : on the headline model's autoencoder arena (standard quantizer, 256^2, bf16 shadow on: the configuration of bench.py)
           vqk_adamw against ITSELF in alternating windows (the run-to-run spread every other number is read against),
           vqk_adamw_guarded applied (control block left by one vqk_step_guard call), vqk_adamw_guarded skipped (apply = 0: every
           block returns after the control block), vqk_step_guard alone, and the guard's own one-group vqk_arena_stats pass;
  step   : the graphed headline step (bf16, batch 32) with the guard off, on, and on with a scalar log attached (the statistics
           pass is then the log's: one pass per step), alternating windows of --steps steps;
  gan    : the same for the graphed VQ-GAN step (gumbel_vqgan.yaml, adversarial phase, batch 16, both optimizers guarded).
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
HBM_COPY_BPS = 6.29e12            # MI355X_MICROARCH.md: the measured streaming-copy rate (read + write bytes per second)


def _stats(values, unit):
    return {'median_' + unit: round(float(np.median(values)), 3), 'min_' + unit: round(float(min(values)), 3),
            'max_' + unit: round(float(max(values)), 3)}


def bench_kernel() -> dict:
    from scalarlog_bench import build
    ops = importlib.import_module(PKG + '.ops')
    native = importlib.import_module(PKG + '._native')
    model, trainer, batch = build(False)
    opt = trainer.optimizers[0]
    trainer.capture(model, batch, warmup=2)
    for i in range(3):
        trainer.train_batch_graphed(model, batch, i)                  # real gradients in the arena, non-trivial moments
    opt.enable_guard(skip_nonfinite=True, max_grad_norm=1e9)
    gd, g0 = opt.guard, opt.param_groups[0]
    b1, b2 = g0['betas']
    lib, stream = native.lib(), torch.cuda.current_stream().cuda_stream
    n = opt.flat_p.numel()
    common = (opt.flat_p.data_ptr(), opt.flat_g.data_ptr(), 0 if opt.flat_m is None else opt.flat_m.data_ptr(), opt.flat_v.data_ptr(), n,
              opt.seg_end.data_ptr(), opt.seg_wd.data_ptr(), opt.seg_end.numel(), float(g0['lr']), float(b1), float(b2), float(g0['eps']))
    shadow = 0 if opt.shadow is None else opt.shadow.data_ptr()

    def adamw():
        native.check(lib.vqk_adamw(*common, 100, 1.0, shadow, stream), 'adamw')

    def guarded():
        native.check(lib.vqk_adamw_guarded(*common, gd['ctrl'].data_ptr(), shadow, stream), 'adamw_guarded')

    def stats():
        ops.arena_stats(opt.flat_g, opt.seg_end, gd['seg_group'], 1, 1.0, gd['ws'], gd['out'])

    def guard():
        native.check(lib.vqk_step_guard(gd['out'][3:6].data_ptr(), 1, 1e9, float(g0['lr']), 1.0, gd['bias'].data_ptr(), gd['bias'].shape[0],
                                        gd['state'].data_ptr(), gd['ctrl'].data_ptr(), stream), 'step_guard')

    def window(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    stats()
    gd['state'][0] = 99.0                                             # the control block of step 100, as vqk_adamw(step = 100) above
    guard()
    torch.cuda.synchronize()
    applied_ctrl = gd['ctrl'].clone()
    skipped_ctrl = applied_ctrl.clone()
    skipped_ctrl[0] = 0
    variants = {'adamw_a': (adamw, applied_ctrl, 20), 'adamw_b': (adamw, applied_ctrl, 20), 'guarded_applied': (guarded, applied_ctrl, 20),
                'guarded_skipped': (guarded, skipped_ctrl, 200), 'step_guard': (guard, applied_ctrl, 200), 'arena_stats_1group': (stats, applied_ctrl, 50)}
    times = {k: [] for k in variants}
    for rnd in range(6):                                              # round 0 warms every variant up
        for name, (fn, ctrl, iters) in variants.items():
            gd['ctrl'].copy_(ctrl)
            dt = window(fn, iters)
            if rnd:
                times[name].append(dt)
    moved = n * 4 * (2 * 2 + 1 + (2 if opt.flat_m is not None else 0)) + (n * 2 if opt.shadow is not None else 0)      # p, v read + write; g read
    out = dict(arena_elements=n, bytes_moved_per_adamw=moved, shadow=opt.shadow is not None, windows_per_variant=5)
    for name, v in times.items():
        out[name] = _stats(v, 'us')
    out['adamw_a']['gb_per_s'] = round(moved / (out['adamw_a']['median_us'] * 1e-6) / 1e9, 1)
    out['guarded_applied']['gb_per_s'] = round(moved / (out['guarded_applied']['median_us'] * 1e-6) / 1e9, 1)
    out['adamw_self_spread_percent'] = round(100.0 * abs(out['adamw_a']['median_us'] - out['adamw_b']['median_us']) / out['adamw_a']['median_us'], 3)
    out['guarded_vs_adamw_percent'] = round(100.0 * (out['guarded_applied']['median_us'] - out['adamw_a']['median_us']) / out['adamw_a']['median_us'], 3)
    return out


def bench_step(gan: bool, steps: int) -> dict:
    from scalarlog_bench import build
    scalarlog = importlib.import_module(PKG + '.scalarlog')
    model, trainer, batch = build(gan)
    trainer.enable_guards(True, 1.0)                                  # before the capture; skipping and clipping both on
    guards = [o.guard for o in trainer.optimizers]
    trainer.capture(model, batch, warmup=2)
    log = scalarlog.ScalarLog(None, grad_stats_every=1)
    count = [0]

    def window(mode):
        for o, gd in zip(trainer.optimizers, guards):
            o.guard = None if mode == 'off' else gd
        model.scalar_log = log if mode == 'on_log' else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            trainer.train_batch_graphed(model, batch, count[0] % 1000)
            count[0] += 1
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps * 1e3
        if mode == 'on_log':
            log.epoch_end('train_epoch', 0, trainer.global_step)      # (outside the window: the epoch's one copy)
        return dt
    modes = ('off', 'on', 'on_log')
    for mode in modes:
        window(mode)                                                  # warm-up of every path
    times = {mode: [] for mode in modes}
    for _ in range(3):
        for mode in modes:
            times[mode].append(window(mode))
    med = {mode: float(np.median(v)) for mode, v in times.items()}
    arena = sum(o.flat_g.numel() * 4 for o in trainer.optimizers)
    states = [o.guard_state() for o in trainer.optimizers]
    out = dict(config='gumbel_vqgan bs16' if gan else 'standard bs32', steps_per_window=steps, arena_bytes=arena,
               guard_exposed_us=round((med['on'] - med['off']) * 1e3, 1), guard_exposed_percent=round(100.0 * (med['on'] - med['off']) / med['off'], 3),
               guard_with_log_exposed_us=round((med['on_log'] - med['off']) * 1e3, 1),
               guard_with_log_exposed_percent=round(100.0 * (med['on_log'] - med['off']) / med['off'], 3),
               expected_from_bytes_us=round(arena / HBM_COPY_BPS * 1e6 + 3 * 2.0, 1),
               guard_counts=[{k: s[k] for k in ('applied', 'skipped', 'clipped')} for s in states])
    for mode in modes:
        out[mode] = _stats(times[mode], 'ms')
        out[mode]['windows_ms'] = [round(x, 4) for x in times[mode]]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=['kernel', 'step', 'gan', 'all'], default='all')
    ap.add_argument('--steps', type=int, default=40, help='train steps per timed window')
    ap.add_argument('--out', type=str, default=None, help='also write the JSON to this file')
    args = ap.parse_args()
    out = {}
    if args.part in ('kernel', 'all'):
        out['kernel'] = bench_kernel()
    if args.part in ('step', 'all'):
        out['step'] = bench_step(False, args.steps)
    if args.part in ('gan', 'all'):
        out['gan'] = bench_step(True, args.steps)
    text = json.dumps(out)
    if args.out:
        with open(args.out, 'w', encoding='utf-8') as f:
            f.write(text + '\n')
    print(text, flush=True)


if __name__ == '__main__':
    main()
