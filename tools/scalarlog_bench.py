"""Measurements of the scalar log; one JSON line.

    python tools/scalarlog_bench.py [--part kernel|step|gan|all] [--steps 40]

Every timed window starts after warm-up and is closed by a device synchronise; reported is the median of 3.
  kernel : vqk_arena_stats over the headline model's autoencoder gradient arena (standard quantizer, K = 1024, 256^2: the
           configuration of bench.py) next to vqk_calib_copy over the same number of bytes (the streaming-copy yardstick: it moves
           twice the bytes, read + write) -- 'warm': launches back to back (an arena below 256 MiB stays in the Infinity Cache),
           'cold': each launch behind a 1 GiB fill that evicts it, timed with events; 'behind_step': the launch as the trainer
           issues it, right after the backward of a graphed step, timed with events;
  step   : the graphed headline step (bf16, batch 32) without a log, with the scalar path only (--grad_stats_every 0) and with
           the whole log, in ONE process, alternating windows of --steps steps: the differences are the exposed cost;
  gan    : the same for the graphed VQ-GAN step (gumbel_vqgan.yaml, adversarial phase, batch 16).
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
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
HBM_COPY_BPS = 6.29e12            # MI355X_MICROARCH.md: the measured streaming-copy rate (read + write bytes per second)


def build(gan: bool):
    train_mod = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    dev = torch.device('cuda', 0)
    conf = train_mod.get_model_conf(os.path.join(ROOT, 'example_confs', 'gumbel_vqgan.yaml' if gan else 'standard_vqvae.yaml'))
    over = {'training.cumulative_bs': 16 if gan else 32, 'image_size': 256}
    if gan:
        over['loss.adversarial_params.start_epoch'] = 0
    run = train_mod.derive_run_config(conf, 1, over)
    torch.manual_seed(0)
    model = model_mod.VQVAE(run['image_size'], run['ae_conf'], run['q_conf'], run['l_conf'], run['t_conf'],
                            compute_dtype=torch.bfloat16).to(dev).train()
    if gan:
        model.criterion.discriminator.compute_dtype = model.compute_dtype
        model.criterion.perceptual_loss.net.compute_dtype = model.compute_dtype
    trainer = trainer_mod.MiniTrainer(num_training_batches=10 ** 6)
    trainer.attach(model)
    model.on_train_start()
    batch = torch.rand(run['batch_size_per_device'], 3, 256, 256, device=dev)
    return model, trainer, batch


def _median3(fn):
    return float(np.median([fn() for _ in range(3)]))


def bench_kernel(steps: int) -> dict:
    ops = importlib.import_module(PKG + '.ops')
    native = importlib.import_module(PKG + '._native')
    scalarlog = importlib.import_module(PKG + '.scalarlog')
    model, trainer, batch = build(False)
    opt = trainer.optimizers[0]
    log = scalarlog.ScalarLog(None)
    model.scalar_log = log
    trainer.capture(model, batch, warmup=2)
    for i in range(3):
        trainer.train_batch_graphed(model, batch, i)                  # builds the group table, leaves real gradients in the arena
    st = log._opts['autoencoder']
    nbytes = opt.flat_g.numel() * 4
    acc = torch.zeros(4 * ops.ARENA_ACC, dtype=torch.float64, device=batch.device)
    dst = torch.empty_like(opt.flat_g)
    evict = torch.empty(1 << 28, dtype=torch.float32, device=batch.device)
    lib, stream = native.lib(), torch.cuda.current_stream().cuda_stream

    def stats():
        ops.arena_stats(opt.flat_g, opt.seg_end, st['seg_group'], 3, 1.0, st['ws'], st['out'], acc)

    def copy():
        native.check(lib.vqk_calib_copy(opt.flat_g.data_ptr(), dst.data_ptr(), nbytes, stream), 'calib_copy')

    def warm(fn, iters=50):
        def window():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters
        window()
        return _median3(window)

    def cold(fn, iters=5):
        def window():
            total = 0.0
            for _ in range(iters):
                evict.fill_(1.0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                total += e0.elapsed_time(e1) * 1e-3
            return total / iters
        window()
        return _median3(window)

    out = dict(arena_elements=opt.flat_g.numel(), arena_bytes=nbytes, segments=int(opt.seg_end.numel()),
               blocks=ops.arena_stats_ws_doubles(opt.flat_g.numel(), 3) // 9)
    for name, fn, moved in (('arena_stats', stats, nbytes), ('calib_copy', copy, 2 * nbytes)):
        for mode, timer in (('warm', warm), ('cold', cold)):
            dt = timer(fn)
            out[f'{name}_{mode}_us'] = round(dt * 1e6, 2)
            out[f'{name}_{mode}_gb_per_s'] = round(moved / dt / 1e9, 1)
            out[f'{name}_{mode}_share_of_copy_rate'] = round(moved / dt / HBM_COPY_BPS, 4)
    # as the trainer issues it: behind the backward of a graphed step
    events = []
    real = log.grad_stats

    def timed(o, name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(o, name)
        e1.record()
        events.append((e0, e1))
    log.grad_stats = timed

    def behind():
        events.clear()
        for i in range(steps):
            trainer.train_batch_graphed(model, batch, i)
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(b) for a, b in events])) * 1e-3
    behind()
    dt = _median3(behind)
    out['arena_stats_behind_step_us'] = round(dt * 1e6, 2)
    out['arena_stats_behind_step_gb_per_s'] = round(nbytes / dt / 1e9, 1)
    return out


def bench_step(gan: bool, steps: int) -> dict:
    scalarlog = importlib.import_module(PKG + '.scalarlog')
    model, trainer, batch = build(gan)
    trainer.capture(model, batch, warmup=2)
    logs = {'off': None, 'scalars': scalarlog.ScalarLog(None, grad_stats_every=0), 'full': scalarlog.ScalarLog(None, grad_stats_every=1)}
    count = [0]

    def window(mode):
        model.scalar_log = logs[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            trainer.train_batch_graphed(model, batch, count[0] % 1000)
            count[0] += 1
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        if logs[mode] is not None:
            logs[mode].epoch_end('train_epoch', 0, trainer.global_step)          # (outside the window: the epoch's one copy)
        return dt
    for mode in logs:
        window(mode)                                                  # warm-up of every path
    times = {mode: [] for mode in logs}
    for _ in range(3):
        for mode in logs:
            times[mode].append(window(mode))
    med = {mode: float(np.median(v)) for mode, v in times.items()}
    arena = sum(o.flat_g.numel() * 4 for o in trainer.optimizers)
    return dict(config='gumbel_vqgan bs16' if gan else 'standard bs32', steps_per_window=steps, arena_bytes=arena,
                off_ms=round(med['off'] * 1e3, 4), scalars_ms=round(med['scalars'] * 1e3, 4), full_ms=round(med['full'] * 1e3, 4),
                scalars_exposed_us=round((med['scalars'] - med['off']) * 1e6, 1), full_exposed_us=round((med['full'] - med['off']) * 1e6, 1),
                full_exposed_percent=round(100.0 * (med['full'] - med['off']) / med['off'], 3),
                expected_from_bytes_us=round(arena / HBM_COPY_BPS * 1e6 + 3 * 2.0, 1),
                windows_ms={mode: [round(x * 1e3, 4) for x in v] for mode, v in times.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=['kernel', 'step', 'gan', 'all'], default='all')
    ap.add_argument('--steps', type=int, default=40, help='train steps per timed window')
    args = ap.parse_args()
    out = {}
    if args.part in ('kernel', 'all'):
        out['kernel'] = bench_kernel(args.steps)
    if args.part in ('step', 'all'):
        out['step'] = bench_step(False, args.steps)
    if args.part in ('gan', 'all'):
        out['gan'] = bench_step(True, args.steps)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
