"""Measurements of the dataset ingest path ("Ingest"); one JSON line.

    python tools/ingest_bench.py [--part kernel|decode|step|all] [--images 256] [--steps 40]

Seeded synthetic images are written once into a temporary folder: JPEGs of 500x375 (an ImageNet-like photo size) and of
1600x1200.  Every timed window starts after warm-up and is closed by a device synchronise.
  kernel : vqk_ingest_u8 alone, 32 images -> 256^2: time per launch; bytes moved (source bytes inside the boxes + 4 * N * 3 * S^2
           written) over that time, as a share of the streaming-copy HBM rate (MI355X_MICROARCH.md: about 6.3e12 B/s achievable);
  decode : HOST rate of the decode-and-pack half (no device involved) in images/s for 1, 4, 8, 16 threads;
  step   : the graphed train step (standard quantizer, K = 1024, 256^2, batch 32, bf16: the headline configuration of bench.py)
           fed by the folder loader against the SAME step on a tensor resident on the device, in the same process, alternating
           windows of --steps steps; the difference is what the loader leaves exposed.
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
HBM_COPY_BPS = 6.3e12


def write_images(folder: str, count: int, h: int, w: int, seed: int) -> None:
    """photo-like content (smooth structure, some noise: a JPEG of ordinary entropy), seeded"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    os.makedirs(folder, exist_ok=True)
    for k in range(count):
        f = rng.uniform(20, 90, size=6)
        base = np.stack([127 + 100 * np.sin(xx / f[c] + k) * np.cos(yy / f[c + 3] - c) for c in range(3)], axis=2)
        img = np.clip(base + rng.normal(0, 8, size=(h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(folder, f'{k:05d}.jpg'), quality=90)


def bench_kernel(ops, h: int, w: int, n: int = 32, size: int = 256, iters: int = 50) -> dict:
    dev = torch.device('cuda', 0)
    desc = ops.ingest_desc([(h, w)] * n)
    nbytes = ops.ingest_packed_bytes(desc)
    pixels = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev)
    desc_dev = torch.from_numpy(desc.view(np.uint8)).to(dev)
    out = torch.empty(n, 3, size, size, device=dev)
    for _ in range(5):
        ops.ingest_u8(pixels, desc, size, out=out, desc_dev=desc_dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        ops.ingest_u8(pixels, desc, size, out=out, desc_dev=desc_dev)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    moved = n * 3 * h * w + 4 * n * 3 * size * size
    return dict(source=f'{w}x{h}', n=n, out=size, us=round(dt * 1e6, 1), bytes_moved=moved, gb_per_s=round(moved / dt / 1e9, 1),
                share_of_hbm_copy_rate=round(moved / dt / HBM_COPY_BPS, 4))


def bench_decode(data, folder: str, threads: int, batch: int = 32) -> dict:
    loader = data.DeviceImageLoader(folder, 256, batch, workers=threads, staging_bytes=batch * 3 * 1600 * 1200)
    n = 0
    t0 = time.perf_counter()
    pipe = loader.host_pipeline()
    for hb in pipe:
        n += len(hb.indices)
        pipe.release(hb.slot)
    dt = time.perf_counter() - t0
    pipe.close()
    loader.close()
    return dict(threads=threads, images=n, host_images_per_s=round(n / dt, 1))


def bench_step(data, folder: str, workers: int, steps: int, rounds: int = 3) -> dict:
    train_mod = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    dev = torch.device('cuda', 0)
    conf = train_mod.get_model_conf(os.path.join(ROOT, 'example_confs', 'standard_vqvae.yaml'))
    run = train_mod.derive_run_config(conf, 1, {'training.cumulative_bs': 32, 'image_size': 256})
    torch.manual_seed(0)
    model = model_mod.VQVAE(run['image_size'], run['ae_conf'], run['q_conf'], run['l_conf'], run['t_conf'],
                            compute_dtype=torch.bfloat16).to(dev).train()
    trainer = trainer_mod.MiniTrainer(num_training_batches=10 ** 6)
    trainer.attach(model)
    model.on_train_start()
    loader = data.DeviceImageLoader(folder, 256, 32, workers=workers, device=dev, shuffle=True, drop_last=True, seed=0,
                                    staging_bytes=32 * 3 * 512 * 512)
    resident = next(iter(loader)).clone()
    trainer.capture(model, resident, warmup=2)

    def window_resident():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            trainer.train_batch_graphed(model, resident, i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    epoch = [0]

    def window_loader():
        done = 0
        it = iter(loader)
        first = next(it)                                             # the pipeline is primed: start-up is not the steady state
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.train_batch_graphed(model, first, 0)
        done += 1
        while done < steps:
            for batch in it:
                trainer.train_batch_graphed(model, batch, done)
                done += 1
                if done == steps:
                    break
            else:
                epoch[0] += 1
                loader.set_epoch(epoch[0])
                it = iter(loader)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    window_resident(), window_loader()                               # warm-up of both paths
    res, ldr = [], []
    for _ in range(rounds):
        res.append(window_resident())
        ldr.append(window_loader())
    loader.close()
    r, l = float(np.median(res)), float(np.median(ldr))
    return dict(workers=workers, steps_per_window=steps, rounds=rounds, resident_ms=round(r * 1e3, 3), loader_ms=round(l * 1e3, 3),
                exposed_ms=round((l - r) * 1e3, 3), resident_images_per_s=round(32 / r, 1), loader_images_per_s=round(32 / l, 1),
                resident_windows_ms=[round(x * 1e3, 3) for x in res], loader_windows_ms=[round(x * 1e3, 3) for x in ldr])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=['kernel', 'decode', 'step', 'all'], default='all')
    ap.add_argument('--images', type=int, default=256, help='images written per size')
    ap.add_argument('--steps', type=int, default=40, help='train steps per timed window')
    ap.add_argument('--workers', type=int, default=16)
    args = ap.parse_args()
    data = importlib.import_module(PKG + '.data')
    ops = importlib.import_module(PKG + '.ops')
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        small, large = os.path.join(tmp, 'photo'), os.path.join(tmp, 'large')
        if args.part in ('decode', 'step', 'all'):
            write_images(small, args.images, 375, 500, 0)
        if args.part in ('decode', 'all'):
            write_images(large, max(32, args.images // 4), 1200, 1600, 1)
        if args.part in ('kernel', 'all'):
            out['kernel'] = [bench_kernel(ops, 375, 500), bench_kernel(ops, 1200, 1600)]
        if args.part in ('decode', 'all'):
            out['host_decode_500x375'] = [bench_decode(data, small, t) for t in (1, 4, 8, 16)]
            out['host_decode_1600x1200'] = [bench_decode(data, large, t) for t in (1, 4, 8, 16)]
        if args.part in ('step', 'all'):
            out['step'] = bench_step(data, small, args.workers, args.steps)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
