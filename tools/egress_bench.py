"""Measurements of the image egress path; one JSON line.

    python tools/egress_bench.py [--part kernel|evaluate|all] [--images 256] [--windows 5]

Every timed window starts after warm-up and is closed by a device synchronise; each figure is the median of --windows windows
with their minimum and maximum beside it.
  calibration : a 1 GiB device-to-device copy on this box (bytes read + written per second), so lines from different boxes compare;
  kernel      : vqk_egress_u8 alone against the torch formulation of the SAME bytes (slice, mul, add, clamp, mul, add, to(uint8),
                permute, contiguous, and for a panel: a zero fill and one strided copy per cell), in alternating windows, on
                  panel  : the panel of log_reconstructions at the headline size -- 8 fp32 targets over 8 bf16 reconstructions,
                           both padded NHWC with 8 channels, 256^2, padding 2 (two launches);
                  stack  : 32 bf16 padded NHWC reconstructions -> 32 plain images (one launch);
                  nchw   : 32 fp32 NCHW images in [0,1] -> 32 plain images (one launch).
                GB/s = (source bytes the kernel asks for: one 16- / 8-byte vector or three elements per pixel) + canvas bytes, over
                the kernel's time; the equality of the two results is checked before timing;
  evaluate    : the test loop of evaluate.py (standard quantizer, 256^2, batch 32, bf16, seeded synthetic images resident on the
                device) with and without --save_reconstructions, in alternating passes, for 1 / 4 / 16 encode threads: images/s,
                the slowdown, and PNGs/s per thread.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
DEV = torch.device('cuda', 0)


def stats(samples, scale=1.0, digits=2):
    s = sorted(samples)
    return dict(median=round(float(np.median(s)) * scale, digits), min=round(s[0] * scale, digits), max=round(s[-1] * scale, digits))


def windows(fns, count, iters):
    """alternating windows of `iters` calls of each function; seconds per call, per function"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(count):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / iters)
    return out


def calibration():
    src = torch.empty(1 << 30, dtype=torch.uint8, device=DEV).fill_(1)
    dst = torch.empty_like(src)
    (t,) = windows([lambda: dst.copy_(src)], 5, 10)
    return dict(copy_1gib_tb_per_s=stats([2 * src.numel() / x / 1e12 for x in t], digits=3))


def nhwc(n, cpad, dtype, seed, lo=-1.1, hi=1.1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    store = torch.rand(n, 256, 256, cpad, device=DEV, generator=g) * (hi - lo) + lo
    return store.to(dtype).permute(0, 3, 1, 2)


def torch_u8(x, value_range):
    t = x[:, :3].float()
    if value_range == 'sym':
        t = t.mul(0.5).add(0.5)
    return t.clamp(0, 1).mul(255).add(0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def torch_grid(sources, ranges, nrow, pad):
    imgs = torch.cat([torch_u8(s, r) for s, r in zip(sources, ranges)])
    k, h, w, _ = imgs.shape
    cols = min(nrow, k)
    rows = -(-k // cols)
    grid = torch.zeros(rows * (h + pad) + pad, cols * (w + pad) + pad, 3, dtype=torch.uint8, device=imgs.device)
    for i in range(k):
        y0, x0 = pad + (i // cols) * (h + pad), pad + (i % cols) * (w + pad)
        grid[y0:y0 + h, x0:x0 + w].copy_(imgs[i])
    return grid


def asked_bytes(x):
    n, c, h, w = x.shape
    vec = x.stride(1) == 1 and c >= 4
    return n * h * w * (4 * x.element_size() if vec else 3 * x.element_size())


def bench_kernel(ops, count):
    out = {}
    target, recon = nhwc(8, 8, torch.float32, 1), nhwc(8, 8, torch.bfloat16, 2)
    _, _, hg, wg = ops.image_grid_shape(16, 256, 256, 8, 2)
    canvas = torch.empty(hg, wg, 3, dtype=torch.uint8, device=DEV)
    stack_src = nhwc(32, 8, torch.bfloat16, 3)
    nchw = torch.rand(32, 3, 256, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    stack = torch.empty(32, 256, 256, 3, dtype=torch.uint8, device=DEV)
    cases = {
        'panel': (lambda: ops.image_grid_u8([target, recon], 8, 2, value_ranges='sym', out=canvas),
                  lambda: torch_grid([target, recon], ['sym', 'sym'], 8, 2), asked_bytes(target) + asked_bytes(recon) + canvas.numel(), 2),
        'stack': (lambda: ops.egress_u8(stack_src, 'sym', out=stack), lambda: torch_u8(stack_src, 'sym'),
                  asked_bytes(stack_src) + stack.numel(), 1),
        'nchw': (lambda: ops.egress_u8(nchw, 'unit', out=stack), lambda: torch_u8(nchw, 'unit'), asked_bytes(nchw) + stack.numel(), 1),
    }
    for name, (kernel, formulation, moved, launches) in cases.items():
        same = bool(torch.equal(kernel(), formulation()))
        tk, tt = windows([kernel, formulation], count, 200)
        out[name] = dict(launches=launches, bytes_moved=moved, equal_to_torch=same, kernel_us=stats(tk, 1e6),
                         kernel_gb_per_s=stats([moved / x / 1e9 for x in tk], digits=1), torch_us=stats(tt, 1e6),
                         torch_over_kernel=round(float(np.median(tt) / np.median(tk)), 2))
    return out


def bench_evaluate(images_count, count):
    train_mod = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    imagelog = importlib.import_module(PKG + '.imagelog')
    conf = train_mod.get_model_conf(os.path.join(ROOT, 'example_confs', 'standard_vqvae.yaml'))
    torch.manual_seed(0)
    model = model_mod.VQVAE(256, conf['autoencoder'], conf['quantizer'], None, None, load_loss=False,
                            compute_dtype=torch.bfloat16).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    yy, xx = np.mgrid[0:256, 0:256]
    base = torch.from_numpy(np.stack([0.5 + 0.4 * np.sin(xx / 23.0 + c) * np.cos(yy / 31.0 - c) for c in range(3)])).float()
    data = (base[None] + 0.05 * torch.randn(images_count, 3, 256, 256, generator=g)).clamp(0, 1)      # photo-like: smooth + noise
    batches = [data[i:i + 32].to(DEV) for i in range(0, images_count, 32)]
    trainer = trainer_mod.MiniTrainer()

    def run(workers, directory):
        saver = None
        if workers:
            names = [[f'{i + j:06d}.png' for j in range(b.shape[0])] for i, b in zip(range(0, images_count, 32), batches)]
            saver = imagelog.ReconstructionSaver(imagelog.ImageWriter(directory, workers=workers), names, None)
        model.reconstruction_sink = saver
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = trainer.test(model, batches)
        float(out['mse'])
        if saver is not None:
            saver.close()                                            # every file on disk
        torch.cuda.synchronize()
        model.reconstruction_sink = None
        return time.perf_counter() - t0

    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        run(0, None), run(4, os.path.join(tmp, 'warm'))
        for workers in (1, 4, 16):
            plain, saving = [], []
            for k in range(count):
                plain.append(run(0, None))
                saving.append(run(workers, os.path.join(tmp, f'w{workers}_{k}')))
            p, s = float(np.median(plain)), float(np.median(saving))
            size = float(np.mean([os.path.getsize(os.path.join(tmp, f'w{workers}_0', f)) for f in os.listdir(os.path.join(tmp, f'w{workers}_0'))]))
            res[f'threads_{workers}'] = dict(images=images_count, plain_images_per_s=stats([images_count / x for x in plain], digits=1),
                                             saving_images_per_s=stats([images_count / x for x in saving], digits=1),
                                             slowdown=round(s / p, 2), pngs_per_s_per_thread=round(images_count / s / workers, 1),
                                             mean_png_bytes=int(size))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=['kernel', 'evaluate', 'all'], default='all')
    ap.add_argument('--images', type=int, default=256, help='images per pass of the evaluate part')
    ap.add_argument('--windows', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('egress_bench.py measures on an MI355X: no device, no numbers')
    ops = importlib.import_module(PKG + '.ops')
    out = dict(calibration=calibration())
    if args.part in ('kernel', 'all'):
        out['kernel'] = bench_kernel(ops, args.windows)
    if args.part in ('evaluate', 'all'):
        out['evaluate'] = bench_evaluate(args.images, max(3, args.windows - 2))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
