"""Finite-scalar-quantizer timings on one GPU, device events after warm-up, the contenders alternating in one process:
(a) the fused forward / backward kernels (csrc/fsq.hip) against the same computation in plain torch ops on the device,
(b) both against the kernels of the codebook lookup (VQLookupFn's, K = 1024) on the same rows,
(c) the graphed headline train step (batch 32 at 256x256, bf16) with the `standard` quantizer against `fsq`.
N = 8192 rows (32 images x 16x16), D = 256, levels [8,5,5,5] and [8,8,8,5,5,5].  Writes profiles/fsq_bench.txt (--out)."""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
DEV = 'cuda:0'


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3            # us


def alternate(contenders: dict, iters: int, rounds: int) -> dict:
    """every contender warmed up, then `rounds` passes over all of them in turn; median us per call and the spread"""
    for fn in contenders.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, fn in contenders.items():
            times[name].append(timed(fn, iters))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def torch_fsq(levels):
    lv = torch.tensor(levels, dtype=torch.float32, device=DEV)
    half_l = (lv - 1) * (1 + 1e-3) / 2
    offset = torch.where(lv % 2 == 0, 0.5, 0.0)
    shift = torch.atanh(offset / half_l)
    hw = torch.floor(lv / 2)
    basis = torch.cumprod(torch.cat([torch.ones(1, device=DEV), lv[:-1]]), 0)
    k = int(np.prod(levels))

    def fwd(z, w_in, b_in, w_out, b_out):
        u = torch.addmm(b_in, z, w_in.t())
        t = torch.tanh(u + shift)
        r = torch.round(t * half_l - offset)
        c = r / hw
        idx = ((r + hw) * basis).sum(-1).long()
        hist = torch.bincount(idx, minlength=k)
        q = torch.addmm(b_out, c, w_out.t()).to(torch.bfloat16)
        return q, idx, hist, t, c

    def bwd(z, t, c, dq, w_in, w_out):
        dq = dq.float()
        du = (dq @ w_out) / hw * half_l * (1 - t * t)
        return du @ w_in, du.t() @ z, du.sum(0), dq.t() @ c, dq.sum(0)
    return fwd, bwd


def kernels(out, n, dm, levels, iters, rounds):
    g = torch.Generator().manual_seed(1)
    d = len(levels)
    z = torch.randn(n, dm, generator=g).to(DEV)
    w_in = ((torch.rand(d, dm, generator=g) * 2 - 1) * 2 / dm ** 0.5).to(DEV)
    b_in = (torch.rand(d, generator=g) - 0.5).to(DEV)
    w_out = (torch.rand(dm, d, generator=g) * 2 - 1).to(DEV)
    b_out = (torch.rand(dm, generator=g) - 0.5).to(DEV)
    dq = torch.randn(n, dm, generator=g).to(DEV).to(torch.bfloat16)
    tfwd, tbwd = torch_fsq(levels)
    _, tidx, _, tt, tc = tfwd(z, w_in, b_in, w_out, b_out)

    native = importlib.import_module(PKG + '._native')
    lib, st = native.lib(), ops._stream()
    lv, _, k = ops._levels_arg(levels)
    idx = torch.empty(n, dtype=torch.int64, device=DEV)
    u = torch.empty(n, d, device=DEV)
    q = torch.empty(n, dm, dtype=torch.bfloat16, device=DEV)
    hist = torch.zeros(k, dtype=torch.int32, device=DEV)
    dz = torch.empty(n, dm, device=DEV)
    grads = [torch.empty_like(p) for p in (w_in, b_in, w_out, b_out)]
    ws = torch.empty(lib.vqk_fsq_backward_ws_bytes(n, dm, d), dtype=torch.uint8, device=DEV)

    def fused_fwd():
        hist.zero_()
        native.check(lib.vqk_fsq_forward(z.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), n, dm, d, lv,
                                         idx.data_ptr(), u.data_ptr(), 0, q.data_ptr(), hist.data_ptr(), st), 'fsq_forward')

    def fused_bwd():
        native.check(lib.vqk_fsq_backward(z.data_ptr(), u.data_ptr(), dq.data_ptr(), 1, w_in.data_ptr(), w_out.data_ptr(), n, dm, d, lv,
                                          dz.data_ptr(), *(t.data_ptr() for t in grads), 0, ws.data_ptr(), ws.numel(), st), 'fsq_backward')

    fused_fwd()
    agree = float((idx == tidx).float().mean())

    # the codebook lookup on the same rows: a trained-like codebook (codes = perturbed latents), K = 1024
    kk = 1024
    zs = (z * 0.36).contiguous()
    e = (zs[torch.randperm(n, generator=g)[:kk].to(DEV)] + 0.01 * torch.randn(kk, dm, device=DEV)).contiguous()
    vws = torch.empty(lib.vqk_vq_filter_ws_bytes(kk, dm), dtype=torch.uint8, device=DEV)
    native.check(lib.vqk_vq_prepare_f32(e.data_ptr(), kk, dm, vws.data_ptr(), vws.numel(), st), 'vq_prepare')
    vbuf = torch.zeros(kk + 1, dtype=torch.int32, device=DEV)
    de = torch.empty(kk, dm, device=DEV)
    gs = torch.ones((), device=DEV)

    def lookup_fwd():
        vbuf.zero_()
        native.check(lib.vqk_vq_forward_f32(zs.data_ptr(), e.data_ptr(), vws.data_ptr(), vws.numel(), n, kk, dm, 0, idx.data_ptr(), 0,
                                            q.data_ptr(), vbuf[kk:].data_ptr(), vbuf.data_ptr(), st), 'vq_forward')

    lookup_fwd()
    vidx = idx.clone()

    def lookup_bwd():
        de.zero_()
        native.check(lib.vqk_vq_backward_fused_f32(zs.data_ptr(), e.data_ptr(), vidx.data_ptr(), dq.data_ptr(), 1, n, kk, dm,
                                                   0.25 * 2.0 / (n * dm), 2.0 / (n * dm), gs.data_ptr(), dz.data_ptr(), de.data_ptr(), st),
                     'vq_backward_fused')

    res = alternate({'fsq fused forward (fill + 1 kernel)': fused_fwd,
                     'fsq torch-ops forward': lambda: tfwd(z, w_in, b_in, w_out, b_out),
                     'vq lookup forward K=1024 (fill + 1 kernel)': lookup_fwd,
                     'fsq fused backward (kernel + slab sum)': fused_bwd,
                     'fsq torch-ops backward': lambda: tbwd(z, tt, tc, dq, w_in, w_out),
                     'vq lookup backward K=1024 (fill + 1 kernel)': lookup_bwd}, iters, rounds)
    print(f'N = {n}, D = {dm}, levels = {list(levels)} (K = {int(np.prod(levels))}); tokens equal to the torch-ops evaluation on '
          f'{agree * 100:.3f} % of rows (random latents: no boundary rows removed)', file=out)
    for name, (med, lo, hi) in res.items():
        print(f'  {name:44s} {med:9.2f} us   (min {lo:.2f}, max {hi:.2f}; {rounds} rounds x {iters} calls, host-issued launches)', file=out)
    moved = n * dm * 4 + n * dm * 2 + n * (8 + 4 * d)
    med = res['fsq fused forward (fill + 1 kernel)'][0]
    print(f'  forward moves {moved / 1e6:.1f} MB: {moved / med / 1e6:.2f} TB/s at the fused time', file=out)


def train_step(out, steps, rounds):
    train = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    images = torch.rand(32, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(DEV)
    runs = {}
    for name in ('standard', 'fsq'):
        conf = train.get_model_conf(os.path.join(ROOT, 'example_confs', f'{name}_vqvae.yaml'))
        run = train.derive_run_config(conf, 1, {'training.cumulative_bs': 32})
        torch.manual_seed(0)
        m = model_mod.VQVAE(run['image_size'], run['ae_conf'], run['q_conf'], run['l_conf'], run['t_conf'],
                            compute_dtype=torch.bfloat16).to(DEV).train()
        tr = trainer_mod.MiniTrainer(num_training_batches=1000)
        tr.attach(m)
        m.on_train_start()
        tr.capture(m, images, warmup=3)
        counter = [3]

        def step(m=m, tr=tr, counter=counter):
            tr.train_batch_graphed(m, images, counter[0])
            counter[0] += 1
        runs[f'{name}_vqvae.yaml'] = step
    res = alternate(runs, steps, rounds)
    print('graphed train step, batch 32 at 256x256, bf16 (zero_grad + forward + backward replayed, AdamW launch after it)', file=out)
    for name, (med, lo, hi) in res.items():
        print(f'  {name:24s} {med / 1e3:8.3f} ms/step  {32 / med * 1e6:8.1f} images/s   (min {lo / 1e3:.3f}, max {hi / 1e3:.3f} ms; '
              f'{rounds} rounds x {steps} steps)', file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fsq_bench.txt'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-train-step', action='store_true')
    args = ap.parse_args()
    with open(args.out, 'w') as out:
        print(f'tools/fsq_bench.py on {torch.cuda.get_device_name(0)}: medians of device-event timings, contenders alternating in one '
              'process.', file=out)
        for levels in ((8, 5, 5, 5), (8, 8, 8, 5, 5, 5)):
            kernels(out, 8192, 256, levels, args.iters, args.rounds)
            out.flush()
        if not args.no_train_step:
            train_step(out, args.steps, args.rounds)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
