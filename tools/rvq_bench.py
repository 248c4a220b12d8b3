"""Residual-quantizer timings on one GPU, device events after warm-up, the contenders alternating in one process:
(a) the fused multi-stage forward (csrc/rvq.hip) against the staged formulation (ops.rvq_staged: one lookup kernel per stage + torch
    subtraction / addition) and, at depth 1, against the single-stage forward vqk_vq_forward_f32,
(b) the fused backward (default and deterministic form) against the autograd backward of the staged emulation (one VQLookupFn per stage),
(c) the graphed headline train step (batch 32 at 256x256, bf16) with the `standard` quantizer against `residual` (depth 4).
N = 8192 rows (32 images x 16x16), K = 1024, D = 256, depth 1 / 2 / 4 / 8.  Writes profiles/rvq_bench.txt (--out)."""
import argparse
import importlib
import os
import statistics
import sys

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


def kernels(out, n, k, dm, depth, iters, rounds):
    native = importlib.import_module(PKG + '._native')
    lib, st = native.lib(), ops._stream()
    g = torch.Generator().manual_seed(1)
    # a trained-like codebook: codes = perturbed latents (as tools/fsq_bench.py sizes the lookup)
    z = (torch.randn(n, dm, generator=g) * 0.36).to(DEV).contiguous()
    e = torch.nn.Parameter((z[torch.randperm(n, generator=g)[:k].to(DEV)] + 0.01 * torch.randn(k, dm, device=DEV)).contiguous())
    dq = torch.randn(n, dm, generator=g).to(DEV).to(torch.bfloat16)
    ws = ops.vq_prepared(e)
    idx = torch.empty(n, depth, dtype=torch.int64, device=DEV)
    q = torch.empty(n, dm, dtype=torch.bfloat16, device=DEV)
    zbuf = torch.zeros(depth * k + depth, dtype=torch.int32, device=DEV)
    dz, de, gs = torch.empty(n, dm, device=DEV), torch.empty(k, dm, device=DEV), torch.ones((), device=DEV)
    rws = torch.empty(lib.vqk_rvq_backward_ws_bytes(n, dm, depth), dtype=torch.uint8, device=DEV)
    cz, ce = 0.25 * 2.0 / (n * dm), 2.0 / (n * dm)

    def fused_fwd():
        zbuf.zero_()
        native.check(lib.vqk_rvq_forward_f32(z.data_ptr(), e.data_ptr(), ws.data_ptr(), ws.numel(), n, k, dm, depth, idx.data_ptr(), 0,
                                             q.data_ptr(), zbuf[depth * k:].data_ptr(), zbuf.data_ptr(), st), 'rvq_forward')

    def lookup_fwd():
        zbuf.zero_()
        native.check(lib.vqk_vq_forward_f32(z.data_ptr(), e.data_ptr(), ws.data_ptr(), ws.numel(), n, k, dm, 0, idx.data_ptr(), 0,
                                            q.data_ptr(), zbuf[depth * k:].data_ptr(), zbuf.data_ptr(), st), 'vq_forward')

    def fused_bwd():
        de.zero_()
        native.check(lib.vqk_rvq_backward_f32(z.data_ptr(), e.data_ptr(), idx.data_ptr(), dq.data_ptr(), 1, n, k, dm, depth, cz, ce,
                                              gs.data_ptr(), dz.data_ptr(), de.data_ptr(), rws.data_ptr(), rws.numel(), st), 'rvq_backward')

    def fused_bwd_det():
        native.check(lib.vqk_set_deterministic(1, 0, 0), 'set_deterministic')
        try:
            fused_bwd()
        finally:
            native.check(lib.vqk_set_deterministic(0, 0, 0), 'set_deterministic')

    # the emulation a user writes today: one VQLookupFn per stage on the running residual, autograd through all of them
    img = lambda t: t.view(1, n, 1, dm).permute(0, 3, 1, 2)
    zg = z.clone().requires_grad_(True)
    r, zhat, loss = zg, None, 0.0
    for _ in range(depth):
        qs, _, ls, _ = ops.VQLookupFn.apply(img(r), e, 0.25, True, 0, torch.float32)
        qs = qs.permute(0, 2, 3, 1).reshape(n, dm).detach()
        r, zhat, loss = r - qs, (qs if zhat is None else zhat + qs), loss + ls
    q_st = zg + (zhat - zg).detach()

    def staged_bwd():
        torch.autograd.grad([q_st, loss], [zg, e], [dq.float(), gs], retain_graph=True)

    fused_fwd()
    s_idx = ops.rvq_staged(z, e, depth, want_lo=True)[0]
    agree = bool(torch.equal(idx, s_idx))
    contenders = {'rvq fused forward (fill + 1 kernel)': fused_fwd,
                  'rvq staged forward (ops.rvq_staged)': lambda: ops.rvq_staged(z, e, depth, want_lo=True)}
    if depth == 1:
        contenders['vq lookup forward (fill + 1 kernel)'] = lookup_fwd
    contenders.update({'rvq fused backward, default (fill + 1 kernel)': fused_bwd,
                       'rvq fused backward, deterministic (fill + 2)': fused_bwd_det,
                       'staged autograd backward (VQLookupFn x depth)': staged_bwd})
    res = alternate(contenders, iters, rounds)
    print(f'N = {n}, K = {k}, D = {dm}, depth = {depth}; fused tokens equal to the staged formulation: {agree}', file=out)
    for name, (med, lo, hi) in res.items():
        print(f'  {name:46s} {med:9.2f} us   (min {lo:.2f}, max {hi:.2f}; {rounds} rounds x {iters} calls, host-issued launches)', file=out)
    f, s = res['rvq fused forward (fill + 1 kernel)'], res['rvq staged forward (ops.rvq_staged)']
    print(f'  forward: staged / fused = {s[0] / f[0]:.2f}; the fused median is {s[0] - f[0]:.2f} us below the staged one, the spreads are '
          f'{f[2] - f[1]:.2f} (fused) and {s[2] - s[1]:.2f} us (staged)', file=out)
    if depth == 1:
        v = res['vq lookup forward (fill + 1 kernel)']
        print(f'  depth 1: fused / vqk_vq_forward_f32 = {f[0] / v[0]:.3f}', file=out)
    return res


def train_step(out, steps, rounds):
    train = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    images = torch.rand(32, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(DEV)
    runs = {}
    for name in ('standard', 'residual'):
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rvq_bench.txt'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-train-step', action='store_true')
    args = ap.parse_args()
    with open(args.out, 'w') as out:
        print(f'tools/rvq_bench.py on {torch.cuda.get_device_name(0)}: medians of device-event timings, contenders alternating in one '
              'process.', file=out)
        for depth in (1, 2, 4, 8):
            kernels(out, 8192, 1024, 256, depth, args.iters, args.rounds)
            out.flush()
        if not args.no_train_step:
            train_step(out, args.steps, args.rounds)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
