"""Rotation-trick backward timings on one GPU, device events after warm-up, the contenders alternating in one process:
(a) vqk_vq_backward_rot_f32 (csrc/vq_rot.hip) against the straight-through vqk_vq_backward_fused_f32 (csrc/vq_filter.hip, unchanged
    from the parent commit) on the same inputs -- bf16 and fp32 dq, with the codebook gradient (standard) and without (EMA); the
    straight-through kernel is listed TWICE (A / B): the difference of two runs of the same kernel is the box's spread;
(b) the graphed `standard` train step (bf16) with `quantizer.params.gradient` absent and set to `rotation`, the plain step twice.
Sizes: the headline latent N = 8192 (32 images x 16x16), D = 256, K = 1024, and N = 32768 (128 images), D = 256, K = 8192.
Writes profiles/rot_bench.txt (--out)."""
import argparse
import importlib
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
DEV = 'cuda:0'
SIZES = ((8192, 1024), (32768, 8192))                    # (N, K) at D = 256


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


def kernels(out, n, k, iters, rounds):
    native = importlib.import_module(PKG + '._native')
    lib, st, d = native.lib(), ops._stream(), 256
    g = torch.Generator().manual_seed(1)
    # a trained-like codebook: codes = perturbed latents, every row on its nearest code
    z = (torch.randn(n, d, generator=g) * 0.36).to(DEV).contiguous()
    pick = torch.randint(0, n, (k,), generator=g).to(DEV)
    e = (z[pick] + 0.01 * torch.randn(k, d, device=DEV)).contiguous()
    idx = ops.vq_assign(z, e, 0)
    dq32 = (0.1 * torch.randn(n, d, generator=g)).to(DEV)
    dqlo = dq32.to(torch.bfloat16)
    dz, de, gs = torch.empty(n, d, device=DEV), torch.zeros(k, d, device=DEV), torch.ones((), device=DEV)
    cz, ce = 0.25 * 2.0 / (n * d), 2.0 / (n * d)

    def call(fn, dq, with_de):
        code = ops.dcode(dq.dtype)
        return lambda: native.check(fn(z.data_ptr(), e.data_ptr(), idx.data_ptr(), dq.data_ptr(), code, n, k, d, cz, ce, gs.data_ptr(),
                                       dz.data_ptr(), de.data_ptr() if with_de else 0, st), 'backward')

    print(f'N = {n}, K = {k}, D = {d}; codes in use {int(torch.unique(idx).numel())}', file=out)
    for dq_name, dq in (('bf16', dqlo), ('fp32', dq32)):
        for with_de in (True, False):
            res = alternate({'st A': call(lib.vqk_vq_backward_fused_f32, dq, with_de), 'rot': call(lib.vqk_vq_backward_rot_f32, dq, with_de),
                             'st B': call(lib.vqk_vq_backward_fused_f32, dq, with_de)}, iters, rounds)
            a, r, b = res['st A'], res['rot'], res['st B']
            base = 0.5 * (a[0] + b[0])
            spread = max(a[2], b[2]) / min(a[1], b[1]) - 1.0
            print(f'  dq {dq_name}, {"dz + de (standard)" if with_de else "dz only (EMA)     "}: straight-through fused {a[0]:7.2f} / {b[0]:7.2f} us '
                  f'(A / B medians; min {min(a[1], b[1]):.2f}, max {max(a[2], b[2]):.2f}: spread {100 * spread:.1f} %), rotation {r[0]:7.2f} us '
                  f'(min {r[1]:.2f}, max {r[2]:.2f}); rotation / straight-through = {r[0] / base:.3f}   [{rounds} rounds x {iters} calls]', file=out)
    out.flush()


def step_runner(k: int, batch: int, gradient):
    train = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    images = torch.rand(batch, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(DEV)
    conf = train.get_model_conf(os.path.join(HERE, 'example_confs', 'standard_vqvae.yaml'))
    over = {'training.cumulative_bs': batch, 'quantizer.num_embeddings': k}
    if gradient is not None:
        over['quantizer.params.gradient'] = gradient
    run = train.derive_run_config(conf, 1, over)
    torch.manual_seed(0)
    m = model_mod.VQVAE(run['image_size'], run['ae_conf'], run['q_conf'], run['l_conf'], run['t_conf'],
                        compute_dtype=torch.bfloat16).to(DEV).train()
    assert m.quantizer.rotate == (gradient == 'rotation')
    tr = trainer_mod.MiniTrainer(num_training_batches=1000)
    tr.attach(m)
    m.on_train_start()
    tr.capture(m, images, warmup=3)
    counter = [3]

    def step():
        tr.train_batch_graphed(m, images, counter[0])
        counter[0] += 1
    return step


def train_step(out, n, k, steps, rounds):
    batch = n // 256
    res = alternate({'plain A': step_runner(k, batch, None), 'rotation': step_runner(k, batch, 'rotation'), 'plain B': step_runner(k, batch, None)},
                    steps, rounds)
    print(f'graphed standard train step, batch {batch} at 256x256 (N = {n}), K = {k}, bf16 (zero_grad + forward + backward replayed, AdamW after it)',
          file=out)
    for name, (med, lo, hi) in res.items():
        print(f'  {name:10s} {med / 1e3:8.3f} ms/step  {batch / med * 1e6:8.1f} images/s   (min {lo / 1e3:.3f}, max {hi / 1e3:.3f} ms; '
              f'{rounds} rounds x {steps} steps)', file=out)
    a, r, b = res['plain A'], res['rotation'], res['plain B']
    print(f'  rotation / plain = {r[0] / (0.5 * (a[0] + b[0])):.4f}; plain A / plain B = {a[0] / b[0]:.4f} (the same step twice: the spread)', file=out)
    out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'rot_bench.txt'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-train-step', action='store_true')
    args = ap.parse_args()
    with open(args.out, 'w') as out:
        print(f'tools/rot_bench.py on {torch.cuda.get_device_name(0)}: medians of device-event timings, contenders alternating in one '
              'process; "straight-through fused" is vqk_vq_backward_fused_f32, the kernel of the parent commit.', file=out)
        for n, k in SIZES:
            kernels(out, n, k, args.iters, args.rounds)
        if not args.no_train_step:
            for n, k in SIZES:
                train_step(out, n, k, args.steps, args.rounds)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
