"""Self-attention timings on one GPU, device events after warm-up, the contenders alternating in one process:
(a) the fused forward (csrc/attn.hip: one kernel) against the staged formulation (ops.attention_staged: torch matmul / softmax with
    fp32 logits, the B x heads x N x N matrix materialised), fp32 and bf16 storage,
(b) the fused backward (delta + dK/dV pass + dQ pass) against the staged path's autograd backward,
(c) the graphed headline train step (batch 32 at 256x256, bf16) of standard_vqvae.yaml with and without attn_resolutions: [16].
Shapes (B, N, heads, d): (32, 256, 1, 512) -- the canonical single-head block at 16x16 --, (32, 1024, 1, 256), (32, 256, 8, 64).
Writes profiles/attn_bench.txt (--out)."""
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
SHAPES = [(32, 256, 1, 512), (32, 1024, 1, 256), (32, 256, 8, 64)]


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
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, fn in contenders.items():
            times[name].append(timed(fn, iters))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def kernels(out, shape, dtype, iters, rounds):
    b, n, heads, d = shape
    g = torch.Generator().manual_seed(1)
    q, k, v, do = (torch.randn(b, n, heads * d, generator=g).to(DEV).to(dtype) for _ in range(4))
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o_f = ops.attention(*leaves, heads)
    o_s = ops.attention_staged(*leaves, heads)
    diff = float((o_f.detach().float() - o_s.detach().float()).abs().max())

    def fwd(fn):
        def call():
            with torch.no_grad():
                fn(q, k, v, heads)
        return call

    def bwd(o):
        return lambda: torch.autograd.grad(o, leaves, do, retain_graph=True)

    names = ('fused forward (1 kernel)', 'staged forward (torch)', 'fused backward (3 kernels)', 'staged backward (autograd)')
    res = alternate(dict(zip(names, (fwd(ops.attention), fwd(ops.attention_staged), bwd(o_f), bwd(o_s)))), iters, rounds)
    flops = 4.0 * b * heads * n * n * d
    tag = 'fp32' if dtype == torch.float32 else 'bf16'
    print(f'B = {b}, N = {n}, heads = {heads}, d = {d}, {tag}; max|fused - staged| of o = {diff:.2e}', file=out)
    for i, (name, (med, lo, hi)) in enumerate(res.items()):
        tf = flops * (1.0 if i < 2 else 2.5) / med / 1e6
        print(f'  {name:30s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f}; {rounds} rounds x {iters} calls)  {tf:7.1f} TFLOP/s', file=out)
    print(f'  staged / fused: forward {res[names[1]][0] / res[names[0]][0]:.2f}, backward {res[names[3]][0] / res[names[2]][0]:.2f}', file=out)


def step_runner(overrides: dict):
    train = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    images = torch.rand(32, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(DEV)
    conf = train.get_model_conf(os.path.join(HERE, 'example_confs', 'standard_vqvae.yaml'))
    run = train.derive_run_config(conf, 1, dict({'training.cumulative_bs': 32}, **overrides))
    torch.manual_seed(0)
    m = model_mod.VQVAE(run['image_size'], run['ae_conf'], run['q_conf'], run['l_conf'], run['t_conf'],
                        compute_dtype=torch.bfloat16).to(DEV).train()
    tr = trainer_mod.MiniTrainer(num_training_batches=1000)
    tr.attach(m)
    m.on_train_start()
    tr.capture(m, images, warmup=3)
    counter = [3]

    def step():
        tr.train_batch_graphed(m, images, counter[0])
        counter[0] += 1
    return step


def train_step(out, steps, rounds):
    res = alternate({'standard_vqvae.yaml': step_runner({}),
                     '+ attn_resolutions: [16]': step_runner({'autoencoder.attn_resolutions': [16]})}, steps, rounds)
    print('graphed train step, batch 32 at 256x256, bf16 (zero_grad + forward + backward replayed, AdamW launch after it); [16] adds six '
          'blocks: d = 512 x 4, d = 256 x 2, N = 256', file=out)
    for name, (med, lo, hi) in res.items():
        print(f'  {name:26s} {med / 1e3:8.3f} ms/step  {32 / med * 1e6:8.1f} images/s   (min {lo / 1e3:.3f}, max {hi / 1e3:.3f} ms; '
              f'{rounds} rounds x {steps} steps)', file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'attn_bench.txt'))
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-train-step', action='store_true')
    args = ap.parse_args()
    with open(args.out, 'w') as out:
        arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
        print(f'tools/attn_bench.py on {torch.cuda.get_device_name(0)} ({arch}): medians of device-event timings, contenders alternating in one '
              'process.  TFLOP/s: 4 B heads N^2 d per forward, 2.5 times that per backward.', file=out)
        for shape in SHAPES:
            for dtype in (torch.float32, torch.bfloat16):
                kernels(out, shape, dtype, args.iters, args.rounds)
                out.flush()
        if not args.no_train_step:
            train_step(out, args.steps, args.rounds)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
