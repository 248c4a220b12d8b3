"""Spatially conditioned GroupNorm timings on one GPU at the decoder's shapes (batch 32, 256x256 images, channels 128, multipliers
[1, 2, 2, 4]: r from 1 at the 16x16 latents to 16 at the head), fp32 and bf16 storage, device events after warm-up, the contenders
alternating in one process:
(a) the fused forward / backward (csrc/spnorm.hip: statistics + apply; two sweeps + two small finishing launches),
(b) the staged torch formulation of the same function (ops.spatial_norm_staged, its backward by autograd),
(c) the plain GroupNorm + SiLU forward / backward of csrc/norm.hip at the same shape -- the yardstick for how close to the HBM rate
    the new passes run (the spatial backward moves one more pass's worth of reads).
GB/s: the passes over the map a kernel set makes (forward 3: f twice, out once; spatial backward 5: f and dy twice, df once; GroupNorm
backward 5 in its two-kernel form) times the map's bytes over the time -- the small tables are left out.
(d) the graphed headline train step (batch 32 at 256x256, bf16) of standard_vqvae.yaml with decoder_norm group and spatial.
Writes profiles/spnorm_bench.txt (--out)."""
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
CL = torch.channels_last
# (C, map side, r) of the decoder norms of the 256x256 configs, latents 16x16
SHAPES = [(512, 16, 1), (256, 32, 2), (256, 64, 4), (128, 64, 4), (128, 128, 8), (128, 256, 16)]


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
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, fn in contenders.items():
            times[name].append(timed(fn, iters))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def shape_run(out, batch, c, side, r, dtype, iters, rounds):
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)      # noqa: E731
    lat = side // r
    f = (rnd(batch, c, side, side) + 0.5).to(dtype).contiguous(memory_format=CL)
    dy = rnd(batch, c, side, side).to(dtype).contiguous(memory_format=CL)
    m = (1 + 0.5 * rnd(batch, c, lat, lat)).contiguous(memory_format=CL)
    a = (0.5 * rnd(batch, c, lat, lat)).contiguous(memory_format=CL)
    gamma, beta = 1 + 0.2 * rnd(c), 0.2 * rnd(c)
    dgam, dbet = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    assert ops.spnorm_fused_serves(f, m)
    y_f, stats = ops.raw_spnorm_forward(f, m, a, gamma, beta, 1e-6, True)
    leaves = [t.clone().requires_grad_(True) for t in (f, m, a, gamma, beta)]
    y_s = ops.spatial_norm_staged(*leaves, 32, 1e-6, True)
    diff = float((y_f.float() - y_s.detach().float()).abs().max())
    _, gstats = ops.raw_gn_forward(f, gamma, beta, 32, 1e-6, True)

    def staged_fwd():
        with torch.no_grad():
            ops.spatial_norm_staged(f, m, a, gamma, beta, 32, 1e-6, True)

    contenders = {
        'fused forward (3 launches)': lambda: ops.raw_spnorm_forward(f, m, a, gamma, beta, 1e-6, True),
        'staged forward (torch)': staged_fwd,
        'GroupNorm forward (norm.hip)': lambda: ops.raw_gn_forward(f, gamma, beta, 32, 1e-6, True),
        'fused backward (4 launches)': lambda: ops.raw_spnorm_backward(f, stats, m, a, gamma, beta, dy, True, dgam, dbet),
        'staged backward (autograd)': lambda: torch.autograd.grad(y_s, leaves, dy, retain_graph=True),
        'GroupNorm backward (norm.hip)': lambda: ops.raw_gn_backward(f, gstats, gamma, beta, dy, 32, True, dgam, dbet),
    }
    res = alternate(contenders, iters, rounds)
    nb = f.numel() * f.element_size()
    gn_bwd_passes = 3 if side * side <= 1024 else 5
    passes = {'fused forward (3 launches)': 3, 'GroupNorm forward (norm.hip)': 2 if side * side <= 1024 else 3,
              'fused backward (4 launches)': 5, 'GroupNorm backward (norm.hip)': gn_bwd_passes}
    tag = 'fp32' if dtype == torch.float32 else 'bf16'
    print(f'N = {batch}, C = {c}, map {side}x{side}, r = {r}, {tag} ({nb / 2 ** 20:.0f} MiB per map); max|fused - staged| of out = {diff:.2e}', file=out)
    for name, (med, lo, hi) in res.items():
        rate = f'{passes[name] * nb / med / 1e3:8.0f} GB/s ({passes[name]} passes)' if name in passes else ''
        print(f'  {name:30s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f}; {rounds} rounds x {iters} calls) {rate}', file=out)
    n = list(res)
    print(f'  staged / fused: forward {res[n[1]][0] / res[n[0]][0]:.2f}, backward {res[n[4]][0] / res[n[3]][0]:.2f};  '
          f'fused / GroupNorm: forward {res[n[0]][0] / res[n[2]][0]:.2f}, backward {res[n[3]][0] / res[n[5]][0]:.2f}', file=out)


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
                     '+ decoder_norm: spatial': step_runner({'autoencoder.decoder_norm': 'spatial'})}, steps, rounds)
    print('graphed train step, batch 32 at 256x256, bf16 (zero_grad + forward + backward replayed, AdamW launch after it); spatial: the '
          "decoder's 21 norms on the spatial kernels, its ResBlocks composed from conv2d nodes instead of the fused res_block node", file=out)
    for name, (med, lo, hi) in res.items():
        print(f'  {name:26s} {med / 1e3:8.3f} ms/step  {32 / med * 1e6:8.1f} images/s   (min {lo / 1e3:.3f}, max {hi / 1e3:.3f} ms; '
              f'{rounds} rounds x {steps} steps)', file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'spnorm_bench.txt'))
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-kernels', action='store_true')
    ap.add_argument('--no-train-step', action='store_true')
    args = ap.parse_args()
    with open(args.out, 'w') as out:
        arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
        print(f'tools/spnorm_bench.py on {torch.cuda.get_device_name(0)} ({arch}): medians of device-event timings, contenders alternating in '
              'one process; SiLU fused behind every norm.', file=out)
        for c, side, r in ([] if args.no_kernels else SHAPES):
            for dtype in (torch.float32, torch.bfloat16):
                shape_run(out, args.batch, c, side, r, dtype, args.iters, args.rounds)
                out.flush()
                torch.cuda.empty_cache()
        if not args.no_train_step:
            train_step(out, args.steps, args.rounds)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
