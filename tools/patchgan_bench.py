"""PatchGAN discriminator timings on one GPU: device events after warm-up, medians with min..max over rounds, a device synchronise
closing every window, contenders alternating in one process.
(a) per layer of the 256x256 network (ndf 64, n_layers 3) at B = 16 and 32, bf16 and fp32: forward, data gradient and weight gradient
    of the 4x4 conv (csrc/patchgan.hip) in us and TFLOP/s, next to the yardstick -- vqk_conv2d_general (the im2col kernel the
    StyleGAN2 discriminator's odd shapes run on) on the 3x3 stride-2 conv of the same tensors -- and the BatchNorm passes in GB/s,
(b) the whole discriminator, forward + backward with parameter gradients,
(c) the graphed VQ-GAN step of gumbel_vqgan.yaml (batch 16 at 256x256, bf16, adversary on from step 0) with `type: patchgan` next to
    the same step with the StyleGAN2 discriminator (R1 every 16 steps, as that config has it).
Writes profiles/patchgan_bench.txt (--out)."""
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
pg = importlib.import_module(PKG + '.modules.loss.patchgan')
DEV = 'cuda:0'
CL = torch.channels_last
# (input side, Cin, Cout, stride, BatchNorm behind it) of the 256x256 network
LAYERS = [(256, 3, 64, 2, False), (128, 64, 128, 2, True), (64, 128, 256, 2, True), (32, 256, 512, 1, True), (31, 512, 1, 1, False)]


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


def layer(out, spec, batch, dtype, iters, rounds):
    side, cin, cout, stride, bn = spec
    g = torch.Generator().manual_seed(1)
    e = ops.epc(dtype)
    cin_ld, co_ld = -(-cin // e) * e, -(-cout // e) * e
    x = torch.zeros(batch, cin_ld, side, side)
    x[:, :cin] = torch.randn(batch, cin, side, side, generator=g)
    x = x.to(DEV).to(dtype).contiguous(memory_format=CL)
    w = (torch.randn(cout, cin, 4, 4, generator=g) * 0.02).to(DEV).contiguous(memory_format=CL)
    wmem = w.permute(0, 2, 3, 1)
    so = ops.conv4x4_out(side, stride)
    dy = torch.zeros(batch, co_ld, so, so)
    dy[:, :cout] = torch.randn(batch, cout, so, so, generator=g)
    dy = dy.to(DEV).to(dtype).contiguous(memory_format=CL)
    dw = torch.zeros(cout, 4, 4, cin, device=DEV)
    w3 = (torch.randn(cout, cin, 3, 3, generator=g) * 0.02).to(DEV).contiguous(memory_format=CL)
    contenders = {
        'fprop': lambda: ops.raw_conv4x4_fprop(x, wmem, None, stride, True),
        'dgrad': lambda: ops.raw_conv4x4_dgrad(dy, wmem, side, side, cin_ld, stride),
        'wgrad': lambda: ops.raw_conv4x4_wgrad(x, dy, dw, cout, cin, stride, 1.0, True),
        'yardstick: conv2d_general 3x3 s2': lambda: ops.conv_act(x, w3, None, k=3, stride=2, pad=1, act='lrelu'),
    }
    note = ''
    with torch.no_grad():
        try:
            contenders['yardstick: conv2d_general 3x3 s2']()
        except RuntimeError as err:                     # a shape the existing kernel does not serve: said, not timed
            del contenders['yardstick: conv2d_general 3x3 s2']
            note = f'  yardstick not served here: {err}'
        res = alternate(contenders, iters, rounds)
    flops = 2.0 * batch * so * so * cout * cin * 16
    s3 = (side + 2 - 3) // 2 + 1
    flops3 = 2.0 * batch * s3 * s3 * cout * cin * 9
    tag = 'fp32' if dtype == torch.float32 else 'bf16'
    plan = ops.conv4x4_wgrad_plan(batch, side, side, cin_ld, cin, cout, stride)
    print(f'B = {batch}, {side}x{side} -> {so}x{so}, {cin} -> {cout}, stride {stride}, {tag}  ({flops / 1e9:.2f} GFLOP per pass, wgrad in {plan} '
          f'partials)', file=out)
    for name, (med, lo, hi) in res.items():
        f = flops3 if name.startswith('yardstick') else flops
        print(f'  {name:34s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})  {f / med / 1e6:7.1f} TFLOP/s', file=out)
    if note:
        print(note, file=out)
    if bn:
        y = torch.randn(batch, cout, so, so, generator=g).to(DEV).to(dtype).contiguous(memory_format=CL)
        gamma, beta = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
        rm, rv, nbt = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
        leaf = y.clone().requires_grad_(True)
        z = ops.batch_norm_lrelu(leaf, gamma, beta, rm, rv, nbt)

        def fwd():
            with torch.no_grad():
                ops.batch_norm_lrelu(y, gamma, beta, rm, rv, nbt)
        r2 = alternate({'BatchNorm + LeakyReLU forward': fwd,
                        'BatchNorm + LeakyReLU backward': lambda: torch.autograd.grad(z, leaf, dy, retain_graph=True)}, iters, rounds)
        nbytes = y.numel() * y.element_size()
        for name, (med, lo, hi) in r2.items():
            moved = nbytes * (3 if 'forward' in name else 5)      # forward: read x twice, write y; backward: read x, dy twice, write dx
            print(f'  {name:34s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})  {moved / med / 1e3:7.1f} GB/s', file=out)


def whole(out, batch, dtype, iters, rounds):
    torch.manual_seed(0)
    d = pg.NLayerDiscriminator(3, 64, 3).to(DEV).train()
    d.compute_dtype = dtype
    img = torch.randn(batch, 3, 256, 256, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
    params = list(d.parameters())

    def fwd_bwd():
        logits = d(img)
        torch.autograd.grad(logits.sum(), [img] + params)

    def fwd():
        with torch.no_grad():
            d(img)
    res = alternate({'forward': fwd, 'forward + backward': fwd_bwd}, iters, rounds)
    tag = 'fp32' if dtype == torch.float32 else 'bf16'
    gflop = sum(2.0 * ops.conv4x4_out(s, st) ** 2 * co * ci * 16 for s, ci, co, st, _ in LAYERS) / 1e9
    for name, (med, lo, hi) in res.items():
        mult = 1.0 if name == 'forward' else 3.0
        print(f'whole discriminator, B = {batch}, 256x256, {tag}: {name:20s} {med / 1e3:8.3f} ms  (min {lo / 1e3:.3f}, max {hi / 1e3:.3f})  '
              f'{gflop * batch * mult / med * 1e3:6.1f} TFLOP/s of {gflop * mult:.1f} GFLOP per image', file=out)


def step_runner(overrides: dict):
    train = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    images = torch.rand(16, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(DEV)
    conf = train.get_model_conf(os.path.join(HERE, 'example_confs', 'gumbel_vqgan.yaml'))
    run = train.derive_run_config(conf, 1, dict({'training.cumulative_bs': 16, 'loss.adversarial_params.start_epoch': 0}, **overrides))
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
    res = alternate({'StyleGAN2 discriminator (R1 every 16)': step_runner({}),
                     'type: patchgan (ndf 64, n_layers 3)': step_runner({'loss.adversarial_params.discriminator': dict(type='patchgan', ndf=64, n_layers=3),
                                                                         'loss.adversarial_params.r1_reg_weight': None})}, steps, rounds)
    print('graphed VQ-GAN step of gumbel_vqgan.yaml, batch 16 at 256x256, bf16, adversary on (three graph replays + two AdamW launches per '
          'step)', file=out)
    for name, (med, lo, hi) in res.items():
        print(f'  {name:40s} {med / 1e3:8.3f} ms/step  {16 / med * 1e6:8.1f} images/s   (min {lo / 1e3:.3f}, max {hi / 1e3:.3f} ms; '
              f'{rounds} rounds x {steps} steps)', file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'patchgan_bench.txt'))
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--no-train-step', action='store_true')
    args = ap.parse_args()
    with open(args.out, 'w') as out:
        arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
        print(f'tools/patchgan_bench.py on {torch.cuda.get_device_name(0)} ({arch}): medians of device-event timings over {args.rounds} rounds x '
              f'{args.iters} calls, contenders alternating in one process, random operands.  TFLOP/s: 2 B Ho Wo Cout Cin 16 per conv pass '
              '(9 taps for the 3x3 yardstick); GB/s: the bytes a pass has to move.', file=out)
        for batch in (16, 32):
            for dtype in (torch.bfloat16, torch.float32):
                for spec in LAYERS:
                    layer(out, spec, batch, dtype, args.iters, args.rounds)
                    out.flush()
                whole(out, batch, dtype, args.iters, args.rounds)
                out.flush()
        if not args.no_train_step:
            train_step(out, args.steps, args.rounds)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
