"""IBQ timings on one GPU, device events after warm-up, the contenders alternating in one process:
(a) the fused forward (csrc/ibq.hip: vqk_ibq_forward_f32, training mode: lse, ebar, tokens, bf16 q, sse, hist) against ops.ibq_staged,
    and the argmax-only call (ops.ibq_assign),
(b) the fused backward (vqk_ibq_backward_f32: row pass, code-owning pass, row-owning pass) against ops.ibq_backward_staged,
(c) torch.cuda.max_memory_allocated over one forward + backward of each contender, above what the inputs hold,
(d) the graphed headline train step (batch 32 at 256x256, bf16) of ibq_vqvae.yaml next to standard_vqvae.yaml; with --parent DIR
    (a checkout of the parent commit, built) the standard step of both trees, in child processes that alternate.
N = 8192 rows (32 images x 16x16), (K, D) in {(1024, 256), (4096, 256), (16384, 256), (16384, 64), (65536, 64), (65536, 256)}; a staged contender
that does not fit in memory is reported as such.  The number of calls per timing follows a pilot call (about 20 ms of device time per
timing, 3 to 200 calls).  Writes profiles/ibq_bench.txt (--out)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[sys.argv.index('--root') + 1]) if '--root' in sys.argv else HERE
sys.path.insert(0, ROOT)
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
DEV = 'cuda:0'
SHAPES = ((1024, 256), (4096, 256), (16384, 256), (16384, 64), (65536, 64), (65536, 256))
BETA = 0.25


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3            # us


def alternate(contenders: dict, rounds: int, iters: int | None = None) -> dict:
    """every contender warmed up, then `rounds` passes over all of them in turn; (median us per call, min, max, calls per timing)"""
    calls = {}
    for name, fn in contenders.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = iters or max(3, min(200, int(20000.0 / max(timed(fn, 2), 1.0))))
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, fn in contenders.items():
            times[name].append(timed(fn, calls[name]))
    return {name: (statistics.median(t), min(t), max(t), calls[name]) for name, t in times.items()}


def verdict(out, what, fused, staged):
    gap, spread = staged[0] - fused[0], (fused[2] - fused[1]) + (staged[2] - staged[1])
    met = gap > spread
    print(f'  {what}: staged / fused = {staged[0] / fused[0]:.2f}; the fused median is {gap:.2f} us below the staged one, the two min-max '
          f'spreads add up to {spread:.2f} us: keep criterion {"MET" if met else "NOT MET"}', file=out)
    return met


def peak_above_inputs(fn) -> float:
    """MiB torch.cuda.max_memory_allocated rises above the allocation level at entry over one call"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def kernels(out, n, k, d, rounds):
    ibq = importlib.import_module(PKG + '._ops_ibq')
    g = torch.Generator().manual_seed(1)
    e = (torch.randn(k, d, generator=g) * d ** -0.5).to(DEV).contiguous()
    # trained-like latents: perturbed codes
    z = (e[torch.randint(0, k, (n,), generator=g).to(DEV)] + 0.3 * float(e.std()) * torch.randn(n, d, device=DEV)).contiguous()
    dq = torch.randn(n, d, generator=g).to(DEV).to(torch.bfloat16)
    gs = torch.ones((), device=DEV)
    dz, de = torch.empty(n, d, device=DEV), torch.zeros(k, d, device=DEV)
    cz, ce = BETA * 2.0 / (n * d), 2.0 / (n * d)
    idx, _, _, _, _, lse, ebar = ibq._ibq_forward(z, e, 1.0, True, False, True, True)

    def fused_fwd():
        return ibq._ibq_forward(z, e, 1.0, True, False, True, True)

    def assign():
        ops.ibq_assign(z, e, 1.0)

    def staged_fwd():
        return ops.ibq_staged(z, e, 1.0, want_lo=True)

    def fused_bwd():
        ops.ibq_backward_rows(z, e, idx, lse, ebar, dq, 1.0, cz, ce, gs, dz, de)

    def staged_bwd():
        ops.ibq_backward_staged(z, e, idx, lse, ebar, dq, 1.0, gs * cz, gs * ce)

    def fused_both():
        f = fused_fwd()
        ops.ibq_backward_rows(z, e, f[0], f[5], f[6], dq, 1.0, cz, ce, gs, dz, de)

    def staged_both():
        f = staged_fwd()
        ops.ibq_backward_staged(z, e, f[0], f[5], f[6], dq, 1.0, gs * cz, gs * ce)

    names = ['forward, fused (vqk_ibq_forward_f32)', 'argmax-only call (ops.ibq_assign)', 'backward, fused (vqk_ibq_backward_f32)',
             'forward, staged (ops.ibq_staged)', 'backward, staged (torch operations)']
    contenders = {names[0]: fused_fwd, names[1]: assign, names[2]: fused_bwd}
    staged_fits = True
    try:
        staged_both()
        torch.cuda.synchronize()
        contenders[names[3]], contenders[names[4]] = staged_fwd, staged_bwd
    except torch.OutOfMemoryError:
        staged_fits = False
        torch.cuda.empty_cache()
    res = alternate(contenders, rounds)
    flop_f, flop_b = 4.0 * n * k * d, 14.0 * n * k * d            # 2 products forward; 4 in the code-owning and 3 in the row-owning pass
    print(f'N = {n}, K = {k}, D = {d}' + ('' if staged_fits else '; the staged formulation does NOT fit in memory'), file=out)
    for name, (med, lo, hi, calls) in res.items():
        note = ''
        if name == names[0]:
            note = f'   {flop_f / med * 1e-6:6.1f} TFLOP/s'
        elif name == names[2]:
            note = f'   {flop_b / med * 1e-6:6.1f} TFLOP/s'
        print(f'  {name:44s} {med:10.2f} us   (min {lo:.2f}, max {hi:.2f}; {rounds} rounds x {calls} calls, host-issued launches){note}', file=out)
    mem_f = peak_above_inputs(fused_both)
    print(f'  peak memory above the inputs, forward + backward: fused {mem_f:.1f} MiB', file=out, end='')
    if not staged_fits:
        print('', file=out)
        return None, None
    mem_s = peak_above_inputs(staged_both)
    print(f', staged {mem_s:.1f} MiB: ratio {mem_s / mem_f:.1f}', file=out)
    s_idx = staged_fwd()[0]
    print(f'  tokens equal between the fused and the staged forward: {float((idx == s_idx).double().mean()):.4f}', file=out)
    return verdict(out, 'forward', res[names[0]], res[names[3]]), verdict(out, 'backward', res[names[2]], res[names[4]])


def step_runner(conf_name: str):
    train = importlib.import_module(PKG + '.train')
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    images = torch.rand(32, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(DEV)
    conf = train.get_model_conf(os.path.join(ROOT, 'example_confs', f'{conf_name}_vqvae.yaml'))
    run = train.derive_run_config(conf, 1, {'training.cumulative_bs': 32})
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


def fmt_step(name, med, lo, hi, rounds, steps, note=''):
    return (f'  {name:24s} {med / 1e3:8.3f} ms/step  {32 / med * 1e6:8.1f} images/s   (min {lo / 1e3:.3f}, max {hi / 1e3:.3f} ms; '
            f'{rounds} rounds x {steps} steps){note}')


def train_step(out, steps, rounds):
    res = alternate({f'{name}_vqvae.yaml': step_runner(name) for name in ('standard', 'ibq')}, rounds, steps)
    print('graphed train step, batch 32 at 256x256, bf16 (zero_grad + forward + backward replayed, AdamW launch after it)', file=out)
    for name, (med, lo, hi, _) in res.items():
        print(fmt_step(name, med, lo, hi, rounds, steps), file=out)


def parent_compare(out, parent, steps, rounds):
    """the standard step of this tree and of the parent commit's tree, one child process each, alternating twice"""
    print('standard_vqvae.yaml, this tree against the parent commit built on the same box (child processes in turn, same session)', file=out)
    for turn in range(2):
        for label, root in (('this tree', HERE), ('parent commit', os.path.abspath(parent))):
            cp = subprocess.run([sys.executable, os.path.abspath(__file__), '--root', root, '--step-only', 'standard', '--steps', str(steps),
                                 '--rounds', str(rounds)], capture_output=True, text=True, timeout=400)
            if cp.returncode != 0:
                raise RuntimeError(f'{label}: child failed with {cp.returncode}\n{cp.stderr[-2000:]}')
            med, lo, hi, _ = json.loads(cp.stdout.strip().splitlines()[-1])
            print(fmt_step('standard_vqvae.yaml', med, lo, hi, rounds, steps, f'   <- {label}, turn {turn + 1}'), file=out)
            out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'ibq_bench.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-train-step', action='store_true')
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: its standard step is timed next to this tree\'s')
    ap.add_argument('--root', default=None, help='import the package from this tree (child processes of --parent)')
    ap.add_argument('--step-only', default=None, help='time the graphed step of one config and print [median, min, max, steps] in us')
    args = ap.parse_args()
    if args.step_only:
        res = alternate({'step': step_runner(args.step_only)}, args.rounds, args.steps)['step']
        print(json.dumps(res))
        return
    with open(args.out, 'w') as out:
        print(f'tools/ibq_bench.py on {torch.cuda.get_device_name(0)}: medians of device-event timings, contenders alternating in one '
              'process.', file=out)
        verdicts = {}
        for k, d in SHAPES:
            verdicts[(k, d)] = kernels(out, 8192, k, d, args.rounds)
            out.flush()
        print('keep criterion (fused ahead of staged by more than the two runs\' combined min-max spread; forward / backward): '
              + ', '.join(f'K{k} D{d} ' + ('staged does not fit' if vs[0] is None else ' / '.join('met' if v else 'NOT met' for v in vs))
                          for (k, d), vs in verdicts.items()), file=out)
        if not args.no_train_step:
            train_step(out, args.steps, args.rounds)
            out.flush()
        if args.parent:
            parent_compare(out, args.parent, args.steps, args.rounds)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
