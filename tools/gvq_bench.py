"""Grouped-quantizer timings on one GPU, device events after warm-up, the contenders alternating in one process:
(a) the fused forward (csrc/gvq.hip: fill + vqk_row_sqnorm_f32 over the codebook + one kernel) against the staged formulation
    (ops.gvq_staged: per group a slice copy, two row_sqnorm launches, vqk_vq_assign_f32, vqk_vq_gather_f32 and two slot copies) --
    the only way the standard quantizer's kernels express this quantizer -- and the |e|^2 launch alone,
(b) the fused backward (default and deterministic form) against the staged path's autograd backward (the closed forms as torch
    operations: ops.GVQLookupFn with ops.GVQ_FUSED off),
(c) the graphed headline train step (batch 32 at 256x256, bf16) of grouped_vqvae.yaml next to standard_vqvae.yaml; with --parent DIR
    (a checkout of the parent commit, built) the standard step of both trees, in child processes that alternate.
N = 8192 rows (32 images x 16x16), (K, d, G) in {(1024, 32, 2), (4096, 8, 8), (1024, 64, 4)}.  Writes profiles/gvq_bench.txt (--out)."""
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
SHAPES = ((1024, 32, 2), (4096, 8, 8), (1024, 64, 4))


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


def kernels(out, n, k, d, groups, iters, rounds):
    native = importlib.import_module(PKG + '._native')
    lib, st = native.lib(), ops._stream()
    g = torch.Generator().manual_seed(1)
    dm = groups * d
    # trained-like codebooks: the codes of group g = perturbed slices of the latents (as tools/cos_bench.py sizes the lookup)
    z = (torch.randn(n, dm, generator=g) * 0.36).to(DEV).contiguous()
    pick = torch.randint(0, n, (groups, k), generator=g).to(DEV)
    e = torch.stack([z[pick[j], j * d:(j + 1) * d] for j in range(groups)]).reshape(groups * k, d)
    e = torch.nn.Parameter((e + 0.01 * torch.randn(groups * k, d, device=DEV)).contiguous())
    dq = torch.randn(n, dm, generator=g).to(DEV).to(torch.bfloat16)
    idx = torch.empty(n, groups, dtype=torch.int64, device=DEV)
    q = torch.empty(n, dm, dtype=torch.bfloat16, device=DEV)
    e2 = torch.empty(groups * k, dtype=torch.float32, device=DEV)
    zbuf = torch.zeros(groups * k + 1, dtype=torch.int32, device=DEV)
    dz, de, gs = torch.empty(n, dm, device=DEV), torch.empty(groups * k, d, device=DEV), torch.ones((), device=DEV)
    ws = torch.empty(lib.vqk_gvq_backward_ws_bytes(n, d, groups), dtype=torch.uint8, device=DEV)
    cz, ce = 0.25 * 2.0 / (n * dm), 2.0 / (n * dm)

    def e2_only():
        native.check(lib.vqk_row_sqnorm_f32(e.data_ptr(), groups * k, d, e2.data_ptr(), st), 'row_sqnorm(e)')

    def fused_fwd():
        zbuf.zero_()
        e2_only()
        native.check(lib.vqk_gvq_forward_f32(z.data_ptr(), e.data_ptr(), e2.data_ptr(), n, k, d, groups, idx.data_ptr(), 0, q.data_ptr(),
                                             zbuf[groups * k:].data_ptr(), zbuf.data_ptr(), st), 'gvq_forward')

    def staged_fwd():
        ops.gvq_staged(z, e, groups, want_lo=True)

    def fused_bwd():
        de.zero_()
        native.check(lib.vqk_gvq_backward_f32(z.data_ptr(), e.data_ptr(), idx.data_ptr(), dq.data_ptr(), 1, n, k, d, groups, cz, ce,
                                              gs.data_ptr(), dz.data_ptr(), de.data_ptr(), ws.data_ptr(), ws.numel(), st), 'gvq_backward')

    def fused_bwd_det():
        native.check(lib.vqk_set_deterministic(1, 0, 0), 'set_deterministic')
        try:
            fused_bwd()
        finally:
            native.check(lib.vqk_set_deterministic(0, 0, 0), 'set_deterministic')

    img = lambda t: t.view(1, n, 1, dm).permute(0, 3, 1, 2)
    zg = z.clone().requires_grad_(True)
    saved = ops.GVQ_FUSED
    ops.GVQ_FUSED = False
    try:
        qs, _, ls, _ = ops.GVQLookupFn.apply(img(zg), e, 0.25, groups, torch.bfloat16)
    finally:
        ops.GVQ_FUSED = saved

    def staged_bwd():
        torch.autograd.grad([qs, ls], [zg, e], [img(dq), gs], retain_graph=True)

    fused_fwd()
    s_idx = ops.gvq_staged(z, e, groups)[0]
    agree = bool(torch.equal(idx, s_idx))
    used = int((zbuf[:groups * k] > 0).sum())
    names = ('gvq fused forward (fill + |e|^2 + 1 kernel)', f'gvq staged forward (ops.gvq_staged, {groups} groups)', '|e|^2 launch alone (vqk_row_sqnorm_f32)',
             'gvq fused backward, default (fill + 1 kernel)', 'gvq fused backward, deterministic (fill + 2)',
             'staged autograd backward (torch operations)')
    res = alternate(dict(zip(names, (fused_fwd, staged_fwd, e2_only, fused_bwd, fused_bwd_det, staged_bwd))), iters, rounds)
    print(f'N = {n}, K = {k}, d = {d}, G = {groups} (D = {dm}); fused tokens equal to the staged formulation: {agree}; codes in use '
          f'{used} of {groups * k}', file=out)
    for name, (med, lo, hi) in res.items():
        print(f'  {name:50s} {med:9.2f} us   (min {lo:.2f}, max {hi:.2f}; {rounds} rounds x {iters} calls, host-issued launches)', file=out)
    f, s = res[names[0]], res[names[1]]
    gap, spread = s[0] - f[0], (f[2] - f[1]) + (s[2] - s[1])
    print(f'  forward: staged / fused = {s[0] / f[0]:.2f}; the fused median is {gap:.2f} us below the staged one, the two min-max spreads '
          f'add up to {spread:.2f} us: keep criterion {"MET" if gap > spread else "NOT MET"}', file=out)
    b, t = res[names[3]], res[names[5]]
    gap_b, spread_b = t[0] - b[0], (b[2] - b[1]) + (t[2] - t[1])
    print(f'  backward: staged autograd / fused default = {t[0] / b[0]:.2f} ({gap_b:.2f} us against a combined spread of {spread_b:.2f} us: '
          f'keep criterion {"MET" if gap_b > spread_b else "NOT MET"}); deterministic / default = {res[names[4]][0] / b[0]:.2f}', file=out)
    return gap > spread and gap_b > spread_b


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
    res = alternate({f'{name}_vqvae.yaml': step_runner(name) for name in ('standard', 'grouped')}, steps, rounds)
    print('graphed train step, batch 32 at 256x256, bf16 (zero_grad + forward + backward replayed, AdamW launch after it)', file=out)
    for name, (med, lo, hi) in res.items():
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
            med, lo, hi = json.loads(cp.stdout.strip().splitlines()[-1])
            print(fmt_step('standard_vqvae.yaml', med, lo, hi, rounds, steps, f'   <- {label}, turn {turn + 1}'), file=out)
            out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'gvq_bench.txt'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-train-step', action='store_true')
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: its standard step is timed next to this tree\'s')
    ap.add_argument('--root', default=None, help='import the package from this tree (child processes of --parent)')
    ap.add_argument('--step-only', default=None, help='time the graphed step of one config and print [median, min, max] in us')
    args = ap.parse_args()
    if args.step_only:
        res = alternate({'step': step_runner(args.step_only)}, args.steps, args.rounds)['step']
        print(json.dumps(res))
        return
    with open(args.out, 'w') as out:
        print(f'tools/gvq_bench.py on {torch.cuda.get_device_name(0)}: medians of device-event timings, contenders alternating in one '
              'process.', file=out)
        verdicts = {}
        for k, d, groups in SHAPES:
            verdicts[(k, d, groups)] = kernels(out, 8192, k, d, groups, args.iters, args.rounds)
            out.flush()
        print('keep criterion (fused ahead of staged by more than the two runs\' combined min-max spread, forward and backward): '
              + ', '.join(f'K{k} d{d} G{g} {"met" if v else "NOT met"}' for (k, d, g), v in verdicts.items()), file=out)
        if not args.no_train_step:
            train_step(out, args.steps, args.rounds)
            out.flush()
        if args.parent:
            parent_compare(out, args.parent, args.steps, args.rounds)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
