"""SimVQ timings on one GPU, device events after warm-up, the contenders alternating in one process:
(a) the projection alone (csrc/simvq.hip: vqk_simvq_project_f32) against torch.addmm, the prepare launch alone (D = 256:
    vqk_vq_prepare_f32 on the fresh E) and the lookup alone on a given E,
(b) the whole forward: E + lookup as ops.SimVQLookupFn's product route issues them (ops.simvq_effective: torch.addmm unless
    ops.SIMVQ_PROJECT is on; D = 256: prepare + the one-kernel lookup) against ops.simvq_staged, and the same with the HIP projection,
(c) the backward pair (vqk_simvq_backward_f32: dz + per-block partials, then the ordered sum into dW / db) against the staged backward
    (ops.simvq_backward_staged: the closed forms as torch operations with the [K, D] scatter target and the D x K x D product),
(d) the graphed headline train step (batch 32 at 256x256, bf16) of simvq_vqvae.yaml next to standard_vqvae.yaml; with --parent DIR
    (a checkout of the parent commit, built) the standard step of both trees, in child processes that alternate.
N = 8192 rows (32 images x 16x16), (K, D) in {(8192, 256), (65536, 256), (65536, 128), (262144, 64)}.  The number of calls per timing
follows a pilot call (about 20 ms of device time per timing, 3 to 200 calls).  Writes profiles/simvq_bench.txt (--out)."""
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
SHAPES = ((8192, 256), (65536, 256), (65536, 128), (262144, 64))


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


def kernels(out, n, k, d, rounds):
    native = importlib.import_module(PKG + '._native')
    sv = importlib.import_module(PKG + '._ops_simvq')
    lib, st = native.lib(), ops._stream()
    g = torch.Generator().manual_seed(1)
    c = (torch.randn(k, d, generator=g) * d ** -0.5).to(DEV).contiguous()
    # a layer some way into training: the identity plus a dense perturbation, a small bias
    w = (torch.eye(d) + 0.1 * d ** -0.5 * torch.randn(d, d, generator=g)).to(DEV).contiguous()
    b = (0.01 * torch.randn(d, generator=g)).to(DEV)
    e = ops.simvq_project(c, w, b)
    # trained-like latents: perturbed effective codes
    z = (e[torch.randint(0, k, (n,), generator=g).to(DEV)] + 0.3 * float(e.std()) * torch.randn(n, d, device=DEV)).contiguous()
    dq = torch.randn(n, d, generator=g).to(DEV).to(torch.bfloat16)
    e_out = torch.empty_like(e)
    gs = torch.ones((), device=DEV)
    dz, dw, db = torch.empty(n, d, device=DEV), torch.zeros(d, d, device=DEV), torch.zeros(d, device=DEV)
    ws = torch.empty(lib.vqk_simvq_backward_ws_bytes(n, d), dtype=torch.uint8, device=DEV)
    cz, ce = 0.25 * 2.0 / (n * d), 2.0 / (n * d)
    idx = sv._simvq_lookup(z, e, False, False, False)[0]

    def project():
        native.check(lib.vqk_simvq_project_f32(c.data_ptr(), w.data_ptr(), b.data_ptr(), k, d, e_out.data_ptr(), st), 'simvq_project')

    def addmm():
        torch.addmm(b, c, w.t(), out=e_out)

    def lookup():
        sv._simvq_lookup(z, e, False, True, True)

    def fused_fwd():
        sv._simvq_lookup(z, ops.simvq_effective(c, w, b), False, True, True)

    def fused_fwd_hip():
        sv._simvq_lookup(z, ops.simvq_project(c, w, b), False, True, True)

    def staged_fwd():
        ops.simvq_staged(z, c, w, b, want_lo=True)

    def fused_bwd():
        native.check(lib.vqk_simvq_backward_f32(z.data_ptr(), e.data_ptr(), c.data_ptr(), idx.data_ptr(), dq.data_ptr(), 1, n, k, d, cz, ce,
                                                gs.data_ptr(), dz.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), st),
                     'simvq_backward')

    def staged_bwd():
        ops.simvq_backward_staged(z, e, c, idx, dq, gs * cz, gs * ce)

    contenders = {'projection, HIP (vqk_simvq_project_f32)': project, 'projection, torch.addmm': addmm,
                  'lookup alone on a given E (bf16 q, sse, hist)': lookup,
                  'whole forward, product route (E + lookup)': fused_fwd, 'whole forward, staged (ops.simvq_staged)': staged_fwd,
                  'backward, HIP pair (vqk_simvq_backward_f32)': fused_bwd, 'backward, staged (torch operations)': staged_bwd}
    if d == 256:
        pws = torch.empty(lib.vqk_vq_filter_ws_bytes(k, d), dtype=torch.uint8, device=DEV)

        def prepare():
            native.check(lib.vqk_vq_prepare_f32(e.data_ptr(), k, d, pws.data_ptr(), pws.numel(), st), 'vq_prepare')
        contenders['prepare launch alone (vqk_vq_prepare_f32)'] = prepare
    contenders['whole forward with the HIP projection'] = fused_fwd_hip
    res = alternate(contenders, rounds)
    s_idx = ops.simvq_staged(z, c, w, b)[1]
    agree = float((idx == s_idx).double().mean())
    flop = 2.0 * k * d * d
    print(f'N = {n}, K = {k}, D = {d}; tokens equal between the fused and the staged forward: {agree:.4f} (two evaluations of E); backward '
          f'grid {lib.vqk_simvq_backward_ws_bytes(n, d) // ((d * d + d) * 4)} blocks', file=out)
    for name, (med, lo, hi, calls) in res.items():
        note = f'   {flop / med * 1e-6:6.1f} TFLOP/s, {2.0 * k * d * 4 / med * 1e-6:5.2f} TB/s' if name.startswith('projection') else ''
        print(f'  {name:50s} {med:10.2f} us   (min {lo:.2f}, max {hi:.2f}; {rounds} rounds x {calls} calls, host-issued launches){note}', file=out)
    names = list(contenders)
    ok_p = verdict(out, 'projection', res[names[0]], res[names[1]])
    ok_f = verdict(out, 'forward', res[names[3]], res[names[4]])
    ok_b = verdict(out, 'backward', res[names[5]], res[names[6]])
    return ok_p, ok_f, ok_b


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
    res = alternate({f'{name}_vqvae.yaml': step_runner(name) for name in ('standard', 'simvq')}, rounds, steps)
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
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'simvq_bench.txt'))
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
        print(f'tools/simvq_bench.py on {torch.cuda.get_device_name(0)}: medians of device-event timings, contenders alternating in one '
              'process.', file=out)
        verdicts = {}
        for k, d in SHAPES:
            verdicts[(k, d)] = kernels(out, 8192, k, d, args.rounds)
            out.flush()
        print('keep criterion (fused ahead of staged by more than the two runs\' combined min-max spread; projection / forward / backward): '
              + ', '.join(f'K{k} D{d} ' + ' / '.join('met' if v else 'NOT met' for v in vs) for (k, d), vs in verdicts.items()), file=out)
        if not args.no_train_step:
            train_step(out, args.steps, args.rounds)
            out.flush()
        if args.parent:
            parent_compare(out, args.parent, args.steps, args.rounds)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
