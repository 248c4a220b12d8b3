"""Binary-spherical-quantizer timings on one GPU, in the manner of tools/lfq_bench.py: device events, the median of 30 samples after 5
warm-up samples (a sample = 20 calls back to back), the contenders alternating in one process:
(a) the fused forward (kernel + ordered finish, after the histogram fill) and backward (kernel + ordered slab sum) of csrc/bsq.hip at
    N = 8192 rows (32 images x 16x16), D = 256, for bits 10 / group 10 and bits 18 / group 9, bf16 q and dq,
(b) next to the LFQ calls (csrc/lfq.hip) at the same shapes on the same rows -- the yardstick: lfq does strictly less arithmetic per
    row and reduces its projections with one butterfly per channel, bsq with the transposing reduction of csrc/proj_quant.h,
(c) next to the floor bytes moved / streaming-copy rate, the copy rate measured in the same run (a 256 MiB device copy),
(d) the replayed train step of the small model (32x32, channels 32, one ResBlock, multipliers (1, 2), D = 64, batch 4, fp32) with
    `lfq` and with `bsq` (bits 10).
Writes profiles/bsq_bench.txt (--out)."""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
from lfq_bench import CALLS, DEV, SAMPLES, WARMUP, alternate, copy_rate, projections  # noqa: E402  the one sampling scheme

TAU = {'lfq': 0.01, 'bsq': 0.02}            # each quantizer at its shipped temperature


def kernels(out, n, dm, rate):
    g = torch.Generator().manual_seed(1)
    lib, st = native.lib(), ops._stream()
    z = torch.randn(n, dm, generator=g).to(DEV)
    dq = torch.randn(n, dm, generator=g).to(DEV).to(torch.bfloat16)
    idx = torch.empty(n, dtype=torch.int64, device=DEV)
    q = torch.empty(n, dm, dtype=torch.bfloat16, device=DEV)
    dz = torch.empty(n, dm, device=DEV)
    one = torch.ones((), device=DEV)
    contenders, moved = {}, {}

    for bits, grp in ((10, 10), (18, 9)):
        w_in, b_in, w_out, b_out = projections(g, bits, dm)
        for kind in ('lfq', 'bsq'):
            u = torch.empty(n, bits, device=DEV)
            r = torch.empty(n, device=DEV)
            hist = torch.zeros(1 << bits, dtype=torch.int32, device=DEV)
            res = torch.empty(4, device=DEV)
            ltab = torch.empty(((bits + grp - 1) // grp) << grp, device=DEV)
            ws = torch.empty(getattr(lib, f'vqk_{kind}_ws_bytes')(n, dm, bits, grp), dtype=torch.uint8, device=DEV)
            grads = [torch.empty_like(p) for p in (w_in, b_in, w_out, b_out)]
            extra = (r.data_ptr(),) if kind == 'bsq' else ()

            def fwd(kind=kind, bits=bits, grp=grp, w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out, u=u, hist=hist, res=res, ltab=ltab,
                    ws=ws, extra=extra):
                hist.zero_()
                native.check(getattr(lib, f'vqk_{kind}_forward')(z.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(),
                                                                 b_out.data_ptr(), n, dm, bits, grp, TAU[kind], 0.25, 0.1, 1.0,
                                                                 idx.data_ptr(), u.data_ptr(), *extra, 0, q.data_ptr(), hist.data_ptr(),
                                                                 res.data_ptr(), ltab.data_ptr(), ws.data_ptr(), ws.numel(), st),
                             f'{kind}_forward')

            def bwd(kind=kind, bits=bits, grp=grp, w_in=w_in, w_out=w_out, u=u, ltab=ltab, ws=ws, grads=grads, extra=extra):
                native.check(getattr(lib, f'vqk_{kind}_backward')(z.data_ptr(), u.data_ptr(), *extra, dq.data_ptr(), 1, w_in.data_ptr(),
                                                                  w_out.data_ptr(), ltab.data_ptr(), one.data_ptr(), n, dm, bits, grp,
                                                                  TAU[kind], 0.25, 0.1, 1.0, dz.data_ptr(),
                                                                  *(t.data_ptr() for t in grads), 0, ws.data_ptr(), ws.numel(), st),
                             f'{kind}_backward')

            fwd()
            name_f = f'{kind} bits {bits} / g {grp} forward  (fill + kernel + finish)'
            name_b = f'{kind} bits {bits} / g {grp} backward (kernel + slab sum)'
            contenders[name_f], contenders[name_b] = fwd, bwd
            rbytes = 4 * n if kind == 'bsq' else 0
            # z in, bf16 q out, idx + u (+ r) out, the histogram fill and its updates | z + bf16 dq + u (+ r) in, dz out
            moved[name_f] = n * dm * 4 + n * dm * 2 + n * (8 + 4 * bits) + rbytes + 4 * (1 << bits)
            moved[name_b] = n * dm * 4 + n * dm * 2 + n * 4 * bits + rbytes + n * dm * 4

    res = alternate(contenders)
    print(f'N = {n}, D = {dm}, bf16 q and dq, tau = 0.01 (lfq) / 0.02 (bsq); streaming copy rate measured in this run: '
          f'{rate / 1e12:.2f} TB/s', file=out)
    for name, (med, lo, hi) in res.items():
        floor = moved[name] / rate * 1e6
        print(f'  {name:58s} {med:8.2f} us  (min {lo:.2f}, max {hi:.2f})   moves {moved[name] / 1e6:5.1f} MB: floor {floor:5.2f} us, '
              f'{med / floor:5.1f} x the floor', file=out)
    print('bsq over lfq at the same shape (median over median):', file=out)
    for name, (med, _, _) in res.items():
        if name.startswith('bsq'):
            print(f'  {name[4:]:54s} {med / res["lfq" + name[3:]][0]:6.3f}', file=out)


def train_step(out):
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    ae = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
    tc = dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
    confs = {f'{kind} bits 10': dict(num_embeddings=1024, embedding_dim=64, reinit_every_n_epochs=None, type=kind, params=dict(bits=10))
             for kind in ('lfq', 'bsq')}
    images = torch.rand(4, 3, 32, 32, generator=torch.Generator().manual_seed(0)).to(DEV)
    runs = {}
    for name, qc in confs.items():
        torch.manual_seed(0)
        m = model_mod.VQVAE(32, ae, qc, None, tc).to(DEV).train()
        tr = trainer_mod.MiniTrainer(num_training_batches=100000)
        tr.attach(m)
        m.on_train_start()
        tr.capture(m, images, warmup=3)
        counter = [3]

        def step(m=m, tr=tr, counter=counter):
            tr.train_batch_graphed(m, images, counter[0])
            counter[0] += 1
        runs[name] = step
    res = alternate(runs, calls=10)
    print('replayed train step of the small model (32x32, channels 32, one ResBlock, multipliers (1, 2), D = 64, batch 4, fp32)', file=out)
    for name, (med, lo, hi) in res.items():
        print(f'  {name:24s} {med:8.1f} us/step  (min {lo:.1f}, max {hi:.1f})', file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bsq_bench.txt'))
    ap.add_argument('--no-train-step', action='store_true')
    args = ap.parse_args()
    with open(args.out, 'w') as out:
        print(f'tools/bsq_bench.py on {torch.cuda.get_device_name(0)}: device-event timings, median of {SAMPLES} samples after {WARMUP} '
              f'warm-up samples ({CALLS} host-issued calls per sample), contenders alternating in one process.', file=out)
        kernels(out, 8192, 256, copy_rate())
        out.flush()
        if not args.no_train_step:
            train_step(out)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
