"""Lookup-free-quantizer timings on one GPU: device events, the median of 30 samples after 5 warm-up samples (a sample = 20 calls
back to back), the contenders alternating in one process:
(a) the fused forward (kernel + ordered finish, after the histogram fill) and backward (kernel + ordered slab sum) of csrc/lfq.hip at
    N = 8192 rows (32 images x 16x16), D = 256, for bits 10 / group 10 and bits 18 / group 9, bf16 q and dq,
(b) next to the FSQ kernels (csrc/fsq.hip) on the same rows with levels [8,5,5,5],
(c) next to the floor bytes moved / streaming-copy rate, the copy rate measured in the same run (a 256 MiB device copy),
(d) the replayed train step of the small model (32x32, channels 32, one ResBlock, multipliers (1, 2), D = 64, batch 4, fp32) with
    `fsq` ([8,5,5,5]) and with `lfq` (bits 10).
Writes profiles/lfq_bench.txt (--out)."""
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
native = importlib.import_module(PKG + '._native')
DEV = 'cuda:0'
SAMPLES, WARMUP, CALLS = 30, 5, 20


def sample(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3            # us per call


def alternate(contenders: dict, calls: int = CALLS) -> dict:
    """WARMUP + SAMPLES passes over all contenders in turn; median us per call and the spread of the kept samples"""
    times = {name: [] for name in contenders}
    for i in range(WARMUP + SAMPLES):
        for name, fn in contenders.items():
            t = sample(fn, calls)
            if i >= WARMUP:
                times[name].append(t)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def copy_rate():
    """bytes per second of a streaming device copy (read + write counted)"""
    src = torch.empty(256 << 20, dtype=torch.uint8, device=DEV).random_(0, 255)
    dst = torch.empty_like(src)
    med = alternate({'copy': lambda: dst.copy_(src)}, calls=5)['copy'][0]
    return 2 * src.numel() / (med * 1e-6)


def projections(g, d, dm):
    w_in = ((torch.rand(d, dm, generator=g) * 2 - 1) * 2 / dm ** 0.5).to(DEV)
    b_in = (torch.rand(d, generator=g) - 0.5).to(DEV)
    w_out = (torch.rand(dm, d, generator=g) * 2 - 1).to(DEV)
    b_out = (torch.rand(dm, generator=g) - 0.5).to(DEV)
    return w_in, b_in, w_out, b_out


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
        u = torch.empty(n, bits, device=DEV)
        hist = torch.zeros(1 << bits, dtype=torch.int32, device=DEV)
        res = torch.empty(4, device=DEV)
        ltab = torch.empty(((bits + grp - 1) // grp) << grp, device=DEV)
        ws = torch.empty(lib.vqk_lfq_ws_bytes(n, dm, bits, grp), dtype=torch.uint8, device=DEV)
        grads = [torch.empty_like(p) for p in (w_in, b_in, w_out, b_out)]

        def fwd(bits=bits, grp=grp, w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out, u=u, hist=hist, res=res, ltab=ltab, ws=ws):
            hist.zero_()
            native.check(lib.vqk_lfq_forward(z.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), n, dm,
                                             bits, grp, 0.01, 0.25, 0.1, 1.0, idx.data_ptr(), u.data_ptr(), 0, q.data_ptr(),
                                             hist.data_ptr(), res.data_ptr(), ltab.data_ptr(), ws.data_ptr(), ws.numel(), st), 'lfq_forward')

        def bwd(bits=bits, grp=grp, w_in=w_in, w_out=w_out, u=u, ltab=ltab, ws=ws, grads=grads):
            native.check(lib.vqk_lfq_backward(z.data_ptr(), u.data_ptr(), dq.data_ptr(), 1, w_in.data_ptr(), w_out.data_ptr(),
                                              ltab.data_ptr(), one.data_ptr(), n, dm, bits, grp, 0.01, 0.25, 0.1, 1.0, dz.data_ptr(),
                                              *(t.data_ptr() for t in grads), 0, ws.data_ptr(), ws.numel(), st), 'lfq_backward')

        fwd()
        contenders[f'lfq bits {bits} / g {grp} forward  (fill + kernel + finish)'] = fwd
        contenders[f'lfq bits {bits} / g {grp} backward (kernel + slab sum)'] = bwd
        # z in, bf16 q out, idx + u out, the histogram fill and its updates | z + bf16 dq + u in, dz out
        moved[f'lfq bits {bits} / g {grp} forward  (fill + kernel + finish)'] = n * dm * 4 + n * dm * 2 + n * (8 + 4 * bits) + 4 * (1 << bits)
        moved[f'lfq bits {bits} / g {grp} backward (kernel + slab sum)'] = n * dm * 4 + n * dm * 2 + n * 4 * bits + n * dm * 4

    levels = (8, 5, 5, 5)
    lv, d, k = ops._levels_arg(levels)
    w_in, b_in, w_out, b_out = projections(g, d, dm)
    fu = torch.empty(n, d, device=DEV)
    fhist = torch.zeros(k, dtype=torch.int32, device=DEV)
    fws = torch.empty(lib.vqk_fsq_backward_ws_bytes(n, dm, d), dtype=torch.uint8, device=DEV)
    fgrads = [torch.empty_like(p) for p in (w_in, b_in, w_out, b_out)]

    def fsq_fwd():
        fhist.zero_()
        native.check(lib.vqk_fsq_forward(z.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), n, dm, d, lv,
                                         idx.data_ptr(), fu.data_ptr(), 0, q.data_ptr(), fhist.data_ptr(), st), 'fsq_forward')

    def fsq_bwd():
        native.check(lib.vqk_fsq_backward(z.data_ptr(), fu.data_ptr(), dq.data_ptr(), 1, w_in.data_ptr(), w_out.data_ptr(), n, dm, d, lv,
                                          dz.data_ptr(), *(t.data_ptr() for t in fgrads), 0, fws.data_ptr(), fws.numel(), st), 'fsq_backward')

    fsq_fwd()
    contenders['fsq [8,5,5,5] forward  (fill + kernel)'] = fsq_fwd
    contenders['fsq [8,5,5,5] backward (kernel + slab sum)'] = fsq_bwd
    moved['fsq [8,5,5,5] forward  (fill + kernel)'] = n * dm * 4 + n * dm * 2 + n * (8 + 4 * d) + 4 * k
    moved['fsq [8,5,5,5] backward (kernel + slab sum)'] = n * dm * 4 + n * dm * 2 + n * 4 * d + n * dm * 4

    res = alternate(contenders)
    print(f'N = {n}, D = {dm}, bf16 q and dq, tau = 0.01; streaming copy rate measured in this run: {rate / 1e12:.2f} TB/s', file=out)
    for name, (med, lo, hi) in res.items():
        floor = moved[name] / rate * 1e6
        print(f'  {name:58s} {med:8.2f} us  (min {lo:.2f}, max {hi:.2f})   moves {moved[name] / 1e6:5.1f} MB: floor {floor:5.2f} us, '
              f'{med / floor:5.1f} x the floor', file=out)


def train_step(out):
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    ae = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
    tc = dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
    confs = {'fsq [8,5,5,5]': dict(num_embeddings=1000, embedding_dim=64, reinit_every_n_epochs=None, type='fsq', params=dict(levels=[8, 5, 5, 5])),
             'lfq bits 10': dict(num_embeddings=1024, embedding_dim=64, reinit_every_n_epochs=None, type='lfq', params=dict(bits=10))}
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lfq_bench.txt'))
    ap.add_argument('--no-train-step', action='store_true')
    args = ap.parse_args()
    with open(args.out, 'w') as out:
        print(f'tools/lfq_bench.py on {torch.cuda.get_device_name(0)}: device-event timings, median of {SAMPLES} samples after {WARMUP} '
              f'warm-up samples ({CALLS} host-issued calls per sample), contenders alternating in one process.', file=out)
        kernels(out, 8192, 256, copy_rate())
        out.flush()
        if not args.no_train_step:
            train_step(out)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
