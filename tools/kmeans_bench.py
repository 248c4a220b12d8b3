"""k-means codebook initialisation timings on one GPU: a host clock around work that ends in a device synchronise (the seeding loop is
thousands of launches: its host issue time is part of what a user waits for), after a warm-up run, the contenders alternating in one
process.  Encoder-latent-like rows x [N, 256] fp32, N = 65,536 (256 images x 16x16), K = 1024 and 8192:
(a) the seeding loop ops.kmeans_seed (csrc/kmeans.hip, 2 K - 1 launches, no host read) against a torch formulation of the same rule
    with the pick kept on the device: direct-difference min update + float64 cumsum + searchsorted,
(b) one Lloyd iteration ops.kmeans_lloyd_step (vq_assign + ema_stats + the update kernel) against torch (|x|^2 + |c|^2 - 2 x c^T, argmin,
    index_add_, division),
(c) the whole fit at 10 iterations, ops.kmeans_fit against the torch formulations of (a) and (b),
(d) the seeding step alone (device events over the K - 1 steps of one loop): microseconds per pick, the N x D x 4 bytes of x it reads over
    that time, next to vqk_calib_copy over the same number of bytes on this box (a copy moves twice its size: read + write).
Writes profiles/kmeans_bench.txt (--out)."""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
DEV = 'cuda:0'


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3                     # ms


def alternate(contenders: dict, rounds: int) -> dict:
    for fn in contenders.values():
        fn()                                                    # warm-up: code objects, workspaces, the allocator's blocks
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, fn in contenders.items():
            times[name].append(wall(fn))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def torch_seed(x, k, u):
    """the rule of include/vqk.h in torch operations, no host read: the pick stays a device tensor"""
    n = x.shape[0]
    picks = torch.empty(k, dtype=torch.int64, device=x.device)
    picks[0:1] = torch.floor(u[0:1] * n).clamp(max=n - 1).to(torch.int64)
    mind = torch.full((n,), float('inf'), device=x.device)
    for j in range(1, k):
        c = x.index_select(0, picks[j - 1:j])
        mind = torch.minimum(mind, (x - c).pow(2).sum(1))
        prefix = torch.cumsum(mind.double(), 0)
        picks[j:j + 1] = torch.searchsorted(prefix, u[j:j + 1] * prefix[-1:], right=True).clamp(max=n - 1)
    return picks


def torch_lloyd(x, centres):
    k = centres.shape[0]
    d = (x * x).sum(1, keepdim=True) + (centres * centres).sum(1)[None, :] - 2.0 * (x @ centres.t())
    idx = d.argmin(1)
    counts = torch.bincount(idx, minlength=k).to(torch.float32)
    sums = torch.zeros_like(centres).index_add_(0, idx, x)
    centres.copy_(torch.where(counts[:, None] > 0, sums / counts.clamp(min=1.0)[:, None], centres))
    return counts


def torch_fit(x, k, iters, u):
    centres = x.index_select(0, torch_seed(x, k, u)).contiguous()
    for _ in range(iters):
        torch_lloyd(x, centres)
    return centres


def seed_step_rate(out, x, k, u):
    n, d = x.shape
    lib, st = native.lib(), ops._stream()
    picks = torch.empty(k, dtype=torch.int64, device=DEV)
    mind = torch.empty(n, device=DEV)
    ws = torch.empty(lib.vqk_kmeans_seed_ws_bytes(n), dtype=torch.uint8, device=DEV)

    def loop(first, last):
        for j in range(first, last):
            native.check(lib.vqk_kmeans_seed_step_f32(x.data_ptr(), n, d, k, j, u.data_ptr(), picks.data_ptr(), mind.data_ptr(), 0,
                                                      ws.data_ptr(), ws.numel(), st), 'kmeans_seed_step')
    loop(0, k)
    torch.cuda.synchronize()
    per_pick = []
    for _ in range(3):
        loop(0, 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loop(1, k)
        e1.record()
        torch.cuda.synchronize()
        per_pick.append(e0.elapsed_time(e1) / (k - 1) * 1e3)    # us
    nbytes = n * d * 4
    dst = torch.empty_like(x)
    copies = []
    for _ in range(3):
        for _ in range(5):
            native.check(lib.vqk_calib_copy(x.data_ptr(), dst.data_ptr(), nbytes, st), 'calib_copy')
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            native.check(lib.vqk_calib_copy(x.data_ptr(), dst.data_ptr(), nbytes, st), 'calib_copy')
        e1.record()
        torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1) / 50 * 1e3)
    us, cp = statistics.median(per_pick), statistics.median(copies)
    print(f'  seeding step (2 launches), device events over {k - 1} consecutive picks: {us:.2f} us per pick (min {min(per_pick):.2f}, max '
          f'{max(per_pick):.2f}; host-issued: a pick can not be faster than the host issues its two launches) = '
          f'{nbytes / us / 1e6:.3f} TB/s of x read per pick', file=out)
    print(f'  vqk_calib_copy over the same {nbytes / 2 ** 20:.0f} MiB: {cp:.2f} us = {2 * nbytes / cp / 1e6:.3f} TB/s moved (read + write), '
          f'{nbytes / cp / 1e6:.3f} TB/s read; x stays within the 256 MiB Infinity Cache from pick to pick, the copy\'s '
          f'{2 * nbytes / 2 ** 20:.0f} MiB as well', file=out)


def bench(out, n, k, d, rounds, with_torch_fit):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(n, d, generator=g) * 0.36 + torch.randn(1, d, generator=g)).to(DEV).contiguous()
    u = torch.rand(k, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(DEV)
    same = bool(torch.equal(ops.kmeans_seed(x, k, u), torch_seed(x, k, u)))
    print(f'N = {n}, K = {k}, D = {d}; the torch formulation picks the same rows: {same} (fp32 distances in another summation order: '
          f'a pick may differ where a draw falls within rounding of a boundary)', file=out)
    res = alternate({'seeding loop, ops.kmeans_seed': lambda: ops.kmeans_seed(x, k, u),
                     'seeding loop, torch formulation': lambda: torch_seed(x, k, u)}, rounds)
    centres = x.index_select(0, ops.kmeans_seed(x, k, u)).contiguous()
    c_hip, c_torch = centres.clone(), centres.clone()
    res.update(alternate({'Lloyd iteration, ops.kmeans_lloyd_step': lambda: ops.kmeans_lloyd_step(x, c_hip),
                          'Lloyd iteration, torch formulation': lambda: torch_lloyd(x, c_torch)}, rounds))
    fits = {'fit, 10 iterations, ops.kmeans_fit': lambda: ops.kmeans_fit(x, k, 10, u)}
    if with_torch_fit:
        fits['fit, 10 iterations, torch formulation'] = lambda: torch_fit(x, k, 10, u)
    res.update(alternate(fits, rounds))
    for name, (med, lo, hi) in res.items():
        print(f'  {name:42s} {med:10.3f} ms   (min {lo:.3f}, max {hi:.3f}; {rounds} rounds, host clock around a synchronise)', file=out)
    a, b = res['seeding loop, ops.kmeans_seed'], res['seeding loop, torch formulation']
    print(f'  seeding: torch / HIP = {b[0] / a[0]:.2f}; floor of K passes over N x D x 4 bytes at the copy\'s read rate: see below', file=out)
    seed_step_rate(out, x, k, u)
    out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmeans_bench.txt'))
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--rows', type=int, default=65536)
    ap.add_argument('--codes', type=int, nargs='+', default=[1024, 8192])
    args = ap.parse_args()
    with open(args.out, 'w') as out:
        print(f'tools/kmeans_bench.py on {torch.cuda.get_device_name(0)}: medians, the contenders alternating in one process.', file=out)
        for k in args.codes:
            bench(out, args.rows, k, 256, args.rounds, with_torch_fit=True)
    print(open(args.out).read())


if __name__ == '__main__':
    main()
