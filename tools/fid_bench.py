"""Time the FID Inception-v3 (fid.py) on one MI355X and print one JSON line.

    python tools/fid_bench.py [--batch 32] [--size 256] [--runs 30] [--warmup 5]

InceptionFeatures.features at B = --batch from --size^2 inputs (random weights in the published naming: the time does not depend
on the values): median of --runs device-event timings after --warmup untimed runs, images/s, TF/s of the 11.42 GFLOP per image
and its share of the 157.3 TF fp32 peak.  The split into conv / pool / preprocess / statistics comes from HIP events around every
launch, in separate runs (the events add host work).  Last, VQVAE.test_step on the config-2 model (channels 128, mult 1-2-2-4,
K = 1024, bf16) at the same batch, with and without rFID."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'vqvae-vqgan-pytorch-lightning_amd'
GFLOP_PER_IMAGE = 11.42
PEAK_TF = 157.3


def random_weights(seed=0):
    fid = importlib.import_module(PKG + '.fid')
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in fid.expected_keys().items():
        if key.endswith('conv.weight'):
            sd[key] = torch.randn(*shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif key.endswith('running_var') or key.endswith('bn.weight'):
            sd[key] = 0.5 + torch.rand(*shape, generator=g)
        else:
            sd[key] = 0.1 * torch.randn(*shape, generator=g)
    return sd


def time_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-test-step', action='store_true', help='skip the test_step timing of the config-2 model')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('fid_bench.py needs an MI355X')
    fid = importlib.import_module(PKG + '.fid')
    dev = torch.device('cuda:0')
    net = fid.InceptionFeatures(random_weights(), dev)
    b = args.batch
    images = torch.rand(b, 3, args.size, args.size, generator=torch.Generator().manual_seed(1)).to(dev)
    med, lo, hi = time_ms(lambda: net.features(images), args.runs, args.warmup)
    tf = GFLOP_PER_IMAGE * 1e9 * b / (med * 1e-3) / 1e12
    res = dict(batch=b, size=args.size, runs=args.runs, features_ms_median=round(med, 3), features_ms_min=round(lo, 3),
               features_ms_max=round(hi, 3), images_per_s=round(b / (med * 1e-3), 1), tflops=round(tf, 2),
               fraction_of_peak=round(tf / PEAK_TF, 4))

    # split by kind: events around every launch, summed per run, median over runs
    metric = fid.FrechetInceptionDistance(net)
    per_kind = {k: [] for k in ('conv', 'pool', 'preprocess', 'stats')}
    per_conv = {}
    for i in range(args.warmup + args.runs):
        net.events = []
        f = net.features(images)
        metric.update_features(f, True)
        torch.cuda.synchronize()
        if i < args.warmup:
            continue
        sums = {k: 0.0 for k in per_kind}
        convs = [e for e in net.events if e[0] == 'conv']
        for kind, e0, e1 in net.events:
            sums[kind] += e0.elapsed_time(e1)
        for j, (_, e0, e1) in enumerate(convs):
            per_conv.setdefault(j, []).append(e0.elapsed_time(e1))
        for k in per_kind:
            per_kind[k].append(sums[k])
    net.events = None
    res['split_ms_median'] = {k: round(statistics.median(v), 3) for k, v in per_kind.items()}
    names = list(fid.conv_specs())
    conv_med = sorted(((statistics.median(v), names[j]) for j, v in per_conv.items()), reverse=True)
    res['slowest_convs_ms'] = [[n, round(t, 3)] for t, n in conv_med[:8]]
    res['convs_per_batch'] = len(per_conv)

    if not args.no_test_step:
        model_mod = importlib.import_module(PKG + '.model')
        ae = dict(channels=128, num_res_blocks=2, channel_multipliers=(1, 2, 2, 4))
        qc = dict(num_embeddings=1024, embedding_dim=256, reinit_every_n_epochs=None, type='standard',
                  params=dict(commitment_cost=0.25))
        torch.manual_seed(0)
        model = model_mod.VQVAE(256, ae, qc, None, None, compute_dtype=torch.bfloat16).to(dev).eval()
        batch = torch.rand(b, 3, 256, 256, generator=torch.Generator().manual_seed(2)).to(dev)
        out = {}
        for label, weights in (('without_fid', None), ('with_fid', random_weights())):
            model.fid_weights = weights
            model.on_test_epoch_start()
            med_ts, _, _ = time_ms(lambda: model.test_step(batch, 0), max(10, args.runs // 2), args.warmup)
            out[label] = round(med_ts, 3)
        res['test_step_ms_median'] = out
    print(json.dumps(res), flush=True)
    return res


if __name__ == '__main__':
    main()
