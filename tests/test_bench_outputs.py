"""bench.py's output contract, on the CPU: the arrays ``--dump-outputs`` writes (names, dtypes, the seeded sample of a large tensor,
the size cap) and the command line its HBM-traffic passes run (workload options kept, run length / measurement / output dropped)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    return importlib.import_module('bench')


def _model():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 64, 3), torch.nn.BatchNorm2d(64), torch.nn.Linear(300, 200))
    m[0](torch.randn(1, 3, 8, 8)).sum().backward()          # gradients for the conv only
    return m


def test_dump_outputs_names_dtypes_and_sample(tmp_path):
    bench = _bench()
    m = _model()
    d = bench.dump_outputs(str(tmp_path / 'a'), m, torch.tensor(0.5))
    files = sorted(os.listdir(tmp_path / 'a'))
    want = (['loss.npy'] + [f'state.{k}.npy' for k in m.state_dict()] +
            [f'grad.{k}.npy' for k, p in m.named_parameters() if p.grad is not None])
    assert files == sorted(want) and d['files'] == len(want)
    arr = {f[:-4]: np.load(tmp_path / 'a' / f) for f in files}
    assert arr['loss'].dtype == np.float64 and arr['loss'].tolist() == [0.5]
    assert arr['state.1.num_batches_tracked'].dtype == np.float64                 # integer buffers as float64
    assert all(a.dtype == np.float32 for k, a in arr.items() if k not in ('loss', 'state.1.num_batches_tracked'))
    np.testing.assert_array_equal(arr['grad.0.weight'], m[0].weight.grad.reshape(-1).numpy())  # small tensors whole
    big = m[2].weight.detach().reshape(-1)                                        # 60000 > DUMP_SAMPLE elements
    assert big.numel() > bench.DUMP_SAMPLE
    idx = torch.randint(big.numel(), (bench.DUMP_SAMPLE,), generator=torch.Generator().manual_seed(big.numel()))
    np.testing.assert_array_equal(arr['state.2.weight'], big[idx].numpy())
    assert d['bytes'] == sum(a.nbytes for a in arr.values())
    bench.dump_outputs(str(tmp_path / 'b'), m, torch.tensor(0.5))                # the same sample in every call
    for f in files:
        np.testing.assert_array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f))


def test_dump_outputs_size_cap(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, 'DUMP_LIMIT', 1 << 16)
    with pytest.raises(RuntimeError, match='--dump-outputs'):
        bench.dump_outputs(str(tmp_path), _model(), torch.tensor(0.5))


def test_traffic_passes_keep_only_the_workload_options():
    bench = _bench()
    argv = ['--gan', '--batch', '16', '--full', '--dump-outputs', 'out', '--steps', '5', '--warmup=2', '--dump-outputs=o2',
            '--no-graph', '--sustain-s', '0', '--quick', '--dtype', 'bf16x3', '--deterministic']
    assert bench.traffic_argv(argv) == ['--gan', '--batch', '16', '--dtype', 'bf16x3', '--deterministic']
