"""The scalar log on the GPU: vqk_scalar_accum and vqk_arena_stats against the float64 restatement of
tests/scalarlog_reference.py, and the log end to end through MiniTrainer (eager, graphed, VQ-GAN with its re-capture, validation,
train.py --log_dir) on the small 64 x 64 configs the other tests use.

Bounds.  ``sum`` / ``wsum`` of the scalar accumulators: BITWISE equal to the float64 host loop (exact products, fixed order).
``sumsq`` of the arena statistics: relative error at most n * 2^-53 for a group of n finite elements -- the bound of any order of n
float64 additions of non-negative, exactly represented terms (the float64 squares, which the kernel and the reference round
identically); ``norm`` within half of that plus 2^-52; ``maxabs`` and ``nonfinite`` exact; two runs bitwise equal.  The reference
sum is ``math.fsum`` up to 2^20 elements and numpy's pairwise float64 sum above.

Ablation: the check run with the fp64 accumulators of arena_stats_kernel / arena_finish_kernel replaced by fp32 ones (squares
still taken in fp64, then rounded and added in fp32) has NOT been made yet.  What to expect of it: an fp32 sum carries a relative
error of the order of 2^-24 per addition, seven orders of magnitude above n * 2^-53 for every case here (n from 50 to 1.7e7), and
the inputs span twelve decades -- every arena case must fail under it, the large ones by the widest margin.
"""
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import scalarlog_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
model_mod = importlib.import_module(PKG + '.model')
trainer_mod = importlib.import_module(PKG + '.trainer')
scalarlog = importlib.import_module(PKG + '.scalarlog')
ops = importlib.import_module(PKG + '.ops')
DEV = 'cuda:0'
S, B = 64, 4
AE = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
TC = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
QC_STD = dict(num_embeddings=64, embedding_dim=16, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
QC_EMA = dict(num_embeddings=64, embedding_dim=16, reinit_every_n_epochs=None, type='ema',
              params=dict(commitment_cost=0.25, decay=0.95, epsilon=1e-5))
LC_GAN = dict(l1_weight=0.8, l2_weight=0.2, perc_weight=1.0,
              adversarial_params=dict(start_epoch=1, loss_type='non-saturating', g_weight=0.1, use_adaptive=False,
                                      r1_reg_weight=10.0, r1_reg_every=2))

@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.set_deterministic(False)


def _same(a, b):
    """equal as float64 values, NaN equal to NaN"""
    return (math.isnan(a) and math.isnan(b)) or a == b


def _lines(path):
    return [json.loads(line) for line in open(path, encoding='utf-8').read().splitlines()]


# ---------------------------------------------------------------------------------------------- vqk_scalar_accum
def _new_block(nslots):
    blk = torch.zeros(nslots, ops.SCALAR_SLOT, dtype=torch.float64)
    blk[:, 3], blk[:, 4] = math.inf, -math.inf
    return blk.to(DEV)


@pytest.mark.parametrize('weights', ['ones', 'short_last_batch'])
def test_scalar_accum_is_the_float64_host_loop(weights):
    steps, n32, n16 = 200, 4, 3
    g = torch.Generator().manual_seed(1)
    v32 = (torch.randn(steps, n32, generator=g) * torch.tensor([1.0, 1e-3, 1e4, 3.0])).float()
    v16 = (torch.randn(steps, n16, generator=g) * 5.0).to(torch.bfloat16)
    v32[50, 1], v32[60, 2], v32[199, 3] = math.nan, math.inf, -0.0
    v16[70, 0], v16[71, 0] = -math.inf, math.nan
    w = [1] * steps if weights == 'ones' else [32] * (steps - 1) + [7]
    d32, d16 = v32.to(DEV), v16.to(DEV)
    blk = _new_block(12)
    slots = [5, 0, 11, 2, 7, 3, 9]                                    # any slots, in any order
    for i in range(steps):
        ops.scalar_accum([d32[i, j] for j in range(n32)] + [d16[i, j] for j in range(n16)], [w[i]] * 7, slots, blk)
    got = blk.cpu().tolist()
    for j in range(7):
        col = v32[:, j] if j < n32 else v16[:, j - n32].float()
        ref = R.new_slot()
        for i in range(steps):
            R.scalar_accum(ref, float(col[i]), w[i])
        row = got[slots[j]]
        print(f'SCALARLOGMEASURE accum {weights} source {j}: sum {row[0]!r} ref {ref[0]!r} wsum {row[1]} nonfinite {row[5]}')
        assert _same(row[0], ref[0]) and (math.isnan(ref[0]) or np.float64(row[0]).tobytes() == np.float64(ref[0]).tobytes())
        assert row[1] == ref[1] == float(sum(w))
        assert _same(row[2], ref[2]) and (math.isnan(ref[2]) or math.copysign(1.0, row[2]) == math.copysign(1.0, ref[2]))
        assert row[3] == ref[3] and row[4] == ref[4] and row[5] == ref[5] and row[6] == steps
    assert math.isnan(got[0][0]) and got[0][5] == 1.0                 # the NaN is counted and propagates into the sum
    assert got[11][0] == math.inf and got[11][4] == math.inf          # +Inf
    assert math.isnan(got[7][0]) and got[7][3] == -math.inf and got[7][5] == 2.0      # -Inf then NaN (bf16)
    for untouched in (1, 4, 6, 8, 10):
        assert got[untouched] == [0.0, 0.0, 0.0, math.inf, -math.inf, 0.0, 0.0, 0.0]


def test_scalar_accum_more_than_sixteen_sources_and_refusals():
    vals = torch.arange(1, 21, dtype=torch.float32).to(DEV)
    blk = _new_block(20)
    ops.scalar_accum([vals[k] for k in range(20)], [3] * 20, list(range(20)), blk)
    got = blk.cpu()
    assert got[:, 0].tolist() == [3.0 * k for k in range(1, 21)] and got[:, 1].tolist() == [3.0] * 20
    with pytest.raises(RuntimeError):
        ops.scalar_accum([vals[0].double()], [1], [0], blk)
    with pytest.raises(RuntimeError):
        ops.scalar_accum([vals[0], vals[1]], [1, 1], [2, 2], blk)


def test_scalar_accum_replayed_n_times_accumulates_n_times():
    static = torch.zeros(3, dtype=torch.float32, device=DEV)
    static16 = torch.zeros(2, dtype=torch.bfloat16, device=DEV)
    blk = _new_block(5)
    srcs = [static[0], static[1], static[2], static16[0], static16[1]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.scalar_accum(srcs, [32] * 5, [0, 1, 2, 3, 4], blk)
    torch.cuda.synchronize()
    assert blk.cpu()[:, 1].tolist() == [0.0] * 5                      # the capture ran nothing
    g = torch.Generator().manual_seed(2)
    refs = [R.new_slot() for _ in range(5)]
    for _ in range(9):
        a, b = torch.randn(3, generator=g), torch.randn(2, generator=g).to(torch.bfloat16)
        static.copy_(a)
        static16.copy_(b)
        graph.replay()
        for j in range(5):
            R.scalar_accum(refs[j], float(a[j]) if j < 3 else float(b[j - 3]), 32)
    got = blk.cpu().tolist()
    for j in range(5):
        assert got[j][:7] == refs[j] and got[j][6] == 9.0


# ---------------------------------------------------------------------------------------------- vqk_arena_stats
def _wide(n, rng):
    """fp32 values over twelve decades: an fp32 accumulation of their squares is nowhere near the bound"""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)


def _arena(lengths, groups, rng, fill=_wide):
    """tensors of the given lengths on 64-element boundaries, the padding poisoned with NaN: (g, seg_end, seg_group)"""
    g, seg_end, seg_group, off = [], [], [], 0
    for n, grp in zip(lengths, groups):
        g.append(fill(n, rng))
        off += n
        seg_end.append(off)
        seg_group.append(grp)
        pad = -n % 64
        if pad:
            g.append(np.full(pad, np.nan, dtype=np.float32))
            off += pad
            seg_end.append(off)
            seg_group.append(-1)
    return np.concatenate(g), seg_end, seg_group


def _run_arena(g, seg_end, seg_group, ngroups, scale, repeat=1):
    dg = torch.from_numpy(g).to(DEV)
    de = torch.tensor(seg_end, dtype=torch.int64, device=DEV)
    dgrp = torch.tensor(seg_group, dtype=torch.int32, device=DEV)
    ws = torch.full((ops.arena_stats_ws_doubles(g.size, ngroups),), math.nan, dtype=torch.float64, device=DEV)
    out = torch.full((ngroups + 1, 3), math.nan, dtype=torch.float64, device=DEV)
    acc = torch.zeros(ngroups + 1, ops.ARENA_ACC, dtype=torch.float64, device=DEV)
    for _ in range(repeat):
        ops.arena_stats(dg, de, dgrp, ngroups, scale, ws, out, acc)
    return out.cpu(), acc.cpu()


def _check_arena(name, g, seg_end, seg_group, ngroups, scale):
    out, acc = _run_arena(g, seg_end, seg_group, ngroups, scale)
    out2, acc2 = _run_arena(g, seg_end, seg_group, ngroups, scale)
    assert torch.equal(out, out2) and torch.equal(acc, acc2), name   # bitwise from run to run
    ref, counts = R.arena_stats(g, seg_end, seg_group, ngroups, scale)
    worst = 0.0
    for q in range(ngroups + 1):
        sumsq, maxabs, nonfinite = out[q].tolist()
        assert maxabs == ref[q][1] and nonfinite == ref[q][2], (name, q)
        rel = abs(sumsq - ref[q][0]) / ref[q][0] if ref[q][0] else abs(sumsq)
        worst = max(worst, rel / R.sumsq_bound(counts[q]))
        assert rel <= R.sumsq_bound(counts[q]), (name, q, rel, counts[q])
        norm, want = float(acc[q, 0]), math.sqrt(ref[q][0])
        assert (abs(norm - want) / want if want else abs(norm)) <= R.norm_bound(counts[q]), (name, q)
        assert acc[q].tolist() == [norm, norm, maxabs, nonfinite, 1.0], (name, q)
    print(f'SCALARLOGMEASURE arena {name}: {g.size} elements, worst sumsq error / bound {worst:.3e}')
    return out, ref


def test_arena_stats_one_short_segment():
    rng = np.random.default_rng(3)
    g, e, s = _arena([50], [0], rng)
    out, _ = _check_arena('one segment of 50', g, e, s, 1, 1.0)
    assert float(out[0, 2]) == 0.0                                    # the 14 NaN of the padding are in no result


def test_arena_stats_ragged_interleaved_groups():
    rng = np.random.default_rng(4)
    lengths = rng.integers(1, 700, 300).tolist() + [9000, 1, 63, 64, 65]
    groups = rng.integers(0, 5, len(lengths)).tolist()
    g, e, s = _arena(lengths, groups, rng)
    assert g.size > 8 * 8192                                          # several chunks
    _check_arena('ragged', g, e, s, 5, 1.0)
    _check_arena('ragged, scale 1/8', g, e, s, 5, 0.125)
    _check_arena('ragged, scale 1/3', g, e, s, 5, 1.0 / 3.0)
    # a group no segment names, and the largest number of groups
    _check_arena('ragged, eight groups', g, e, [x if x < 0 else (x * 3) % 8 for x in s], 8, 0.5)


def test_arena_stats_special_values():
    rng = np.random.default_rng(5)

    def fill(n, rng):
        v = _wide(n, rng)
        v[::7] = rng.choice(np.array([1e-45, -3e-42, 1.1e-38, -0.0, 0.0], dtype=np.float32), v[::7].size)      # denormals, -0
        return v
    lengths = [5000, 129, 40000, 77]
    g, e, s = _arena(lengths, [0, 1, 2, 1], rng, fill)
    _check_arena('denormals and -0', g, e, s, 3, 1.0)
    zeros, ze, zs = _arena([100, 200], [0, 1], rng, lambda n, r: np.full(n, -0.0, dtype=np.float32))
    out, _ = _check_arena('all -0', zeros, ze, zs, 2, 1.0)
    assert out[:, :2].abs().sum() == 0 and not torch.signbit(out[:, 1]).any()
    bad = g.copy()
    assert e[:4] == [5000, 5056, 5185, 5248]                          # tensor, padding, tensor, padding
    bad[3], bad[4999], bad[5056 + 5], bad[5248 + 39999] = np.nan, np.inf, -np.inf, np.nan             # groups 0, 0, 1, 2
    out, ref = _check_arena('injected NaN / Inf', bad, e, s, 3, 0.25)
    assert out[:, 2].tolist() == [2.0, 1.0, 1.0, 4.0]
    assert torch.isfinite(out).all()


@pytest.mark.parametrize('numel', [8 * 1024 * 1024 + 192, 2048 * 8192 + 3 * 8192 + 320])
def test_arena_stats_large(numel):
    """about 8M elements (the fsum / pairwise reference split is at 1M per group), and an arena above the grid cap (2048 blocks
    of 8192 elements: the blocks stride over it)"""
    rng = np.random.default_rng(6)
    lengths = [numel // 2 - 37, 300_000, numel // 4 + 11, 1_000_000]
    lengths.append(numel - sum(-(-n // 64) * 64 for n in lengths) - 64 + 5)
    g, e, s = _arena(lengths, [0, 1, 2, 1, 0], rng)
    assert g.size == numel
    _check_arena(f'large {numel}', g, e, s, 3, 0.5)


# ---------------------------------------------------------------------------------------------- end to end
def _batches(count, seed=5, last=None):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(B if (last is None or i < count - 1) else last, 3, S, S, generator=g).to(DEV) for i in range(count)]


def _model(qc=QC_STD, lc=None, dtype=torch.float32, seed=0):
    torch.manual_seed(seed)
    return model_mod.VQVAE(S, AE, qc, lc, TC, compute_dtype=dtype).to(DEV).train()


def _mean64(values):
    total = 0.0
    for v in values:                                                  # the order the steps arrived in
        total += float(v)
    return total / len(values)


def _train(qc, lc, graphed, log_dir, keys, epochs=2, steps=4, seed=3, deterministic=True):
    """epochs x steps; the test synchronises after every step and collects float(value) of each key itself.  Returns (per epoch
    {key: [values]}, per epoch record, final state)"""
    m = _model(qc, lc, seed=seed)
    if log_dir is not None:
        m.scalar_log = scalarlog.ScalarLog(log_dir, log_every_n_steps=3)
    tr = trainer_mod.MiniTrainer(max_epochs=epochs, num_training_batches=steps, deterministic=deterministic)
    tr.attach(m)
    m.on_train_start()
    feed = _batches(steps, seed=15)
    if graphed:
        tr.capture(m, feed[0], warmup=1, preserve_state=True)
    step = tr.train_batch_graphed if graphed else tr.train_batch
    collected, records = [], []
    for epoch in range(epochs):
        m.current_epoch = epoch
        per = {k: [] for k in keys}
        for i in range(steps):
            step(m, feed[i], i)
            torch.cuda.synchronize()
            for k in keys:
                per[k].append(float(m.logged[k]))
        m.on_train_epoch_end()
        records.append(tr.log_train_epoch(m))
        collected.append(per)
    torch.cuda.synchronize()
    state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for j, o in enumerate(tr.optimizers):
        state[f'optimizer{j}.v'] = o.flat_v.detach().cpu().clone()
    if m.scalar_log is not None:
        m.scalar_log.close()
    return collected, records, state


MSE_KEYS = ('train/loss', 'train/l2_loss', 'train/quant_loss')


_RUNS = {}


def _both_runs(qname, graphed, tmp_path_factory):
    """the run with the log and the run without it, once per (quantizer, mode) for the two tests below"""
    if (qname, graphed) not in _RUNS:
        qc = QC_STD if qname == 'standard' else QC_EMA
        log_dir = str(tmp_path_factory.mktemp(f'log_{qname}_{int(graphed)}'))
        on = _train(qc, None, graphed, log_dir, MSE_KEYS)
        ops.set_deterministic(False)
        off = _train(qc, None, graphed, None, MSE_KEYS)
        _RUNS[(qname, graphed)] = (log_dir, on, off)
    return _RUNS[(qname, graphed)]


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
@pytest.mark.parametrize('qname', ['standard', 'ema'])
def test_epoch_means_are_exact(tmp_path_factory, qname, graphed):
    """2 epochs x 4 steps in deterministic fp32 mode; the test synchronises after every step and collects float(value) itself:
    the written train/loss, train/l2_loss and train/quant_loss equal the float64 mean of the collected values exactly"""
    log_dir, (collected, records, _), (_, none, _) = _both_runs(qname, graphed, tmp_path_factory)
    assert none == [None, None]
    recs = _lines(os.path.join(log_dir, 'metrics.jsonl'))
    epochs = [r for r in recs if r['event'] == 'train_epoch']
    assert len(epochs) == 2 and [r['epoch'] for r in epochs] == [0, 1] and [r['global_step'] for r in epochs] == [4, 8]
    for e in range(2):
        for k in MSE_KEYS:
            want = _mean64(collected[e][k])
            print(f'SCALARLOGMEASURE {qname} graphed={graphed} epoch {e} {k}: logged {epochs[e][k]!r} collected mean {want!r}')
            assert epochs[e][k] == want == records[e][k], (e, k)
            st = epochs[e]['stats'][k]
            assert st['wsum'] == 4.0 and st['last'] == collected[e][k][-1]
            assert st['min'] == min(collected[e][k]) and st['max'] == max(collected[e][k])
        assert epochs[e]['nonfinite_values'] == 0.0
        for grp in ('encoder', 'decoder', 'all') + (('quantizer',) if qname == 'standard' else ()):
            assert epochs[e][f'grad/{grp}/norm_mean'] > 0.0 and epochs[e][f'grad/{grp}/nonfinite'] == 0.0
            assert epochs[e][f'grad/{grp}/norm_max'] >= epochs[e][f'grad/{grp}/norm_mean'] > 0.0
    steps = [r for r in recs if r['event'] == 'step']
    assert [r['global_step'] for r in steps] == [3, 6] and all(r['lr'] == TC['lr'] for r in steps)


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
@pytest.mark.parametrize('qname', ['standard', 'ema'])
def test_log_leaves_training_bit_identical(tmp_path_factory, qname, graphed):
    """deterministic mode: every trained tensor, buffer and second moment after the 8 steps is bit-identical with and without
    the log attached.

    The EMA quantizer is held to the same bound: in deterministic mode its statistics are added in row order
    (ema_stats_ordered_kernel, csrc/vq.hip; tests/test_gpu_ema_ordered.py) -- with the atomic form the codebook differs in its
    last bits between ANY two runs, log or no log (seen on an MI355X: the first tensor to differ was quantizer.ema_weight)."""
    _, (_, _, s_on), (_, _, s_off) = _both_runs(qname, graphed, tmp_path_factory)
    assert set(s_on) == set(s_off)
    differ = [k for k in s_on if not torch.equal(s_on[k], s_off[k])]
    print(f'SCALARLOGMEASURE {qname} graphed={graphed}: {len(differ)} of {len(s_on)} tensors differ with / without the log {differ[:4]}')
    assert not differ


GAN_KEYS = ('train/loss', 'train/l1_loss', 'train/l2_loss', 'train/quant_loss', 'train/perc_loss', 'train/gen_loss',
            'train/disc_loss', 'g_weight', 'r1_penalty')


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
def test_vqgan_epoch_means_across_the_adversarial_start(tmp_path, graphed):
    """start_epoch = 1, R1 every second step: epoch 0 has no adversarial term (g_weight / r1_penalty are Python zeros), epoch 1
    has both discriminator variants; graphed, the epoch boundary re-captures the three graphs -- whose settling steps must not
    reach the accumulators"""
    collected, records, _ = _train(QC_STD, LC_GAN, graphed, str(tmp_path), GAN_KEYS, deterministic=None)
    epochs = [r for r in _lines(tmp_path / 'metrics.jsonl') if r['event'] == 'train_epoch']
    assert len(epochs) == 2
    for e in range(2):
        for k in GAN_KEYS:
            want = _mean64(collected[e][k])
            print(f'SCALARLOGMEASURE vqgan graphed={graphed} epoch {e} {k}: logged {epochs[e][k]!r} collected mean {want!r}')
            assert epochs[e][k] == want, (e, k)
            assert epochs[e]['stats'][k]['wsum'] == 4.0, (e, k)      # the real steps, nothing from a settling step
            assert epochs[e]['stats'][k]['last'] == collected[e][k][-1]
        assert 'grad/all/norm_mean' in epochs[e] and ('grad/discriminator/norm_mean' in epochs[e]) == (e == 1)
    assert epochs[0]['g_weight'] == 0.0 and epochs[0]['train/gen_loss'] == 0.0 and epochs[0]['r1_penalty'] == 0.0
    assert epochs[1]['g_weight'] == 0.1 or abs(epochs[1]['g_weight'] - 0.1) < 1e-7
    assert epochs[1]['train/gen_loss'] != 0.0 and epochs[1]['train/disc_loss'] != 0.0
    r1 = collected[1]['r1_penalty']
    assert r1[0] != 0.0 and r1[1] == 0.0 and r1[2] != 0.0 and r1[3] == 0.0          # both R1 variants ran
    assert epochs[1]['stats']['r1_penalty']['max'] == max(r1)


def test_grad_stats_see_the_arena_the_optimizer_steps_on(tmp_path):
    m = _model(seed=4)
    log = m.scalar_log = scalarlog.ScalarLog(str(tmp_path))
    tr = trainer_mod.MiniTrainer(max_epochs=1, num_training_batches=2)
    tr.attach(m)
    m.on_train_start()
    opt = tr.optimizers[0]
    feed = _batches(2, seed=16)
    copies = []
    real_step = opt.step

    def step_with_copy():                                             # right after the all-reduce and the statistics: the arena AdamW reads
        copies.append((opt.flat_g.detach().cpu().numpy().copy(), float(opt.grad_scale)))
        return real_step()
    opt.step = step_with_copy
    tr.train_batch(m, feed[0], 0)
    rec = tr.log_train_epoch(m)
    g0, scale = copies[0]
    st = log._opts['autoencoder']
    seg_end, seg_group = opt.seg_end.tolist(), st['seg_group'].tolist()
    assert st['names'] == ['encoder', 'decoder', 'quantizer']
    ref, counts = R.arena_stats(g0, seg_end, seg_group, 3, scale)
    for q, name in enumerate(('encoder', 'decoder', 'quantizer', 'all')):
        want = math.sqrt(ref[q][0])
        got = rec[f'grad/{name}/norm_mean']
        print(f'SCALARLOGMEASURE grad/{name}: norm {got!r} reference {want!r} maxabs {rec[f"grad/{name}/maxabs"]!r}')
        assert abs(got - want) / want <= R.norm_bound(counts[q]) and rec[f'grad/{name}/norm_max'] == got
        assert rec[f'grad/{name}/maxabs'] == ref[q][1] and rec[f'grad/{name}/nonfinite'] == 0.0
    # a NaN written into one gradient element before opt.step(): hooked in front of the trainer's statistics call
    opt.step = real_step
    real_stats = log.grad_stats
    p = next(m.decoder.parameters())

    def poisoned(o, name):
        o.flat_g[o.offsets[id(p)] + 1] = math.nan
        return real_stats(o, name)
    log.grad_stats = poisoned
    tr.train_batch(m, feed[1], 1)
    rec = tr.log_train_epoch(m)
    assert rec['grad/decoder/nonfinite'] == 1.0 and rec['grad/all/nonfinite'] == 1.0
    assert rec['grad/encoder/nonfinite'] == 0.0 and rec['grad/quantizer/nonfinite'] == 0.0
    assert math.isfinite(rec['grad/decoder/norm_mean']) and rec['grad/decoder/norm_mean'] > 0.0
    log.close()


def test_validation_means_are_batch_size_weighted(tmp_path):
    feed = _batches(3, seed=17, last=3)                               # 4, 4, 3 images
    m = _model(seed=5)
    tr = trainer_mod.MiniTrainer()
    tr.attach(m)
    plain = tr.validate(m, feed)                                      # no log: today's return
    assert set(plain) == {'validation/loss', 'val_metrics/used_codebook', 'val_metrics/perplexity'}
    log = m.scalar_log = scalarlog.ScalarLog(str(tmp_path))
    seen = []
    real = log.validation_step

    def collecting(logged, batch_size):
        torch.cuda.synchronize()
        seen.append(({k: float(v) for k, v in logged.items() if k.startswith('validation/')}, batch_size))
        return real(logged, batch_size)
    log.validation_step = collecting
    m.current_epoch = 4
    out = tr.validate(m, feed)
    assert [b for _, b in seen] == [4, 4, 3] and set(out) == set(plain)
    keys = sorted(seen[0][0])
    assert 'validation/loss' in keys
    rec = _lines(tmp_path / 'metrics.jsonl')
    assert len(rec) == 1 and rec[0]['event'] == 'validation' and rec[0]['epoch'] == 4
    for k in keys:
        total = 0.0
        for vals, b in seen:
            total += vals[k] * b
        assert out[k] == total / 11.0 == rec[0][k], k
        assert rec[0]['stats'][k]['wsum'] == 11.0
    for k in ('val_metrics/used_codebook', 'val_metrics/perplexity'):
        assert rec[0][k] == out[k] == plain[k]
    # (two forwards of the same batches: the loss is an fp32 atomic sum, 1e-6 relative from run to run -- tests/test_gpu_data_loop.py
    # -- and the log-less return adds the three batches in fp32)
    assert abs(out['validation/loss'] - plain['validation/loss']) <= 5e-6 * abs(plain['validation/loss'])
    m.scalar_log = None
    again = tr.validate(m, feed)
    assert set(again) == set(plain) and abs(again['validation/loss'] - plain['validation/loss']) <= 5e-6 * abs(plain['validation/loss'])
    log.close()


@pytest.mark.parametrize('qtype', ['standard', 'gumbel'])
def test_train_py_log_dir(tmp_path, capsys, qtype):
    """train.py --log_dir on synthetic batches, graphed: DIR/run_name/metrics.jsonl with one train_epoch record per epoch and step
    records that carry the lr the scheduler set (and the Gumbel schedule for a Gumbel config)"""
    train = importlib.import_module(PKG + '.train')
    sched = importlib.import_module(PKG + '.schedulers')
    conf = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'example_confs', 'standard_vqvae.yaml')
    sets = [f'image_size={S}', 'autoencoder.channels=32', 'autoencoder.num_res_blocks=1', 'autoencoder.channel_multipliers=[1, 2]',
            'quantizer.num_embeddings=64', 'quantizer.embedding_dim=16', 'training.cumulative_bs=4', 'training.decay_epochs=3']
    if qtype == 'gumbel':
        sets += ['quantizer.type=gumbel', 'quantizer.params={straight_through: false, temp: 1.0, kl_cost: 0.0005, '
                                          'kl_warmup_epochs: 1, temp_decay_epochs: 2, temp_final: 0.25}']
    args = ['--params_file', conf, '--seed', '3', '--max_epochs', '3', '--batches_per_epoch', '4', '--dtype', 'bf16',
            '--log_dir', str(tmp_path), '--run_name', 'r1', '--log_every_n_steps', '2']
    for item in sets:
        args += ['--set', item]
    capsys.readouterr()
    loss = train.main(args)
    out = capsys.readouterr().out
    assert np.isfinite(loss) and 'eager launches' not in out
    assert '[epoch 2] train/l2_loss' in out                           # the console prints the epoch means
    recs = _lines(tmp_path / 'r1' / 'metrics.jsonl')
    epochs = [r for r in recs if r['event'] == 'train_epoch']
    assert [r['epoch'] for r in epochs] == [0, 1, 2] and [r['global_step'] for r in epochs] == [4, 8, 12]
    assert all(math.isfinite(r['train/loss']) and r['stats']['train/loss']['wsum'] == 4.0 for r in epochs)
    assert all(r['grad/all/norm_mean'] > 0.0 and r['grad/all/nonfinite'] == 0.0 for r in epochs)
    steps = [r for r in recs if r['event'] == 'step']
    assert [r['global_step'] for r in steps] == [2, 4, 6, 8, 10, 12] and [r['epoch'] for r in steps] == [0, 0, 1, 1, 2, 2]
    # the half-cosine over 3 epochs x 4 batches (model.on_train_start): the lr of the step that just ran, index global_step - 1
    lr = train.derive_run_config(train.get_model_conf(conf), 1, train.parse_overrides(sets))['learning_rate']
    cos = sched.CosineScheduler(0, 3 * 4, lr, lr / 2.)
    for r in steps:
        assert r['lr'] == cos.step(r['global_step'] - 1), r
        assert {'gumbel_quantizer/temperature', 'gumbel_quantizer/kl_constant'} <= set(r)      # logged for every config (model.py:229-230)
    assert steps[0]['lr'] > steps[-1]['lr'] > lr / 2.
    if qtype == 'gumbel':
        temp = sched.CosineScheduler(0, 2 * 4, 1.0, 0.25)
        kl = sched.CosineScheduler(0, 1 * 4, 0.0, 0.0005)
        for r in steps:
            assert r['gumbel_quantizer/temperature'] == temp.step(r['global_step'] - 1)
            assert r['gumbel_quantizer/kl_constant'] == kl.step(r['global_step'] - 1)
        assert steps[0]['gumbel_quantizer/temperature'] < 1.0 and steps[-1]['gumbel_quantizer/temperature'] == 0.25
    else:
        assert all(r['gumbel_quantizer/temperature'] == 0.0 for r in steps)
