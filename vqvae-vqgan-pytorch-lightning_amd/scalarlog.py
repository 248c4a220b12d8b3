"""``ScalarLog``: the scalar half of the reference's logging -- epoch means of the losses, the learning rate, the Gumbel
schedule -- plus gradient-health statistics, written as JSON lines instead of to wandb.

The reference logs through ``self.log(..., on_epoch=True, sync_dist=True)`` (vqvae/model.py:229-230, :277-286, :342-348, :365-366)
and ``LearningRateMonitor`` (vqvae/train.py:82-85, :124): Lightning averages every value over the epoch and over the ranks.  Here
the step's scalars are device tensors and the headline step is a hipGraph replay, so nothing may read them on the host per step:

  * ``train_step`` / ``validation_step`` fold the tensors ``VQVAE.log`` left in ``model.logged`` into fp64 accumulators ON THE
    DEVICE with one launch (``vqk_scalar_accum``, csrc/runstats.hip: the tensors' addresses travel as kernel arguments); values
    that arrive as Python floats (``g_weight`` / ``r1_penalty`` are ``0.`` in some phases) go to a host-side fp64 accumulator;
  * ``grad_stats`` reads a ``FlatAdamW`` gradient arena once before the optimizer step (``vqk_arena_stats``): per parameter
    group the gradient norm, the largest magnitude and the number of non-finite elements, folded into epoch accumulators;
  * ``step_event`` writes host floats only (the lr the model just set, the Gumbel temperature and KL weight) every
    ``log_every_n_steps`` optimizer steps (Lightning's default: 50);
  * ``epoch_end`` is the ONE device-to-host copy of the accumulator block, where the epoch synchronises for the code-usage
    statistics anyway; it combines the ranks (mean = sum of sums / sum of weights; maxima by max), writes one record and resets
    the block asynchronously.

Only rank 0 writes: ``log_dir/metrics.jsonl``, one JSON object per line, events ``step``, ``train_epoch`` and ``validation``, each
with ``epoch`` and ``global_step``.  Keys are the reference's names verbatim (``train/loss`` ... ``g_weight``, ``r1_penalty``,
``validation/...``, ``val_metrics/used_codebook``, ``val_metrics/perplexity``, ``gumbel_quantizer/temperature``,
``gumbel_quantizer/kl_constant``); added are ``lr``, ``grad/<group>/{norm_mean,norm_max,maxabs,nonfinite}`` (groups ``encoder``,
``decoder``, ``quantizer`` and ``all`` for the autoencoder's optimizer, ``discriminator`` for the other), ``nonfinite_values``
(how many logged values of the epoch were NaN / Inf) and, under ``stats``, each key's ``last`` / ``min`` / ``max`` / ``wsum``
of the epoch -- the reference logs its losses ``on_step=False``, so there is no per-step curve to restate.

Restated without the third-party code at hand: Lightning is not installed here, so the key ``LearningRateMonitor`` would log
(``lr-AdamW`` and its per-group variants) is NOT pinned -- the learning rate is logged as ``lr``; the step cadence follows
Lightning's documented ``log_every_n_steps`` rule (a record after every n-th optimizer step).

A non-finite mean is written as ``null`` (JSON has no NaN); ``nonfinite_values`` and ``stats`` say what happened.  The file is
line-buffered and flushed at every epoch end: a killed run keeps its log.
"""
from __future__ import annotations

import copy
import json
import math
import os

import torch
import torch.distributed as dist

TRAIN_EXTRA_KEYS = ('g_weight', 'r1_penalty')                 # vqvae/model.py:277-278: logged without the 'train/' prefix
STEP_EXTRA_KEYS = ('gumbel_quantizer/temperature', 'gumbel_quantizer/kl_constant')     # vqvae/model.py:229-230
AE_GROUPS = ('encoder', 'decoder', 'quantizer')
_SLOT = 8                                                     # ops.SCALAR_SLOT
_ACC = 5                                                      # ops.ARENA_ACC
_MAX_OPTS = 2


def build_seg_group(opt, group_of: dict) -> list:
    """One group id per segment of ``opt`` (a ``FlatAdamW``), in the order of ``opt.seg_end``: ``group_of[id(p)]`` for the segment
    that holds parameter ``p``, -1 for the alignment padding behind a tensor (optim.py lays every tensor out on a 64-element
    boundary and gives the gap a segment of its own).  Raises when a parameter has no group or the table does not reproduce the
    optimizer's own segment ends."""
    params = sorted((p for g in opt.param_groups for p in g['params']), key=lambda p: opt.offsets[id(p)])
    ends, groups = [], []
    for k, p in enumerate(params):
        off, n = opt.offsets[id(p)], p.numel()
        if id(p) not in group_of:
            raise ValueError('scalarlog: a parameter of the optimizer belongs to none of the named groups')
        ends.append(off + n)
        groups.append(int(group_of[id(p)]))
        nxt = opt.offsets[id(params[k + 1])] if k + 1 < len(params) else opt.flat_g.numel()
        if nxt != off + n:
            ends.append(nxt)
            groups.append(-1)
    if ends != [int(e) for e in opt.seg_end.tolist()]:
        raise ValueError("scalarlog: the group table does not match the optimizer's segment ends")
    return groups


def _new_host():
    return [0.0, 0.0, math.nan, math.inf, -math.inf, 0.0, 0.0]          # sum, wsum, last, min, max, nonfinite, calls


def combine_key(dev, host, dev_seq: int = 0, host_seq: int = 0):
    """device slot + host accumulator of one key -> (sum, wsum, last, min, max, nonfinite, calls); ``last`` from whichever side
    saw the key later"""
    if dev is None:
        return list(host)
    if host is None:
        return list(dev[:7])
    return [dev[0] + host[0], dev[1] + host[1], dev[2] if dev_seq > host_seq else host[2], min(dev[3], host[3]),
            max(dev[4], host[4]), dev[5] + host[5], dev[6] + host[6]]


def reduce_ranks(sums: list, maxes: list, device=None):
    """SUM all-reduce of ``sums`` and MAX all-reduce of ``maxes`` (float64) over the process group; the lists come back as they
    are without one.  Two collectives per epoch end."""
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return list(sums), list(maxes)
    dev = device if (device is not None and dist.get_backend() == 'nccl') else 'cpu'
    s = torch.tensor(sums, dtype=torch.float64, device=dev)
    m = torch.tensor(maxes, dtype=torch.float64, device=dev)
    if s.numel():
        dist.all_reduce(s, op=dist.ReduceOp.SUM)
        dist.all_reduce(m, op=dist.ReduceOp.MAX)
    return s.tolist(), m.tolist()


def _json_value(v):
    if isinstance(v, float) and not math.isfinite(v):
        return None
    if isinstance(v, dict):
        return {k: _json_value(x) for k, x in v.items()}
    return v


class ScalarLog:
    def __init__(self, log_dir: str | None, rank: int = 0, world: int = 1, log_every_n_steps: int = 50, grad_stats_every: int = 1,
                 max_keys: int = 32):
        """``log_dir`` None: accumulate and return the records, write nothing.  ``grad_stats_every`` N: gradient statistics on
        every N-th optimizer step of each optimizer (0: never)."""
        self.log_dir, self.rank, self.world = log_dir, int(rank), int(world)
        self.log_every_n_steps = max(1, int(log_every_n_steps))
        self.grad_stats_every = max(0, int(grad_stats_every))
        self.max_keys = int(max_keys)
        self.paused = False                 # MiniTrainer: the settling steps of a capture and the captured region never accumulate
        self._file = None
        self._dev = None
        self._blk = {}                      # kind -> device float64 block: max_keys slots (+ the gradient accumulators for 'train')
        self._init = {}                     # kind -> the block's reset value (device)
        self._slots = {'train': {}, 'validation': {}}          # kind -> {key: slot}
        self._host = {'train': {}, 'validation': {}}           # kind -> {key: host accumulator}
        self._seq = 0
        self._seen = {'train': {}, 'validation': {}}           # kind -> {key: [device seq, host seq]} (which side is 'last')
        self._opts = {}                     # name -> dict(index, opt, names, seg_group, ws, out, calls)
        self._pending_groups = {}           # id(opt) -> {group name: parameters}, registered before the device is known

    # ------------------------------------------------------------------ device state (allocated outside any capture)
    def _ensure(self, device):
        if self._dev is not None:
            return
        self._dev = torch.device(device)
        for kind in ('train', 'validation'):
            n = self.max_keys * _SLOT + (_MAX_OPTS * 9 * _ACC if kind == 'train' else 0)
            init = torch.zeros(n, dtype=torch.float64)
            slots = init[:self.max_keys * _SLOT].view(self.max_keys, _SLOT)
            slots[:, 3], slots[:, 4] = math.inf, -math.inf
            self._init[kind] = init.to(self._dev)
            self._blk[kind] = self._init[kind].clone()

    def _slot_block(self, kind):
        return self._blk[kind][:self.max_keys * _SLOT]

    def register_optimizer(self, opt, name: str, groups: dict | None = None) -> None:
        """name the parameter groups of ``opt`` for :meth:`grad_stats`: ``{group name: iterable of parameters}``; without a call
        (or with None) the whole arena is one group called ``name``"""
        self._pending_groups[id(opt)] = None if groups is None else {k: list(v) for k, v in groups.items()}

    def _opt_state(self, opt, name):
        st = self._opts.get(name)
        if st is not None and st['opt'] is opt:
            return st
        from . import ops
        groups = self._pending_groups.get(id(opt))
        if groups is None:
            names, group_of = [name], {id(p): 0 for g in opt.param_groups for p in g['params']}
        else:
            names = list(groups)
            group_of = {id(p): k for k, gname in enumerate(names) for p in groups[gname]}
        if len(names) > ops.ARENA_MAX_GROUPS or (st is None and len(self._opts) >= _MAX_OPTS):
            raise ValueError(f'scalarlog: at most {ops.ARENA_MAX_GROUPS} groups per optimizer and {_MAX_OPTS} optimizers')
        dev = opt.flat_g.device
        self._ensure(dev)
        index = st['index'] if st is not None else len(self._opts)
        st = dict(index=index, opt=opt, names=names, calls=0,
                  seg_group=torch.tensor(build_seg_group(opt, group_of), dtype=torch.int32, device=dev),
                  ws=torch.empty(ops.arena_stats_ws_doubles(opt.flat_g.numel(), len(names)), dtype=torch.float64, device=dev),
                  out=torch.zeros((len(names) + 1) * 3, dtype=torch.float64, device=dev))
        self._opts[name] = st
        return st

    def _grad_acc(self, st):
        lo = self.max_keys * _SLOT + st['index'] * 9 * _ACC
        return self._blk['train'][lo:lo + (len(st['names']) + 1) * _ACC]

    # ------------------------------------------------------------------ per step: no host synchronisation
    def _accumulate(self, kind, items, weight):
        from . import ops
        tensors, slots = [], []
        self._seq += 1
        for key, value in items:
            seen = self._seen[kind].setdefault(key, [0, 0])
            if torch.is_tensor(value):
                if key not in self._slots[kind]:
                    if len(self._slots[kind]) >= self.max_keys:
                        raise RuntimeError(f'scalarlog: more than {self.max_keys} logged keys')
                    self._slots[kind][key] = len(self._slots[kind])
                self._ensure(value.device)
                tensors.append(value)
                slots.append(self._slots[kind][key])
                seen[0] = self._seq
            else:
                x = float(value)
                h = self._host[kind].setdefault(key, _new_host())
                h[0] += x * weight
                h[1] += weight
                h[2] = x
                if x < h[3]:
                    h[3] = x
                if x > h[4]:
                    h[4] = x
                if not math.isfinite(x):
                    h[5] += 1.0
                h[6] += 1.0
                seen[1] = self._seq
        if tensors:
            ops.scalar_accum(tensors, [weight] * len(tensors), slots, self._slot_block(kind))

    def train_step(self, logged: dict) -> None:
        """after an optimizer step: every ``train/*`` value, ``g_weight`` and ``r1_penalty`` of ``model.logged``, weight 1"""
        if self.paused:
            return
        self._accumulate('train', [(k, v) for k, v in logged.items() if k.startswith('train/') or k in TRAIN_EXTRA_KEYS], 1)

    def validation_step(self, logged: dict, batch_size: int) -> None:
        """after a validation step: every ``validation/*`` value, weighted by the batch size (the epoch mean is the mean over
        the images, short last batch included)"""
        if self.paused:
            return
        self._accumulate('validation', [(k, v) for k, v in logged.items() if k.startswith('validation/')], int(batch_size))

    def grad_stats(self, opt, name: str):
        """between the gradient all-reduce and ``opt.step()``, on the stream the step uses: the arena's statistics at the
        optimizer's ``grad_scale`` into the epoch accumulators (every ``grad_stats_every``-th call per optimizer).  Returns the
        device row {sum x^2, max |x|, nonfinite} over ALL groups when the pass ran (the groups cover every parameter segment:
        ``build_seg_group`` refuses anything else) -- what the optimizer's step guard decides on -- else None."""
        if self.paused or not self.grad_stats_every:
            return None
        from . import ops
        st = self._opt_state(opt, name)
        st['calls'] += 1
        if (st['calls'] - 1) % self.grad_stats_every:
            return None
        ops.arena_stats(opt.flat_g, opt.seg_end, st['seg_group'], len(st['names']), float(opt.grad_scale), st['ws'], st['out'],
                        self._grad_acc(st))
        g = len(st['names'])
        return st['out'][3 * g:3 * g + 3]

    def step_event(self, global_step: int, epoch: int, lr: float, extras: dict | None = None) -> dict | None:
        """after optimizer step number ``global_step`` (1-based count of finished steps): host floats only"""
        if self.paused or global_step % self.log_every_n_steps:
            return None
        rec = {'event': 'step', 'epoch': int(epoch), 'global_step': int(global_step), 'lr': float(lr)}
        for k, v in (extras or {}).items():
            if not torch.is_tensor(v):
                rec[k] = float(v)
        self._write(rec)
        return rec

    # ------------------------------------------------------------------ epoch end: the one synchronisation
    def epoch_end(self, kind: str, epoch: int, global_step: int, extras: dict | None = None) -> dict:
        """``kind`` 'train_epoch' or 'validation': copy the block to the host (synchronises), combine the ranks, write the record
        (rank 0) and reset.  Returns the record with non-finite values as floats."""
        which = 'train' if kind == 'train_epoch' else 'validation'
        host_blk = None if self._dev is None else self._blk[which].cpu()
        keys = sorted(set(self._slots[which]) | set(self._host[which]))
        per_key = {}
        for k in keys:
            slot = self._slots[which].get(k)
            dev = None if slot is None else host_blk[slot * _SLOT:(slot + 1) * _SLOT].tolist()
            per_key[k] = combine_key(dev, self._host[which].get(k), *self._seen[which].get(k, (0, 0)))
        grads = []                          # (group key, [norm sum, norm max, maxabs max, nonfinite, steps])
        if which == 'train':
            for name, st in self._opts.items():
                lo = self.max_keys * _SLOT + st['index'] * 9 * _ACC
                rows = host_blk[lo:lo + (len(st['names']) + 1) * _ACC].view(-1, _ACC).tolist()
                labelled = list(zip(st['names'], rows)) + ([('all', rows[-1])] if len(st['names']) > 1 else [])
                grads += [(g, r) for g, r in labelled]
        # the ranks: sums add, extremes combine by max (min as the max of the negation); every rank logs the same keys
        sums = [v for k in keys for v in (per_key[k][0], per_key[k][1], per_key[k][5], per_key[k][6])]
        sums += [v for _, r in grads for v in (r[0], r[3], r[4])]
        maxes = [v for k in keys for v in (per_key[k][4], -per_key[k][3])] + [v for _, r in grads for v in (r[1], r[2])]
        sums, maxes = reduce_ranks(sums, maxes, self._dev)
        rec = {'event': kind, 'epoch': int(epoch), 'global_step': int(global_step)}
        stats, nonfinite = {}, 0.0
        for i, k in enumerate(keys):
            s, w, nf, _calls = sums[4 * i:4 * i + 4]
            rec[k] = s / w if w else math.nan
            stats[k] = {'last': per_key[k][2], 'min': -maxes[2 * i + 1], 'max': maxes[2 * i], 'wsum': w, 'nonfinite': nf}
            nonfinite += nf
        base_s, base_m = 4 * len(keys), 2 * len(keys)
        for j, (g, _) in enumerate(grads):
            nsum, nf, steps = sums[base_s + 3 * j:base_s + 3 * j + 3]
            if steps:
                rec[f'grad/{g}/norm_mean'] = nsum / steps
                rec[f'grad/{g}/norm_max'] = maxes[base_m + 2 * j]
                rec[f'grad/{g}/maxabs'] = maxes[base_m + 2 * j + 1]
                rec[f'grad/{g}/nonfinite'] = nf
        for k, v in (extras or {}).items():
            rec[k] = float(v)
        rec['nonfinite_values'] = nonfinite
        rec['stats'] = stats
        self._write(rec)
        self.flush()
        self._reset(which)
        return rec

    def _reset(self, which):
        if self._dev is not None:
            self._blk[which].copy_(self._init[which], non_blocking=True)
        self._host[which] = {}
        self._seen[which] = {}
        if which == 'train':
            for st in self._opts.values():
                st['calls'] = 0

    # ------------------------------------------------------------------ MiniTrainer._snapshot / _restore
    def snapshot(self):
        return dict(blk={k: v.clone() for k, v in self._blk.items()}, host=copy.deepcopy(self._host), seen=copy.deepcopy(self._seen),
                    slots=copy.deepcopy(self._slots), seq=self._seq, calls={n: st['calls'] for n, st in self._opts.items()})

    def restore(self, snap) -> None:
        for k, v in snap['blk'].items():
            self._blk[k].copy_(v)
        for k in self._blk:
            if k not in snap['blk']:                       # allocated after the snapshot: back to empty
                self._blk[k].copy_(self._init[k])
        self._host, self._seen = copy.deepcopy(snap['host']), copy.deepcopy(snap['seen'])
        self._slots, self._seq = copy.deepcopy(snap['slots']), snap['seq']
        for n, st in self._opts.items():
            st['calls'] = snap['calls'].get(n, 0)

    # ------------------------------------------------------------------ the file
    @property
    def path(self):
        return None if self.log_dir is None else os.path.join(self.log_dir, 'metrics.jsonl')

    def _write(self, rec: dict) -> None:
        if self.rank != 0 or self.log_dir is None:
            return
        if self._file is None:
            os.makedirs(self.log_dir, exist_ok=True)
            self._file = open(self.path, 'a', buffering=1, encoding='utf-8')       # line-buffered: a line is on its way once written
        self._file.write(json.dumps({k: _json_value(v) for k, v in rec.items()}, allow_nan=False) + '\n')

    def flush(self) -> None:
        if self._file is not None:
            self._file.flush()

    def close(self) -> None:
        if self._file is not None:
            self._file.close()
            self._file = None
