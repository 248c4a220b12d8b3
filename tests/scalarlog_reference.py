"""float64 restatement of the two kernels of csrc/runstats.hip and of the epoch / cross-rank reduction of scalarlog.py, in plain
Python and numpy: what the GPU tests compare against.

  * ``scalar_accum``: a slot is (sum, wsum, last, min, max, nonfinite, calls); one value x with weight w does
    sum += float64(x) * w, wsum += w, last = x, min / max skip NaN, nonfinite counts NaN / +-Inf.  Values arrive in call order, so
    ``sum`` is the left-to-right float64 sum -- the kernel's products are exact, its result must have the same bits.
  * ``arena_stats``: x = float64(g) * float64(scale) per element of a group; sumsq = the sum of the float64 squares of the
    finite x (``math.fsum``: the correctly rounded sum, up to 2^20 elements; numpy's pairwise float64 sum above, whose own error
    of about log2(n) 2^-53 is far inside the bound the tests use), maxabs = max |x| over the finite x, nonfinite = the count of
    the others.  Elements of segments with group -1 (the alignment padding) are in no result.  Row G = all groups together.
  * ``epoch_record``: ranks combine by adding sums / weights / counts and by max / min of the extremes; the mean is the sum of
    sums over the sum of weights; ``last`` is rank 0's.
"""
import math

import numpy as np

FSUM_MAX = 1 << 20


def new_slot():
    return [0.0, 0.0, math.nan, math.inf, -math.inf, 0.0, 0.0]


def scalar_accum(slot, x, w):
    """x: a Python float holding the fp32 / bf16 value exactly"""
    x = float(x)
    slot[0] += x * float(w)
    slot[1] += float(w)
    slot[2] = x
    if x < slot[3]:
        slot[3] = x
    if x > slot[4]:
        slot[4] = x
    if not math.isfinite(x):
        slot[5] += 1.0
    slot[6] += 1.0
    return slot


def sum_squares(x64):
    sq = x64 * x64                                                   # float64, one rounding per square
    return math.fsum(sq.tolist()) if sq.size <= FSUM_MAX else float(np.sum(sq))


def arena_stats(g, seg_end, seg_group, ngroups, scale):
    """g: float32 array; returns (out [ngroups + 1][3] as lists, n [ngroups + 1] = finite elements per row)"""
    g = np.asarray(g, dtype=np.float32)
    x = g.astype(np.float64) * np.float64(np.float32(scale))
    pieces = [[] for _ in range(ngroups)]
    lo = 0
    for end, grp in zip(seg_end, seg_group):
        if grp >= 0:
            pieces[grp].append(x[lo:end])
        lo = end
    out, counts = [], []
    allx = []
    for q in range(ngroups):
        v = np.concatenate(pieces[q]) if pieces[q] else np.zeros(0)
        allx.append(v)
        fin = v[np.isfinite(v)]
        out.append([sum_squares(fin), float(np.max(np.abs(fin))) if fin.size else 0.0, float(v.size - fin.size)])
        counts.append(int(fin.size))
    v = np.concatenate(allx) if allx else np.zeros(0)
    fin = v[np.isfinite(v)]
    out.append([sum_squares(fin), float(np.max(np.abs(fin))) if fin.size else 0.0, float(v.size - fin.size)])
    counts.append(int(fin.size))
    return out, counts


def sumsq_bound(n):
    """relative error bound of ANY order of n float64 additions of non-negative, exactly represented terms against their
    correctly rounded sum: n * 2^-53 (no constant from the implementation; an fp32 accumulation is outside it)"""
    return max(n, 1) * 2.0 ** -53


def norm_bound(n):
    return 0.5 * sumsq_bound(n) + 2.0 ** -52


def fold_arena(acc, out):
    """epoch accumulators [G + 1][5] = (sum of norms, max norm, max maxabs, sum of nonfinite, steps) += one step's out"""
    for row, (sumsq, maxabs, nonfinite) in zip(acc, out):
        norm = math.sqrt(sumsq)
        row[0] += norm
        row[1] = max(row[1], norm)
        row[2] = max(row[2], maxabs)
        row[3] += nonfinite
        row[4] += 1.0
    return acc


def epoch_record(per_rank_slots):
    """per_rank_slots: one {key: slot} per rank (every rank logs the same keys) -> {key: dict(mean, last, min, max, wsum,
    nonfinite)} as ScalarLog.epoch_end reports it"""
    rec = {}
    for key in sorted(per_rank_slots[0]):
        s = w = nf = 0.0
        mn, mx = math.inf, -math.inf
        for slots in per_rank_slots:                                 # rank order
            slot = slots[key]
            s += slot[0]
            w += slot[1]
            nf += slot[5]
            mn, mx = min(mn, slot[3]), max(mx, slot[4])
        rec[key] = dict(mean=s / w if w else math.nan, last=per_rank_slots[0][key][2], min=mn, max=mx, wsum=w, nonfinite=nf)
    return rec
