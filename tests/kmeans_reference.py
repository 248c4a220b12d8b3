"""Float64 reference of the k-means codebook initialisation (include/vqk.h, "k-means codebook initialisation"; no GPU):

    pick 0 = min(floor(u[0] N), N - 1);   pick j: mind[i] = min(mind[i], |x[i] - x[pick j-1]|^2), S = sum mind, P = cumsum(mind),
    the smallest i with P[i] > u[j] S;  none: the largest i with mind[i] > 0;  S == 0: min(floor(u[j] N), N - 1).

``seed64`` runs free (its own picks); ``seed_step64`` is ONE teacher-forced step on a given ``mind_in`` and centre row; ``lloyd64`` is a
Lloyd step on GIVEN indices.  ``make_case`` / the shape lists are the inputs of tests/test_gpu_kmeans.py, shared with
tests/test_kmeans_cpu.py; cases are cached and must not be modified."""
import functools

import numpy as np
import torch

KINDS = ['gauss', 'blobs', 'duplicates']
BLOB_SIZES = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 100, 120, 130, 140, 150, 129]       # sum = 1000
# (N, D, K) of the seeding tests: one row; one lane per row; a D that leaves lanes of a row's group idle; a block boundary of the
# 4-wave block (257 = 4 * 64 + 1); several blocks with a ragged tail
SEED_SHAPES = [(1, 256, 1), (63, 4, 8), (130, 12, 8), (257, 64, 33), (4099, 256, 33)]
# (N, K, D) of the Lloyd step: a ragged block on the filtered path; the generic path; many codes
LLOYD_SHAPES = [(67, 32, 256), (1000, 16, 64), (2051, 1024, 256)]
DATA_SEED, U_SEED = 0, 100        # tests/test_kmeans_cpu.py checks that this pair seeds one row in each of the 16 blobs


def draws(k: int, seed: int = U_SEED) -> torch.Tensor:
    return torch.rand(k, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def make_case(n: int, d: int, kind: str, seed: int = DATA_SEED):
    """x [N, D] fp32 (and, for 'blobs', the blob number of every row; else None).
    gauss: standard normal rows.  blobs: 16 centres 10 randn, rows = centre + 0.1 randn, blob sizes BLOB_SIZES at N = 1000 (equal sizes at any other
    N), rows shuffled.  duplicates: N rows that are copies of 5 distinct rows."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'gauss':
        return torch.randn(n, d, generator=g, dtype=torch.float32), None
    if kind == 'blobs':
        centres = 10.0 * torch.randn(len(BLOB_SIZES), d, generator=g, dtype=torch.float32)
        if n == sum(BLOB_SIZES):
            label = torch.repeat_interleave(torch.arange(len(BLOB_SIZES)), torch.tensor(BLOB_SIZES))
        else:                                                         # (any other N: blobs of equal size)
            label = torch.arange(n) % len(BLOB_SIZES)
        x = centres[label] + 0.1 * torch.randn(n, d, generator=g, dtype=torch.float32)
        perm = torch.randperm(n, generator=g)
        return x[perm].contiguous(), label[perm].contiguous()
    if kind == 'duplicates':
        base = torch.randn(5, d, generator=g, dtype=torch.float32)
        which = torch.randint(0, 5, (n,), generator=g)
        which[:min(n, 5)] = torch.arange(min(n, 5))                   # (every distinct row is present when N >= 5)
        return base[which].contiguous(), None
    raise ValueError(kind)


def uniform_pick(u: float, n: int) -> int:
    return min(int(np.floor(u * n)), n - 1)


def sqdist64(x: torch.Tensor, row: int) -> np.ndarray:
    """float64 squared distances of the (fp32) rows of x to x[row], by differences"""
    x64 = x.double().numpy()
    diff = x64 - x64[row][None, :]
    return (diff * diff).sum(1)


def pick_from(mind: np.ndarray, u: float):
    """the rule on a given float64 mind: (pick, S)"""
    n = mind.shape[0]
    prefix = np.cumsum(mind)                                          # sequential, row order
    s = float(prefix[-1])
    if s == 0.0:
        return uniform_pick(u, n), s
    t = u * s
    over = np.nonzero(prefix > t)[0]
    if over.size:
        return int(over[0]), s
    return int(np.nonzero(mind > 0)[0][-1]), s


def seed_step64(x: torch.Tensor, mind_in: np.ndarray, centre_row: int, u_j: float):
    """ONE teacher-forced step j >= 1: (mind_out float64, pick, S)"""
    mind = np.minimum(mind_in.astype(np.float64), sqdist64(x, centre_row))
    pick, s = pick_from(mind, u_j)
    return mind, pick, s


def seed64(x: torch.Tensor, k: int, u: torch.Tensor):
    """free-running float64 seeding: (picks [k] int64, total [k] float64 with total[0] = inf)"""
    n = x.shape[0]
    u = u.numpy()
    picks = np.empty(k, dtype=np.int64)
    total = np.empty(k, dtype=np.float64)
    picks[0], total[0] = uniform_pick(float(u[0]), n), np.inf
    mind = np.full(n, np.inf)
    for j in range(1, k):
        mind, picks[j], total[j] = seed_step64(x, mind, int(picks[j - 1]), float(u[j]))
    return picks, total


def lloyd64(x: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor):
    """Lloyd step on GIVEN indices: (counts [K] int64, new centres [K, D] float64 -- the mean of the rows of a non-empty cluster, the old
    centre of an empty one --, sum of |x| per cluster and component [K, D] float64, moved [K] float64 for the float64 means)"""
    k, d = centres.shape
    counts = torch.bincount(idx, minlength=k)
    sums = torch.zeros(k, d, dtype=torch.float64).index_add_(0, idx, x.double())
    mags = torch.zeros(k, d, dtype=torch.float64).index_add_(0, idx, x.double().abs())
    new = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None].double(), centres.double())
    moved = ((new - centres.double()) ** 2).sum(1)
    return counts, new, mags, moved


def centre_bound(mags: torch.Tensor, centre: torch.Tensor) -> torch.Tensor:
    """per component: n_k 2^-24 sum|x| / n_k (the fp32 summation bound of tests/test_gpu_ema_ordered.py, divided by the count) plus
    2^-24 |c| (the division's rounding)"""
    return 2.0 ** -24 * mags + 2.0 ** -24 * centre.abs()
