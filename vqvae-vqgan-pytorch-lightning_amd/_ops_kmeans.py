"""k-means codebook initialisation over the vqk C-ABI (csrc/kmeans.hip): k-means++ seeding with every pick made on the device, and
Lloyd iterations composed of the launchers the quantizers already use -- ``vq_assign`` (the exact ranking, first minimum wins),
``ema_stats`` (per-cluster counts and sums) -- plus the centroid-update kernel.  Private part of :mod:`ops` like ``_ops_rvq.py``
(imported at the end of ``ops.py``, which re-exports every name); shared infrastructure is reached through ``core``.

Definition (include/vqk.h, "k-means codebook initialisation"): pick 0 is row floor(u[0] N); pick j draws row i with probability
mind[i] / sum(mind), mind[i] = the squared distance of row i to its nearest pick so far, by inverting the float64 running sum of mind
at u[j] sum(mind).  The draws ``u`` are an INPUT (float64 [K] in [0, 1)): the same ``u`` gives the same picks on every run."""
from __future__ import annotations

import torch

from . import _native
from . import ops as core
from ._ops_vq import ema_stats, vq_assign

KMEANS_SEED_ROWS = 64           # rows per block of the seeding step (csrc/kmeans.hip: KM_ROWS): N = multiples of it +- 1 are its edges
_KMEANS_WS: dict = {}               # _wkey() -> the block partial sums of the seeding step (core.grow_ws)


def _check_rows(x: torch.Tensor, what: str) -> None:
    core._require_gpu(x)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f'{what}: x must be a contiguous fp32 [N, D] tensor, got {x.dtype} {tuple(x.shape)}')


def _check_draws(u: torch.Tensor, k: int, device) -> torch.Tensor:
    if u.dtype != torch.float64 or u.dim() != 1 or u.shape[0] != k:
        raise ValueError(f'kmeans: u must be float64 [{k}], got {u.dtype} {tuple(u.shape)}')
    return u.to(device).contiguous()


def kmeans_seed_step(x: torch.Tensor, k: int, j: int, u: torch.Tensor, picks: torch.Tensor, mind: torch.Tensor,
                     total: torch.Tensor | None = None) -> None:
    """ONE pick (vqk_kmeans_seed_step_f32): reads picks[j - 1] and mind, writes mind, picks[j] and total[j], all on the device.
    x [N, D] fp32; u [k] float64, picks [k] int64, mind [N] fp32, total [k] float64 or None: device tensors the caller owns."""
    _check_rows(x, 'kmeans_seed_step')
    n, d = x.shape
    lib = _native.lib()
    nbytes = lib.vqk_kmeans_seed_ws_bytes(n)
    ws = core.grow_ws(_KMEANS_WS, x.device, max(int(nbytes), 16))
    _native.check(lib.vqk_kmeans_seed_step_f32(x.data_ptr(), n, d, k, j, u.data_ptr(), picks.data_ptr(), mind.data_ptr(), core._p(total),
                                               ws.data_ptr(), ws.numel(), core._stream()), 'kmeans_seed_step')


def kmeans_seed(x: torch.Tensor, k: int, u: torch.Tensor, return_total: bool = False, return_mind: bool = False):
    """k-means++ seeding: x [N, D] fp32 on the GPU, u [k] float64 draws -> picks [k] int64 (row numbers of x).  2 k - 1 launches on
    the current stream and no host synchronisation: the previous pick is read on the device.  ``return_total``: also total [k]
    float64, total[j] = sum(mind) that pick j was drawn from (total[0] = inf; 0 once every row coincides with a pick);
    ``return_mind``: also mind [N] fp32 after the last pick.  Returns picks, or a tuple in the order (picks, total, mind)."""
    _check_rows(x, 'kmeans_seed')
    n, d = x.shape
    k = int(k)
    if k < 1:
        raise ValueError(f'kmeans_seed: k must be >= 1, got {k}')
    if n < 1:
        raise ValueError('kmeans_seed: x holds no rows')
    u = _check_draws(u, k, x.device)
    picks = torch.empty(k, dtype=torch.int64, device=x.device)
    mind = torch.empty(n, dtype=torch.float32, device=x.device)
    total = torch.empty(k, dtype=torch.float64, device=x.device) if return_total else None
    lib = _native.lib()
    ws = core.grow_ws(_KMEANS_WS, x.device, max(int(lib.vqk_kmeans_seed_ws_bytes(n)), 16))
    st = core._stream()
    args = (u.data_ptr(), picks.data_ptr(), mind.data_ptr(), core._p(total), ws.data_ptr(), ws.numel(), st)
    fn, xp = lib.vqk_kmeans_seed_step_f32, x.data_ptr()
    for j in range(k):
        _native.check(fn(xp, n, d, k, j, *args), 'kmeans_seed_step')
    out = (picks,) + ((total,) if return_total else ()) + ((mind,) if return_mind else ())
    return out[0] if len(out) == 1 else out


def kmeans_lloyd_step(x: torch.Tensor, centres: torch.Tensor, return_aux: bool = False):
    """One Lloyd iteration, ``centres`` [K, D] fp32 updated IN PLACE: vq_assign(x, centres, 0) (exact ranking, first minimum wins;
    the filtered path where D == 256 and K % 32 == 0), ema_stats (counts and sums per cluster; the ordered form under
    ``set_deterministic(True)``), then centres[c] = sums[c] / counts[c] where counts[c] > 0 -- an empty cluster keeps its centre.
    Returns counts [K] fp32 (a view of the statistics buffer); ``return_aux``: (counts, idx [N] int64, moved [K] fp32 =
    |c_new - c_old|^2)."""
    _check_rows(x, 'kmeans_lloyd_step')
    if centres.dtype != torch.float32 or not centres.is_contiguous() or centres.dim() != 2 or centres.shape[1] != x.shape[1]:
        raise ValueError(f'kmeans_lloyd_step: centres must be a contiguous fp32 [K, {x.shape[1]}] tensor')
    k, d = centres.shape
    idx = vq_assign(x, centres, 0)
    buf = ema_stats(x, idx, k)
    moved = torch.empty(k, dtype=torch.float32, device=x.device)
    _native.check(_native.lib().vqk_kmeans_update_f32(buf.data_ptr(), buf[k:].data_ptr(), k, d, centres.data_ptr(), moved.data_ptr(),
                                                      core._stream()), 'kmeans_update')
    counts = buf[:k]
    return (counts, idx, moved) if return_aux else counts


def kmeans_fit(x: torch.Tensor, k: int, iters: int, u: torch.Tensor) -> dict:
    """k-means++ seeding followed by ``iters`` Lloyd iterations (0 = the seeds).  Returns dict(centres [K, D] fp32, counts [K] int64,
    picks [K] int64, inertia, used): counts, inertia = sum |x - centres[idx]|^2 and used = the share of non-empty clusters belong to
    the assignment of x to the FINAL centres, computed once after the last iteration (torch operations, device scalars).  Under
    ``set_deterministic(True)`` the per-cluster sums are added in row order, so the whole fit is bit-reproducible."""
    _check_rows(x, 'kmeans_fit')
    n, d = x.shape
    k, iters = int(k), int(iters)
    if n < k:
        raise ValueError(f'kmeans_fit: {n} rows cannot seed {k} centres (N < K)')
    if iters < 0:
        raise ValueError(f'kmeans_fit: iters must be >= 0, got {iters}')
    picks = kmeans_seed(x, k, u)
    centres = x.index_select(0, picks).contiguous()
    for _ in range(iters):
        kmeans_lloyd_step(x, centres)
    idx = vq_assign(x, centres, 0)
    counts = torch.bincount(idx, minlength=k)
    inertia = (x - centres.index_select(0, idx)).double().pow(2).sum()
    used = (counts > 0).double().mean()
    return dict(centres=centres, counts=counts, picks=picks, inertia=inertia, used=used)


__all__ = [_n for _n in dir() if not _n.startswith('__') and _n not in ('core', 'annotations', 'vq_assign', 'ema_stats')]
