"""``ImageWriter``: reconstruction grids and images out of the step as PNG files -- the device half of what the reference logs
through ``wandb.Image(make_grid(...))`` (vqvae/model.py:442-456), without wandb.

The counterpart of ``data.DeviceImageLoader``, in the other direction and with the same rules.  The consuming thread (the one
that trains) makes every HIP call: it launches the egress kernel (``ops.image_grid_u8`` / ``ops.egress_u8``: one pass, uint8 HWC
straight from the padded NHWC tensors of the step) on a SIDE stream that waits on the current stream, and copies the bytes to
one of ``SLOTS`` rotating pinned buffers; an event marks the copy.  The training stream is never synchronised: it only waits (on
the device) for the egress kernel's read of the source tensors, so a hipGraph replay may overwrite its static tensors right
after.  Host threads encode the PNGs with PIL from the pinned bytes and write each file under a temporary name, then rename it;
they never touch the device.  A turn's bytes are handed to them by a later call (or ``flush``) of the consuming thread, once its
event has completed.  Buffers are made and grown inside the writer's own calls only, so a graph capture never meets a writer
thread or an allocation of the writer's.  Only rank 0 writes; on the other ranks every call returns at once.
"""
from __future__ import annotations

import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops

SLOTS = 3
MAX_ENCODE_THREADS = 16


def save_png(array, path: str) -> None:
    """uint8 [H,W,3] -> ``path`` (PNG), written under a temporary name and renamed: a reader never sees half a file"""
    from PIL import Image
    array = np.asarray(array)
    if array.dtype != np.uint8 or array.ndim != 3 or array.shape[2] != 3:
        raise ValueError(f'vqk: save_png expects uint8 [H,W,3], got {array.dtype} {array.shape}')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f'{path}.tmp.{os.getpid()}.{threading.get_ident()}'
    try:
        Image.fromarray(array).save(tmp, format='PNG')
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _is_rank0() -> bool:
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


class ImageWriter:
    """PNG files under ``directory`` from device tensors.  ``workers`` encode threads (at most 16).  ``write_grid`` /
    ``write_images`` return as soon as the kernel and the copy are queued; ``flush`` waits for every pending file, ``close``
    flushes and stops the threads.  Relative names are taken under ``directory``."""

    def __init__(self, directory: str, workers: int = 2, enabled: bool | None = None):
        self.directory = str(directory)
        self.workers = max(1, min(int(workers), MAX_ENCODE_THREADS))
        self.enabled = enabled                      # None: decided at the first call (rank 0 of the process group, if any)
        self._pool = None
        self._dev = None                            # device-side state, made at the first device call
        self._turn = 0
        self._futures = []                          # files handed to the pool and not yet checked
        self.files_written = 0

    # ---- host half -----------------------------------------------------------------------------------------------------
    def _path(self, name: str) -> str:
        return name if os.path.isabs(name) else os.path.join(self.directory, name)

    def _submit(self, array, path: str):
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix='vqk-encode')
        return self._pool.submit(save_png, array, path)

    def write_array(self, name: str, array) -> None:
        """a host uint8 [H,W,3] array (copied) through the same encode threads"""
        if self._on():
            self._futures.append(self._submit(np.array(array, dtype=np.uint8, copy=True), self._path(name)))

    def _on(self) -> bool:
        if self.enabled is None:
            self.enabled = _is_rank0()
        return self.enabled

    def _reap(self, futures) -> None:
        for f in futures:
            f.result()                              # an encode / write error surfaces in the consuming thread
            self.files_written += 1

    # ---- device half ---------------------------------------------------------------------------------------------------
    def _slot(self, device, nbytes: int):
        """the next rotating slot, idle (its last turn's files are on disk) and large enough"""
        if self._dev is None or self._dev['device'] != device:
            if self._dev is not None:
                self.flush()
            side = torch.cuda.Stream(device)
            self._dev = dict(device=device, side=side,
                             slots=[dict(dev=None, host=None, copied=torch.cuda.Event(), read=torch.cuda.Event(), pending=None,
                                         futures=[]) for _ in range(SLOTS)])
        sl = self._dev['slots'][self._turn % SLOTS]
        self._turn += 1
        self._hand_over(sl, wait=True)
        self._reap(sl['futures'])                   # the encoders of three turns ago still read this slot's pinned bytes
        sl['futures'] = []
        if sl['dev'] is None or sl['dev'].numel() < nbytes:         # grow: here, in the consuming thread, never during a capture
            side = self._dev['side']
            side.synchronize()
            size = nbytes + nbytes // 4
            with torch.cuda.stream(side):
                sl['dev'] = torch.empty(size, dtype=torch.uint8, device=device)
            sl['host'] = torch.empty(size, dtype=torch.uint8).pin_memory()
        return sl

    def _hand_over(self, sl, wait: bool) -> None:
        """a slot whose copy has completed goes to the encode threads"""
        if sl['pending'] is None:
            return
        if wait:
            sl['copied'].synchronize()              # the side stream's event: the training stream is not waited for by name
        elif not sl['copied'].query():
            return
        views, _keep = sl['pending']
        sl['pending'] = None                        # (_keep: the source tensors, alive until the kernel has read them)
        for path, off, shape in views:
            n = int(np.prod(shape))
            sl['futures'].append(self._submit(sl['host'].numpy()[off:off + n].reshape(shape), path))

    def _poll(self) -> None:
        if self._dev is not None:
            for sl in self._dev['slots']:
                self._hand_over(sl, wait=False)

    def _run(self, device, nbytes: int, sources, launch, views) -> None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('vqk: ImageWriter must not be called inside a graph capture (it copies to the host)')
        self._poll()
        sl = self._slot(device, nbytes)
        cur, side = torch.cuda.current_stream(device), self._dev['side']
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            launch(sl['dev'][:nbytes])
            sl['read'].record(side)
            sl['host'][:nbytes].copy_(sl['dev'][:nbytes], non_blocking=True)
            sl['copied'].record(side)
        cur.wait_event(sl['read'])                  # on the device: whatever overwrites the sources next comes after the kernel
        sl['pending'] = (views, list(sources))

    def write_grid(self, name: str, sources, nrow: int, padding: int = 2, pad_value: int = 0, value_ranges='sym') -> None:
        """one PNG: ``ops.image_grid_u8(sources, nrow, padding, pad_value, value_ranges)``"""
        if not self._on():
            return
        sources = list(sources)
        h, w = sources[0].shape[2:]
        _, _, hg, wg = ops.image_grid_shape(sum(int(s.shape[0]) for s in sources), h, w, nrow, int(padding))
        shape = (hg, wg, 3)
        self._run(sources[0].device, hg * wg * 3, sources,
                  lambda buf: ops.image_grid_u8(sources, nrow, padding, pad_value, value_ranges, out=buf.view(shape)),
                  [(self._path(name), 0, shape)])

    def write_images(self, names, src, value_range='sym') -> None:
        """one PNG per image of ``src`` (``ops.egress_u8``: no padding); ``names``: one file name per image"""
        if not self._on():
            return
        names = list(names)
        n, _, h, w = src.shape
        if len(names) != n:
            raise ValueError(f'vqk: {len(names)} names for {n} images')
        shape = (n, h, w, 3)
        self._run(src.device, n * h * w * 3, [src], lambda buf: ops.egress_u8(src, value_range, out=buf.view(shape)),
                  [(self._path(nm), k * h * w * 3, (h, w, 3)) for k, nm in enumerate(names)])

    # ---- completion ----------------------------------------------------------------------------------------------------
    def flush(self) -> None:
        """every file asked for so far is on disk when this returns (waits for the side stream's copies, not for training)"""
        if self._dev is not None:
            for sl in self._dev['slots']:
                self._hand_over(sl, wait=True)
            for sl in self._dev['slots']:
                self._reap(sl['futures'])
                sl['futures'] = []
        futures, self._futures = self._futures, []
        self._reap(futures)

    def close(self) -> None:
        try:
            self.flush()
        finally:
            if self._pool is not None:
                self._pool.shutdown(wait=True)
                self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unique_stems(paths) -> list:
    """file stems of ``paths``; a stem that occurs more than once (``a/x.png`` and ``b/x.jpg``) gets its index appended"""
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    seen = {}
    for s in stems:
        seen[s] = seen.get(s, 0) + 1
    return [s if seen[s] == 1 else f'{s}_{i:06d}' for i, s in enumerate(stems)]


class ReconstructionSaver:
    """``VQVAE.reconstruction_sink`` of evaluate.py: every reconstruction of the test loop as one PNG (no padding), named by
    ``names_per_batch[batch_index]``, and -- ``grid_every`` = N -- the panel of ``log_reconstructions`` (ground truths over
    reconstructions, at most 8 columns) as ``grids/batch=BBBBBB.png`` for every N-th batch.  Both tensors are in [0,1]."""

    def __init__(self, writer: ImageWriter, names_per_batch, grid_every: int | None = None):
        self.writer, self.names, self.grid_every = writer, list(names_per_batch), int(grid_every or 0)

    def __call__(self, batch_index: int, images, reconstructions) -> None:
        self.writer.write_images(self.names[batch_index], reconstructions, 'unit')
        if self.grid_every > 0 and batch_index % self.grid_every == 0:
            b = min(int(images.shape[0]), 8)
            self.writer.write_grid(f'grids/batch={batch_index:06d}.png', [images[:b], reconstructions[:b]], nrow=b,
                                   value_ranges='unit')

    def close(self) -> None:
        self.writer.close()
