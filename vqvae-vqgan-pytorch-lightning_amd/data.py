"""Image-folder data loading: the reference's ``data/datasets.py::ImageDataset`` + ``data/datamodules.py::ImageDataModule``
with the per-image work moved to the device.

The reference decodes with PIL and runs ``ToTensor()`` + ``Resize((S, S), antialias=True)`` per image in forked DataLoader
workers (its ``ImageDataset`` cannot be imported here: it needs torchvision, which this project does not depend on).  Here

  * host threads only DECODE to uint8 and copy the bytes into one packed, pinned staging buffer (``HostPipeline``: no HIP call,
    usable and tested without a device);
  * the consuming thread uploads the packed bytes and runs ONE kernel for the whole ragged batch (``ops.ingest_u8``:
    ToTensor + crop + ATen's antialiased bilinear resize), on a side stream its own stream waits on (``DeviceImageLoader``).

Threads, not worker processes: PIL releases the GIL while decoding, no child ever inherits an initialised GPU runtime, and the
device sees one process per rank.  Every HIP call (allocation, copy, launch, event) is made by the thread that iterates, and
buffers grow only inside ``__next__``: a ``torch.cuda.graph`` capture on the consuming thread never meets an allocation or a
synchronisation from a loader thread.
"""
from __future__ import annotations

import os
import pathlib
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from . import ops

PATTERNS = ('*.png', '*.jpg', '*.bmp', '*.JPEG')
MAX_DECODE_THREADS = 16
SLOTS = 3                                   # staging / device buffers in rotation: one in use, two ahead


class ImageFolder:
    """The file list of the reference's ``ImageDataset`` (data/datasets.py:12-13): ONE sorted list of every path under ``folder``
    (recursively) matching ``*.png``, ``*.jpg``, ``*.bmp`` or ``*.JPEG``.  The patterns are CASE-SENSITIVE, as there: ``a.PNG``,
    ``b.jpeg`` and ``c.gif`` are not part of the dataset.  Paths sort as ``pathlib`` paths (component by component).
    ``load(i)`` is ``Image.open(path).convert('RGB')`` as a uint8 [h, w, 3] array (greyscale, palette and RGBA sources come out
    as 3 channels)."""

    def __init__(self, folder: str):
        root = pathlib.Path(folder)
        if not root.is_dir():
            raise FileNotFoundError(f'image folder {folder} does not exist')
        self.folder = str(folder)
        self.samples = sorted(p for pattern in PATTERNS for p in root.rglob(pattern))

    def __len__(self) -> int:
        return len(self.samples)

    def path(self, idx: int) -> str:
        return self.samples[idx].absolute().as_posix()

    def open(self, idx: int):
        """the opened (header read, not yet decoded) PIL image: its ``size`` is known without decoding"""
        return Image.open(self.path(idx))

    def load(self, idx: int) -> np.ndarray:
        with self.open(idx) as im:
            return np.asarray(im.convert('RGB'))


def epoch_indices(n: int, shuffle: bool, seed: int, epoch: int, rank: int = 0, world: int = 1) -> list:
    """This rank's share of one epoch.  Every rank draws the SAME order -- ``randperm(n)`` seeded with ``seed + epoch`` when
    ``shuffle``, else 0..n-1 -- keeps its first ``(n // world) * world`` entries and takes every ``world``-th of them from
    ``rank`` on: shares are disjoint, equally long on every rank, and their union is that prefix."""
    if not 0 <= rank < world:
        raise ValueError(f'rank {rank} outside world {world}')
    if shuffle:
        order = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) + int(epoch))).tolist()
    else:
        order = list(range(n))
    return order[rank:(n // world) * world:world]


def batch_indices(share: list, batch_size: int, drop_last: bool) -> list:
    """``share`` cut into batches; the short last one is dropped (train) or kept (validation / test)"""
    out = [share[i:i + batch_size] for i in range(0, len(share), batch_size)]
    if drop_last and out and len(out[-1]) < batch_size:
        out.pop()
    return out


class HostBatch:
    """one decoded batch on the host: ``desc`` (``ops.INGEST_DESC`` table), ``buf`` (uint8 numpy view holding ``nbytes`` packed
    bytes), ``slot`` (which staging buffer ``buf`` is, or -1 when the batch outgrew it and ``buf`` is a private array)"""
    __slots__ = ('indices', 'desc', 'buf', 'nbytes', 'slot')

    def __init__(self, indices, desc, buf, nbytes, slot):
        self.indices, self.desc, self.buf, self.nbytes, self.slot = indices, desc, buf, nbytes, slot


class HostPipeline:
    """The host half of the loader: decodes the batches of ``batches`` (lists of dataset indices), in order, ``SLOTS`` ahead at
    most, into rotating staging buffers.  ``buffers``: ``SLOTS`` 1-D uint8 numpy arrays the caller owns (views of pinned memory
    in ``DeviceImageLoader``; plain arrays work); a batch that does not fit its buffer is returned in a private array with
    ``slot == -1`` and the caller may swap a larger buffer in with ``replace``.  A coordinator thread reads the headers (sizes),
    lays the batch out (``ops.ingest_desc``) and hands one decode-and-copy task per image to the pool; nothing here touches
    the device.  Iterate, and ``release`` a batch's slot once its bytes have been consumed."""

    def __init__(self, folder: ImageFolder, batches: list, pool: ThreadPoolExecutor, mode: str, buffers: list):
        self.folder, self.batches, self.pool, self.mode, self.buffers = folder, batches, pool, mode, buffers
        self._free: queue.Queue = queue.Queue()
        for s in range(len(buffers)):
            self._free.put(s)
        self._ready: queue.Queue = queue.Queue()
        self._stop = threading.Event()
        self._taken = 0
        self._thread = threading.Thread(target=self._run, name='vqk-loader', daemon=True)
        self._thread.start()

    def _decode_into(self, im, entry, buf) -> None:
        with im:
            ops.pack_images([np.asarray(im.convert('RGB'))], entry, buf)

    def _run(self) -> None:
        try:
            for indices in self.batches:
                slot = None
                while slot is None:
                    if self._stop.is_set():
                        return
                    try:
                        slot = self._free.get(timeout=0.05)
                    except queue.Empty:
                        pass
                images = [self.folder.open(i) for i in indices]
                desc = ops.ingest_desc([(im.size[1], im.size[0]) for im in images], self.mode)
                nbytes = ops.ingest_packed_bytes(desc)
                buf = self.buffers[slot]
                if nbytes > buf.shape[0]:
                    self._free.put(slot)
                    buf, slot = np.empty(nbytes, dtype=np.uint8), -1
                futures = [self.pool.submit(self._decode_into, im, desc[k:k + 1], buf) for k, im in enumerate(images)]
                for f in futures:
                    f.result()
                self._ready.put(HostBatch(indices, desc, buf, nbytes, slot))
        except BaseException as exc:                                   # a broken file surfaces in the consuming thread
            self._ready.put(exc)

    def __iter__(self):
        return self

    def __next__(self) -> HostBatch:
        if self._taken == len(self.batches):
            raise StopIteration
        item = self._ready.get()
        if isinstance(item, BaseException):
            self.close()
            raise item
        self._taken += 1
        return item

    def release(self, slot: int) -> None:
        if slot >= 0:
            self._free.put(slot)

    def replace(self, slot: int, buf) -> None:
        """swap a (larger) staging buffer in; only for a slot the coordinator does not hold (a free one)"""
        self.buffers[slot] = buf

    def close(self) -> None:
        self._stop.set()
        self._thread.join()


class DeviceImageLoader:
    """Batches of a folder of images as device fp32 ``[b, 3, S, S]`` in [0,1] -- what ``training_step`` / ``validation_step`` /
    ``test_step`` take.  Iterable and re-iterable: one pass is one epoch; ``set_epoch(e)`` reseeds the shuffle with ``seed + e``.
    Every rank draws the same permutation and takes a disjoint strided share (``epoch_indices``), so ``len()`` is equal on all
    ranks.  ``resize``: 'squash' (the whole image to S x S: the reference's standard loader) or 'center_crop'.
    ``workers`` decode threads (at most 16).  A yielded batch is a view of a rotating buffer: it is valid until the NEXT batch
    is asked for (clone it to keep it).  The device is touched at the first iteration, not at construction."""

    def __init__(self, folder, image_size: int, batch_size: int, workers: int = 1, device=None, shuffle: bool = False,
                 drop_last: bool = False, seed: int = 0, rank: int = 0, world: int = 1, resize: str = 'squash',
                 staging_bytes: int | None = None):
        self.folder = folder if isinstance(folder, ImageFolder) else ImageFolder(folder)
        if resize not in ('squash', 'center_crop'):
            raise ValueError("resize: 'squash' or 'center_crop'")
        if batch_size < 1 or image_size < 1:
            raise ValueError('batch_size and image_size must be >= 1')
        self.image_size, self.batch_size, self.resize = int(image_size), int(batch_size), resize
        self.workers = max(1, min(int(workers), MAX_DECODE_THREADS))
        self.device = torch.device(device) if device is not None else None
        self.shuffle, self.drop_last, self.seed, self.rank, self.world = shuffle, drop_last, int(seed), int(rank), int(world)
        self.epoch = 0
        self.staging_bytes = int(staging_bytes) if staging_bytes else self.batch_size * 3 * 512 * 512
        self._pool = None
        self._pipe = None
        self._dev = None                    # device-side state, made at the first iteration

    # ---- order ---------------------------------------------------------------------------------------------------------
    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def epoch_batches(self, epoch: int | None = None) -> list:
        """this rank's batches (lists of dataset indices) of ``epoch`` (default: the current one)"""
        share = epoch_indices(len(self.folder), self.shuffle, self.seed, self.epoch if epoch is None else epoch, self.rank, self.world)
        return batch_indices(share, self.batch_size, self.drop_last)

    def __len__(self) -> int:
        per_rank = len(self.folder) // self.world
        return per_rank // self.batch_size if self.drop_last else -(-per_rank // self.batch_size)

    # ---- host half -----------------------------------------------------------------------------------------------------
    def host_pipeline(self, buffers: list | None = None, epoch: int | None = None) -> HostPipeline:
        """the decode-and-pack half over this loader's order; without ``buffers`` it stages into plain numpy arrays"""
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix='vqk-decode')
        if buffers is None:
            buffers = [np.empty(self.staging_bytes, dtype=np.uint8) for _ in range(SLOTS)]
        return HostPipeline(self.folder, self.epoch_batches(epoch), self._pool, self.resize, buffers)

    # ---- device half ---------------------------------------------------------------------------------------------------
    def _setup_device(self) -> None:
        if self.device is None or self.device.type != 'cuda':
            raise RuntimeError('vqk: DeviceImageLoader yields device tensors made by a HIP kernel (no CPU fallback); '
                               f'got device {self.device}')
        b, s, dl = self.batch_size, self.image_size, ops.INGEST_DESC.itemsize
        side = torch.cuda.Stream(self.device)
        host = [torch.empty(self.staging_bytes, dtype=torch.uint8).pin_memory() for _ in range(SLOTS)]
        slots = []
        with torch.cuda.stream(side):                                   # owned by the side stream: every write to them is on it
            for _ in range(SLOTS):
                slots.append(dict(pixels=torch.empty(self.staging_bytes, dtype=torch.uint8, device=self.device),
                                  out=torch.empty(b, 3, s, s, dtype=torch.float32, device=self.device),
                                  desc_dev=torch.empty(b * dl, dtype=torch.uint8, device=self.device),
                                  desc_host=torch.empty(b * dl, dtype=torch.uint8).pin_memory(),
                                  copied=torch.cuda.Event(),            # the uploads of this turn have left the pinned memory
                                  ready=torch.cuda.Event(),             # the kernel has written `out`
                                  released=None))                       # the consumer is past its last use of `out`
        side.synchronize()
        self._dev = dict(side=side, host=host, slots=slots)

    def __iter__(self):
        if self._dev is None:
            self._setup_device()
        if self._pipe is not None:                                      # a pass that was left early: settle what it had in flight
            self._pipe.close()
            if self._pending is not None:
                self._pending[0].synchronize()
            if self._last is not None:
                self._last['released'] = torch.cuda.Event()
                self._last['released'].record(torch.cuda.current_stream(self.device))
        self._pipe = self.host_pipeline([h.numpy() for h in self._dev['host']])
        self._turn, self._pending, self._last = 0, None, None
        return self

    def __next__(self) -> torch.Tensor:
        if self._pipe is None:
            raise StopIteration
        cur = torch.cuda.current_stream(self.device)
        if self._last is not None:                                       # the consumer asked for more: it is done with the last batch
            ev = torch.cuda.Event()
            ev.record(cur)
            self._last['released'], self._last = ev, None
        if self._pending is not None:                                    # hand the previous batch's staging buffer back to the decoders
            copied, slot, _src = self._pending
            copied.synchronize()                                         # (issued a whole step ago)
            self._pipe.release(slot)
            self._pending = None
        try:
            hb = next(self._pipe)
        except StopIteration:
            self._pipe.close()
            self._pipe = None
            raise
        sl = self._dev['slots'][self._turn % SLOTS]
        self._turn += 1
        side = self._dev['side']
        n, dbytes = len(hb.desc), len(hb.desc) * ops.INGEST_DESC.itemsize
        if hb.nbytes > sl['pixels'].numel():                             # grow: here, in the consuming thread, never during a capture
            side.synchronize()
            with torch.cuda.stream(side):
                sl['pixels'] = torch.empty(hb.nbytes + hb.nbytes // 4, dtype=torch.uint8, device=self.device)
        src = torch.from_numpy(hb.buf[:hb.nbytes])                       # (a view of pinned memory when the batch sits in its slot)
        if hb.slot < 0:                                                  # the batch outgrew the staging buffers: pin a private copy
            src = src.pin_memory()
        sl['desc_host'][:dbytes].numpy()[:] = hb.desc.view(np.uint8)
        with torch.cuda.stream(side):
            if sl['released'] is not None:
                side.wait_event(sl['released'])                          # `out` of three batches ago may still be read
            pixels = sl['pixels'][:hb.nbytes]
            pixels.copy_(src, non_blocking=True)
            sl['desc_dev'][:dbytes].copy_(sl['desc_host'][:dbytes], non_blocking=True)
            sl['copied'].record(side)
            out = sl['out'][:n]
            ops.ingest_u8(pixels, hb.desc, self.image_size, out=out, desc_dev=sl['desc_dev'])
            sl['ready'].record(side)
        if hb.slot >= 0:
            self._pending = (sl['copied'], hb.slot, src)
        else:
            sl['copied'].synchronize()
            for k, h in enumerate(self._dev['host']):                    # the staging buffers catch up with the data (batches in
                if h.numel() < hb.nbytes:                                # flight keep the array they were decoded into)
                    self._dev['host'][k] = torch.empty(hb.nbytes + hb.nbytes // 4, dtype=torch.uint8).pin_memory()
                    self._pipe.replace(k, self._dev['host'][k].numpy())
        cur.wait_event(sl['ready'])
        self._last = sl
        return out

    def close(self) -> None:
        if self._pipe is not None:
            self._pipe.close()
            self._pipe = None
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DataModule:
    """the loaders of ``get_datamodule``: ``train`` / ``validation`` (mode 'train') or ``test``; an absent folder is ``None``"""

    def __init__(self, train=None, validation=None, test=None):
        self.train, self.validation, self.test = train, validation, test


def get_datamodule(dirpath: str, image_size: int, batch_size: int, workers: int, seed: int, rank: int = 0, world: int = 1,
                   mode: str = 'train', device=None, resize: str = 'squash') -> DataModule:
    """The reference's folder layout (vqvae/common_utils.py::get_datamodule, 'standard' loader): mode 'train' -> ``train/``
    (shuffled, last short batch dropped) and, when present, ``validation/`` (in order, short last batch kept); any other mode ->
    ``test/`` (in order, short last batch kept)."""
    def loader(sub, **kw):
        return DeviceImageLoader(os.path.join(dirpath, sub), image_size, batch_size, workers, device, seed=seed, rank=rank,
                                 world=world, resize=resize, **kw)
    if mode == 'train':
        val = loader('validation') if os.path.isdir(os.path.join(dirpath, 'validation')) else None
        return DataModule(train=loader('train', shuffle=True, drop_last=True), validation=val)
    return DataModule(test=loader('test'))
