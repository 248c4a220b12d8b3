"""The host half of the image-folder loader (data.py, the descriptor helpers of ops.py) and the entry points' command line, without
a device: file order and extension rule of the reference's ``ImageDataset`` (data/datasets.py:12-13), sharding, ``drop_last``,
descriptor tables, and the packed staging buffer against a plain re-read of every image."""
import importlib
import pathlib

import numpy as np
import pytest
from PIL import Image

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
data = importlib.import_module(PKG + '.data')
ops = importlib.import_module(PKG + '.ops')
train = importlib.import_module(PKG + '.train')
evaluate = importlib.import_module(PKG + '.evaluate')


def _rgb(rng, h, w):
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _write(path, arr, mode='RGB'):
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(arr, mode).save(path)


@pytest.fixture()
def folder(tmp_path):
    """names that interleave across the four extensions when sorted, nested folders, and files the rule leaves out"""
    rng = np.random.default_rng(0)
    kept = ['a.png', 'b.jpg', 'c.bmp', 'd.JPEG', 'e.png', 'sub/a.bmp', 'sub/deep/z.png', 'sub/b.png', 'sub-x/a.png', 'f.jpg']
    for k, name in enumerate(kept):
        _write(tmp_path / name, _rgb(rng, 5 + k, 9 - k % 4))
    _write(tmp_path / 'skip.gif', _rgb(rng, 4, 4)[:, :, 0], 'L')
    _write(tmp_path / 'skip.PNG', _rgb(rng, 4, 4))
    _write(tmp_path / 'sub' / 'skip.jpeg', _rgb(rng, 4, 4))
    (tmp_path / 'notes.txt').write_text('not an image')
    return tmp_path, kept


def test_file_list_is_the_references(folder):
    root, kept = folder
    ds = data.ImageFolder(str(root))
    want = sorted(list(pathlib.Path(root).rglob('*.png')) + list(pathlib.Path(root).rglob('*.jpg')) +
                  list(pathlib.Path(root).rglob('*.bmp')) + list(pathlib.Path(root).rglob('*.JPEG')))
    assert ds.samples == want and len(ds) == len(kept)
    rel = [p.relative_to(root).as_posix() for p in ds.samples]
    assert sorted(rel) == sorted(kept)
    assert rel[:6] == ['a.png', 'b.jpg', 'c.bmp', 'd.JPEG', 'e.png', 'f.jpg']                # ONE sorted list, not one per extension
    assert rel.index('sub/deep/z.png') > rel.index('sub/b.png') and rel.index('sub-x/a.png') > rel.index('sub/deep/z.png')
    assert not any('skip' in r for r in rel)
    assert ds.path(0) == (root / 'a.png').absolute().as_posix()


def test_missing_folder_raises(tmp_path):
    with pytest.raises(FileNotFoundError):
        data.ImageFolder(str(tmp_path / 'nope'))


def test_sources_come_out_as_three_channels(tmp_path):
    rng = np.random.default_rng(1)
    grey, rgba = _rgb(rng, 6, 7)[:, :, 0], np.concatenate([_rgb(rng, 5, 4), _rgb(rng, 5, 4)[:, :, :1]], axis=2)
    _write(tmp_path / 'g.png', grey, 'L')
    _write(tmp_path / 'r.png', rgba, 'RGBA')
    pal = Image.fromarray(_rgb(rng, 8, 8)).convert('P')
    pal.save(tmp_path / 'p.png')
    ds = data.ImageFolder(str(tmp_path))
    for i in range(len(ds)):
        a = ds.load(i)
        assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3
        assert np.array_equal(a, np.asarray(Image.open(ds.path(i)).convert('RGB')))
    assert np.array_equal(ds.load(0), np.repeat(grey[:, :, None], 3, axis=2))
    assert np.array_equal(ds.load(2), rgba[:, :, :3])


@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('shuffle', [False, True])
def test_shares_are_disjoint_equal_and_cover_the_prefix(world, shuffle):
    import torch
    n, seed = 23, 7
    for epoch in (0, 1):
        shares = [data.epoch_indices(n, shuffle, seed, epoch, r, world) for r in range(world)]
        assert len({len(s) for s in shares}) == 1 and len(shares[0]) == n // world
        flat = [i for s in shares for i in s]
        assert len(set(flat)) == len(flat)
        order = torch.randperm(n, generator=torch.Generator().manual_seed(seed + epoch)).tolist() if shuffle else list(range(n))
        assert sorted(flat) == sorted(order[:(n // world) * world])
        for r in range(world):
            assert shares[r] == order[r:(n // world) * world:world]
            assert shares[r] == data.epoch_indices(n, shuffle, seed, epoch, r, world)          # same (seed, epoch): same share
    if shuffle:
        assert data.epoch_indices(n, True, seed, 0, 0, world) != data.epoch_indices(n, True, seed, 1, 0, world)
        assert data.epoch_indices(n, True, seed, 1, 0, world) == data.epoch_indices(n, True, seed + 1, 0, 0, world)
    with pytest.raises(ValueError):
        data.epoch_indices(n, shuffle, seed, 0, world, world)


def _dataset(tmp_path, count, sub='', seed=2):
    rng = np.random.default_rng(seed)
    arrays = {}
    for k in range(count):
        name = f'{sub}img{k:03d}' + ('.png' if k % 2 else '.bmp')
        arrays[name] = _rgb(rng, 3 + (5 * k) % 11, 2 + (7 * k) % 13)
        _write(tmp_path / name, arrays[name])
    return arrays


@pytest.mark.parametrize('world', [1, 2, 3])
def test_loader_kinds_len_and_drop_last(tmp_path, world):
    _dataset(tmp_path, 14, 'train/')
    _dataset(tmp_path, 14, 'validation/')
    _dataset(tmp_path, 14, 'test/')
    for rank in range(world):
        dm = data.get_datamodule(str(tmp_path), 16, 4, 2, seed=3, rank=rank, world=world, mode='train')
        per_rank = 14 // world
        assert dm.test is None and dm.train.shuffle and dm.train.drop_last and not dm.validation.shuffle and not dm.validation.drop_last
        tb, vb = dm.train.epoch_batches(), dm.validation.epoch_batches()
        assert len(dm.train) == len(tb) == per_rank // 4 and all(len(b) == 4 for b in tb)
        assert len(dm.validation) == len(vb) == -(-per_rank // 4)
        assert [i for b in vb for i in b] == list(range(rank, per_rank * world, world))          # in order, short last batch kept
        assert len(vb[-1]) == (per_rank % 4 or 4)
        dm.train.set_epoch(1)
        assert dm.train.epoch_batches() == dm.train.epoch_batches(1) != tb
        te = data.get_datamodule(str(tmp_path), 16, 4, 2, seed=3, rank=rank, world=world, mode='test')
        assert te.train is None and te.validation is None and not te.test.shuffle and not te.test.drop_last
        assert len(te.test) == -(-per_rank // 4)
    (tmp_path / 'only').mkdir()
    _dataset(tmp_path / 'only', 3, 'train/')
    assert data.get_datamodule(str(tmp_path / 'only'), 16, 2, 1, seed=0).validation is None       # no validation/ folder


def test_workers_are_capped_at_16(tmp_path):
    _dataset(tmp_path, 2)
    assert data.DeviceImageLoader(str(tmp_path), 8, 2, workers=64).workers == 16
    assert data.DeviceImageLoader(str(tmp_path), 8, 2, workers=0).workers == 1


def test_descriptor_tables():
    sizes = [(375, 500), (7, 4099), (1, 1), (97, 31), (33, 33)]
    sq = ops.ingest_desc(sizes, 'squash')
    assert sq.dtype == ops.INGEST_DESC and sq.dtype.itemsize == 40 and len(sq) == len(sizes)
    for e, (h, w) in zip(sq, sizes):
        assert (e['h'], e['w'], e['stride'], e['x0'], e['y0'], e['bw'], e['bh'], e['flip']) == (h, w, 3 * w, 0, 0, w, h, 0)
    cc = ops.ingest_desc(sizes, 'center_crop')
    for e, (h, w) in zip(cc, sizes):
        m = min(h, w)
        assert e['bw'] == e['bh'] == m
        assert 0 <= e['x0'] and e['x0'] + m <= w and 0 <= e['y0'] and e['y0'] + m <= h              # odd sizes: the box stays inside
        assert abs((w - m - e['x0']) - e['x0']) <= 1 and abs((h - m - e['y0']) - e['y0']) <= 1      # centred
    boxes = [(40, 21, 301, 301), (4000, 0, 99, 7), (0, 0, 1, 1), (30, 96, 1, 1), (1, 2, 3, 4)]
    bx = ops.ingest_desc(sizes, 'boxes', boxes=boxes, flips=[1, 0, 0, 1, 0])
    assert [tuple(int(e[k]) for k in ('x0', 'y0', 'bw', 'bh')) for e in bx] == boxes
    assert list(bx['flip']) == [1, 0, 0, 1, 0]
    # offsets: images do not overlap, start on 16 bytes, and the buffer size covers the last byte
    ends = [int(e['offset']) + (int(e['h']) - 1) * int(e['stride']) + 3 * int(e['w']) for e in sq]
    assert all(int(e['offset']) % 16 == 0 for e in sq) and int(sq[0]['offset']) == 0
    assert all(int(sq[i + 1]['offset']) >= ends[i] for i in range(len(sq) - 1))
    assert ops.ingest_packed_bytes(sq) == max(ends)
    padded = ops.ingest_desc(sizes[:1], strides=[1504], offsets=[64])
    assert int(padded[0]['stride']) == 1504 and int(padded[0]['offset']) == 64
    for bad in ([(10, 10, 500, 1)], [(0, 0, 501, 375)], [(-1, 0, 5, 5)], [(0, 0, 0, 5)], [(0, 371, 5, 5)]):
        with pytest.raises(ValueError):
            ops.ingest_desc(sizes[:1], 'boxes', boxes=bad)
    with pytest.raises(ValueError):
        ops.ingest_desc([(16385, 4)])
    with pytest.raises(ValueError):
        ops.ingest_desc([(4, 0)])
    with pytest.raises(ValueError):
        ops.ingest_desc(sizes[:1], strides=[1499])
    with pytest.raises(ValueError):
        ops.ingest_desc(sizes, 'nearest')


def test_random_crop_boxes_stay_inside_and_are_seeded():
    import torch
    sizes = [(375, 500), (64, 48), (1, 1), (97, 31)] * 8
    boxes, flips = ops.random_crop_boxes(sizes, generator=torch.Generator().manual_seed(5))
    again = ops.random_crop_boxes(sizes, generator=torch.Generator().manual_seed(5))
    assert (boxes, flips) == again and set(flips) == {0, 1}
    for (h, w), (x0, y0, bw, bh) in zip(sizes, boxes):
        m = min(h, w)
        assert bw == bh and 1 <= bw <= m and bw * bw >= 0.69 * m * m - 2 * m
        assert 0 <= x0 and x0 + bw <= w and 0 <= y0 and y0 + bh <= h
    ops.ingest_desc(sizes, 'boxes', boxes=boxes, flips=flips)                                     # accepted as they come


def _unpack(hb, k):
    e = hb.desc[k]
    h, w, stride, off = int(e['h']), int(e['w']), int(e['stride']), int(e['offset'])
    rows = np.lib.stride_tricks.as_strided(hb.buf[off:], shape=(h, 3 * w), strides=(stride, 1))
    return np.array(rows).reshape(h, w, 3)


@pytest.mark.parametrize('workers', [1, 4])
@pytest.mark.parametrize('staging', [None, 64])
def test_packed_staging_buffer_holds_every_image(tmp_path, workers, staging):
    """the decode pool and the packing, against a plain re-read; ``staging=64`` bytes: every batch outgrows its staging buffer"""
    arrays = _dataset(tmp_path, 13)
    names = sorted(arrays)
    loader = data.DeviceImageLoader(str(tmp_path), 16, 4, workers=workers, staging_bytes=staging)
    for _ in range(2):                                                                            # re-iterable
        pipe = loader.host_pipeline()
        seen = []
        for hb in pipe:
            assert hb.nbytes == ops.ingest_packed_bytes(hb.desc) <= hb.buf.shape[0]
            assert (hb.slot == -1) == (staging is not None)
            for k, idx in enumerate(hb.indices):
                e = hb.desc[k]
                want = np.asarray(Image.open(loader.folder.path(idx)).convert('RGB'))
                assert np.array_equal(want, arrays[names[idx]])
                assert (int(e['h']), int(e['w']), int(e['stride'])) == (want.shape[0], want.shape[1], 3 * want.shape[1])
                assert (int(e['x0']), int(e['y0']), int(e['bw']), int(e['bh']), int(e['flip'])) == (0, 0, want.shape[1], want.shape[0], 0)
                assert np.array_equal(_unpack(hb, k), want)
            seen.extend(hb.indices)
            pipe.release(hb.slot)
        assert seen == list(range(13))
        pipe.close()
    loader.close()


def test_pack_images_honours_a_padded_stride():
    rng = np.random.default_rng(4)
    imgs = [_rgb(rng, 5, 7), _rgb(rng, 3, 2)]
    desc = ops.ingest_desc([(5, 7), (3, 2)], strides=[32, 9], offsets=[3, 200])
    buf = np.full(300, 0xAB, dtype=np.uint8)
    ops.pack_images(imgs, desc, buf)
    for k, img in enumerate(imgs):
        off, stride = int(desc[k]['offset']), int(desc[k]['stride'])
        for y in range(img.shape[0]):
            assert np.array_equal(buf[off + y * stride: off + y * stride + 3 * img.shape[1]], img[y].reshape(-1))
    assert buf[:3].tolist() == [0xAB] * 3 and buf[3 + 21:3 + 32].tolist() == [0xAB] * 11          # padding untouched
    with pytest.raises(ValueError):
        ops.pack_images([imgs[1], imgs[0]], desc, buf)


def test_a_broken_file_surfaces_in_the_consumer(tmp_path):
    _dataset(tmp_path, 3)
    (tmp_path / 'img001.png').write_bytes(b'not a png')
    loader = data.DeviceImageLoader(str(tmp_path), 8, 2, workers=2)
    with pytest.raises(Exception):
        list(loader.host_pipeline())
    loader.close()


def test_device_half_refuses_to_run_without_a_gpu(tmp_path):
    _dataset(tmp_path, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        iter(data.DeviceImageLoader(str(tmp_path), 8, 2, device='cpu'))


def test_entry_points_accept_the_reference_command_line(tmp_path):
    ref = ['--params_file', 'example_confs/standard_vqvae.yaml', '--dataloader', 'standard', '--workers', '8',
           '--dataset_path', str(tmp_path) + '/', '--seed', '0']
    a = train.parse_args(ref + ['--save_path', 'runs', '--run_name', 'r', '--num_nodes', '1'])
    assert (a.dataloader, a.workers, a.dataset_path, a.resize, a.check_val_every_n_epoch) == ('standard', 8, str(tmp_path) + '/', 'squash', 5)
    a = train.parse_args(ref + ['--resize', 'center_crop', '--check_val_every_n_epoch', '2'])
    assert (a.resize, a.check_val_every_n_epoch) == ('center_crop', 2)
    assert train.parse_args(['--params_file', 'x.yaml', '--seed', '1']).workers == 1                # the old command line still parses
    e = evaluate.parse_args(ref + ['--batch_size', '16', '--loading_path', 'last.ckpt'])
    assert (e.dataloader, e.workers, e.dataset_path, e.resize) == ('standard', 8, str(tmp_path) + '/', 'squash')
    with pytest.raises(SystemExit):
        train.parse_args(ref + ['--dataloader', 'ffcv'])
