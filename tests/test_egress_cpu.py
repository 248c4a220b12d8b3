"""Host half of the image egress (csrc/egress.hip, ops.egress_u8 / image_grid_u8, imagelog.py): the CPU reference itself, the
argument checks of the entry points (made before any launch, so they run without a device), the new flags of the two entry
scripts and the PNG writer's host path."""
import importlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests import egress_reference as R

PKG = 'vqvae-vqgan-pytorch-lightning_amd'


def test_reference_grid_against_a_hand_written_example():
    """two images of 2 x 3, one row, padding 2: the canvas is 6 x 12, written out by hand"""
    a = torch.arange(1, 19, dtype=torch.uint8).view(1, 2, 3, 3)
    b = a + 100
    grid = R.make_grid(torch.cat([a, b]), nrow=2, padding=2, pad_value=0)
    assert tuple(grid.shape) == (2 + 2 + 2, 2 + 3 + 2 + 3 + 2, 3)
    z = [0, 0, 0]
    row0 = [z, z, [1, 2, 3], [4, 5, 6], [7, 8, 9], z, z, [101, 102, 103], [104, 105, 106], [107, 108, 109], z, z]
    row1 = [z, z, [10, 11, 12], [13, 14, 15], [16, 17, 18], z, z, [110, 111, 112], [113, 114, 115], [116, 117, 118], z, z]
    want = torch.tensor([[z] * 12, [z] * 12, row0, row1, [z] * 12, [z] * 12], dtype=torch.uint8)
    assert torch.equal(grid, want)
    # three images, two columns: the fourth cell stays padding; pad_value is honoured
    g3 = R.make_grid(torch.cat([a, b, a]), nrow=2, padding=1, pad_value=7)
    assert tuple(g3.shape) == (2 * 3 + 1, 2 * 4 + 1, 3)
    assert torch.equal(g3[4:6, 1:4], a[0]) and int((g3[4:6, 5:8] != 7).sum()) == 0 and int(g3[0].max()) == 7
    # nrow larger than the count: one row of `count` columns (make_grid's xmaps = min(nrow, count))
    assert tuple(R.make_grid(torch.cat([a, b]), nrow=8, padding=2).shape) == (6, 12, 3)


def test_reference_rule_round_trips_every_level():
    """k / 255 comes back as k in 'unit', in 'sym' and through bf16: the rule loses nothing a uint8 image holds"""
    k = torch.arange(256, dtype=torch.float32)
    unit = k / 255
    assert torch.equal(R.quantise(unit, 'unit'), k.to(torch.uint8))
    sym = unit * 2 - 1
    assert torch.equal(R.quantise(sym, 'sym'), k.to(torch.uint8))
    assert torch.equal(R.quantise(unit.bfloat16(), 'unit'), k.to(torch.uint8))
    assert torch.equal(R.quantise(sym.bfloat16(), 'sym'), k.to(torch.uint8))
    edge = torch.tensor([float('nan'), float('inf'), -float('inf'), -0.0, 2.0, -3.0])
    assert R.quantise(edge, 'unit').tolist() == [0, 255, 0, 0, 255, 0]
    assert R.quantise(edge, 'sym').tolist() == [0, 255, 0, 128, 255, 0]


def test_entry_points_validate_without_gpu():
    lib = importlib.import_module(PKG + '._native').lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data                                     # a non-NULL pointer: every call below is refused before a launch

    def call(dtype=0, src=p, n=2, c=3, h=4, w=4, strides=(48, 16, 4, 1), rng=0, canvas=p, rows=2, cols=1, row0=0, pad=0, pv=0):
        return lib.vqk_egress_u8(dtype, src, n, c, h, w, *strides, rng, canvas, rows, cols, row0, pad, pv, 0)

    assert call(src=0) == -5 and call(canvas=0) == -5       # NULL pointers
    assert call(n=0) == -1 and call(c=2) == -1
    assert call(h=0) == -1 and call(h=4097) == -1 and call(w=0) == -1 and call(w=4097) == -1
    assert call(dtype=2) == -1 and call(rng=2) == -1 and call(rng=-1) == -1
    assert call(rows=1) == -1                               # two images, one column, one row: a cell outside the canvas
    assert call(row0=1) == -1 and call(row0=-1) == -1
    assert call(pad=-1) == -1 and call(pv=256) == -1 and call(pv=-1) == -1 and call(rows=0) == -1 and call(cols=0) == -1
    assert call(n=60, h=4096, w=4096, rows=60) == -1        # 60 * 4096 * 4096 * 3 bytes >= 2^31
    assert call(src=p + 2) == -3                            # fp32 source off its element alignment
    assert lib.vqk_egress_canvas_bytes(4, 5, 2, 3, 2) == (2 * 6 + 2) * (3 * 7 + 2) * 3
    assert lib.vqk_egress_canvas_bytes(256, 256, 8, 1, 0) == 8 * 256 * 256 * 3
    assert lib.vqk_egress_canvas_bytes(4096, 4096, 43, 1, 0) == -1 and lib.vqk_egress_canvas_bytes(4096, 4096, 42, 1, 0) > 0
    assert lib.vqk_egress_canvas_bytes(0, 4, 1, 1, 0) == -1


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    ops = importlib.import_module(PKG + '.ops')
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.egress_u8(torch.zeros(2, 3, 4, 4), 'unit')
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.image_grid_u8([torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4)], nrow=2)
    assert ops.image_grid_shape(16, 64, 64, 8, 2) == (2, 8, 2 * 66 + 2, 8 * 66 + 2)
    assert ops.image_grid_shape(3, 5, 7, 8, 0) == (1, 3, 5, 21)


def test_entry_scripts_parse_the_new_flags():
    train = importlib.import_module(PKG + '.train')
    ev = importlib.import_module(PKG + '.evaluate')
    base = ['--params_file', 'x.yaml', '--seed', '0']
    assert train.parse_args(base).image_log_dir is None
    assert train.parse_args(base + ['--image_log_dir', 'logs']).image_log_dir == 'logs'
    ebase = base + ['--dataset_path', 'd', '--batch_size', '4', '--loading_path', 'c.ckpt']
    args = ev.parse_args(ebase)
    assert args.save_reconstructions is None and args.save_grid_every is None
    args = ev.parse_args(ebase + ['--save_reconstructions', 'out', '--save_grid_every', '3'])
    assert args.save_reconstructions == 'out' and args.save_grid_every == 3


def test_model_logging_is_off_by_default():
    model_mod = importlib.import_module(PKG + '.model')
    ae = dict(channels=32, num_res_blocks=1, channel_multipliers=(1, 2))
    qc = dict(num_embeddings=64, embedding_dim=16, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
    model = model_mod.VQVAE(32, ae, qc, None, None, init_cb=False, load_loss=False)
    assert model.image_log_dir is None and not model.image_log_due(2)
    assert model.log_reconstructions(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4)) is None      # a no-op: CPU tensors pass
    model.flush_image_log(), model.close_image_log()
    model.image_log_dir = 'somewhere'
    model.current_epoch = 5
    assert model.image_log_due(2) and not model.image_log_due(1)
    model.current_epoch = 6
    assert not model.image_log_due(2)
    model.current_epoch, model.defer_image_logging = 0, True
    assert not model.image_log_due(2)


def test_image_writer_round_trips_an_array_through_png(tmp_path):
    imagelog = importlib.import_module(PKG + '.imagelog')
    rng = np.random.default_rng(0)
    arrays = {f'sub/dir/img{k}.png': rng.integers(0, 256, size=(5 + k, 9, 3), dtype=np.uint8) for k in range(5)}
    writer = imagelog.ImageWriter(str(tmp_path), workers=3)
    for name, a in arrays.items():
        writer.write_array(name, a)
    writer.flush()
    assert writer.files_written == 5
    for name, a in arrays.items():
        assert np.array_equal(np.asarray(Image.open(tmp_path / name).convert('RGB')), a)
    writer.write_array(str(tmp_path / 'absolute.png'), arrays['sub/dir/img0.png'])
    writer.close()
    assert (tmp_path / 'absolute.png').exists()
    leftovers = [p.name for p in tmp_path.rglob('*') if '.tmp.' in p.name]
    assert leftovers == []                                              # temporary names were renamed away
    assert imagelog.ImageWriter(str(tmp_path), workers=99).workers == 16
    silent = imagelog.ImageWriter(str(tmp_path / 'other'), enabled=False)  # a rank that does not write
    silent.write_array('x.png', arrays['sub/dir/img0.png'])
    silent.close()
    assert not (tmp_path / 'other').exists()
    assert imagelog.unique_stems(['a/x.png', 'b/y.bmp', 'c/x.jpg']) == ['x_000000', 'y', 'x_000002']
