"""vqk_ingest_u8 / ops.ingest_u8 (csrc/ingest.hip) against ATen's antialiased bilinear resize in float64 on the CPU
(tests/ingest_reference.py: the bound is 4x the reference's own fp32 error on the same input, floor 2e-7).

Measured on the MI355X (INGESTMEASURE lines: max |kernel - fp64|, the reference's own fp32 error, the bound): photo sizes
2.2e-7..2.9e-7 where ATen's fp32 is at 2.3e-7..2.8e-7; worst absolute 4.3e-7 at (7,4099)->(32,48) (ATen fp32 5.8e-7, bound 2.3e-6);
worst against ATen's fp32 1.33x at the crop -> 128; 1x1 -> 96 is at 1.3e-7 under the 2e-7 floor.  DESIGN.md 8a."""
import importlib

import numpy as np
import pytest
import torch

from tests import ingest_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
_native = importlib.import_module(PKG + '._native')
DEV = 'cuda:0'
CANARY = -7.25

# (name, (h, w), output size, box (x0, y0, bw, bh) or None)
SHAPES = [('photo', (375, 500), 256, None), ('upscale', (64, 48), 256, None), ('large', (1200, 1600), 256, None),
          ('down32', (2048, 3000), 64, None), ('odd', (97, 31), 64, None), ('pixel', (1, 1), 16, None),
          ('wide', (7, 4099), (32, 48), None), ('crop', (333, 517), 128, (40, 21, 301, 301))]


def _image(h, w, seed):
    """smooth structure plus noise: neighbouring taps differ, and so do the channels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 120 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)], axis=2)
    return np.clip(base + rng.integers(-40, 41, size=(h, w, 3)), 0, 255).astype(np.uint8)


def _pack(images, desc):
    buf = np.zeros(ops.ingest_packed_bytes(desc), dtype=np.uint8)
    ops.pack_images(images, desc, buf)
    return torch.from_numpy(buf).to(DEV)


def _check(name, got, img, size, box, flip):
    want, bound, own = R.reference_and_bound(img, size, box, bool(flip))
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    err = float((got.double() - want).abs().max())
    print(f'INGESTMEASURE {name} {img.shape[0]}x{img.shape[1]} -> {tuple(want.shape[1:])} box {box} flip {int(flip)}: '
          f'kernel {err:.3e} reference-fp32 {own:.3e} bound {bound:.3e}')
    assert err <= bound, (name, err, bound)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 + 1e-6


@pytest.mark.parametrize('flip', [0, 1])
@pytest.mark.parametrize('name,hw,size,box', SHAPES, ids=[s[0] for s in SHAPES])
def test_single_image_vs_float64(name, hw, size, box, flip):
    img = _image(*hw, seed=len(name))
    desc = ops.ingest_desc([hw], 'boxes' if box else 'squash', boxes=[box] if box else None, flips=[flip])
    got = ops.ingest_u8(_pack([img], desc), desc, size)
    _check(name, got[0], img, size, box, flip)


def test_padded_row_stride():
    img = _image(120, 77, seed=3)
    desc = ops.ingest_desc([(120, 77)], strides=[77 * 3 + 13], offsets=[20])
    got = ops.ingest_u8(_pack([img], desc), desc, 48)
    _check('stride', got[0], img, 48, None, 0)


def test_ragged_batch_with_shuffled_descriptors():
    """every shape at once (square outputs to one size, the non-square one in a batch of its own below), descriptor order shuffled
    and two entries naming the same source"""
    square = [s for s in SHAPES if isinstance(s[2], int)]
    images = [_image(*s[1], seed=10 + k) for k, s in enumerate(square)]
    layout = ops.ingest_desc([s[1] for s in square])                                        # where the sources sit
    pixels = _pack(images, layout)
    order = np.random.default_rng(5).permutation(len(square)).tolist() + [0]
    boxes = [square[k][3] or (0, 0, square[k][1][1], square[k][1][0]) for k in order]
    flips = [(j * 7 + 1) % 2 for j in range(len(order))]
    desc = ops.ingest_desc([square[k][1] for k in order], 'boxes', boxes=boxes, flips=flips, offsets=[int(layout[k]['offset']) for k in order])
    got = ops.ingest_u8(pixels, desc, 96)
    assert tuple(got.shape) == (len(order), 3, 96, 96)
    for j, k in enumerate(order):
        _check('ragged-' + square[k][0], got[j], images[k], 96, square[k][3], flips[j])
    wide = [_image(7, 4099, seed=30), _image(64, 48, seed=31)]
    d2 = ops.ingest_desc([(64, 48), (7, 4099)], offsets=None)
    got = ops.ingest_u8(_pack(wide[::-1], d2), d2, (32, 48))
    _check('ragged-wide', got[1], wide[0], (32, 48), None, 0)
    _check('ragged-up', got[0], wide[1], (32, 48), None, 0)


def test_scale_one_is_bit_identical_to_totensor():
    img = _image(256, 256, seed=1)
    desc = ops.ingest_desc([(256, 256)])
    got = ops.ingest_u8(_pack([img], desc), desc, 256)[0].cpu()
    assert torch.equal(got, torch.from_numpy(img).permute(2, 0, 1).float().div(255))
    big = _image(300, 411, seed=2)
    box = (100, 31, 256, 256)
    desc = ops.ingest_desc([(300, 411)], 'boxes', boxes=[box])
    got = ops.ingest_u8(_pack([big], desc), desc, 256)[0].cpu()
    assert torch.equal(got, torch.from_numpy(big[31:287, 100:356].copy()).permute(2, 0, 1).float().div(255))
    desc = ops.ingest_desc([(300, 411)], 'boxes', boxes=[box], flips=[1])
    got = ops.ingest_u8(_pack([big], desc), desc, 256)[0].cpu()
    assert torch.equal(got, torch.from_numpy(big[31:287, 100:356].copy()).permute(2, 0, 1).float().div(255).flip(-1))


def test_out_slice_and_repeatability():
    images = [_image(90, 130, seed=4), _image(33, 21, seed=5)]
    desc = ops.ingest_desc([(90, 130), (33, 21)])
    pixels = _pack(images, desc)
    big = torch.full((5, 3, 40, 40), CANARY, device=DEV)
    ret = ops.ingest_u8(pixels, desc, 40, out=big[2:4])
    assert ret.data_ptr() == big[2:4].data_ptr()
    host = big.cpu()
    assert bool((host[:2] == CANARY).all()) and bool((host[4:] == CANARY).all())            # nothing outside the slice
    fresh = ops.ingest_u8(pixels, desc, 40)
    assert torch.equal(fresh.cpu(), host[2:4])
    again = ops.ingest_u8(pixels, desc, 40, desc_dev=torch.from_numpy(desc.view(np.uint8)).to(DEV))
    assert torch.equal(again.cpu(), fresh.cpu())                                            # no atomics, fixed order
    for k, img in enumerate(images):
        _check('slice', host[2 + k], img, 40, None, 0)
    # a strided batch: every other image of a larger tensor
    wide = torch.full((4, 3, 40, 40), CANARY, device=DEV)
    ops.ingest_u8(pixels, desc, 40, out=wide[0::2])
    w = wide.cpu()
    assert torch.equal(w[0::2], fresh.cpu()) and bool((w[1::2] == CANARY).all())


def _raw_call(pixels, desc, n, sh, sw, out, bstride=None):
    dd = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).to(DEV)
    st = _native.lib().vqk_ingest_u8(pixels.data_ptr(), pixels.numel(), np.ascontiguousarray(desc).ctypes.data, dd.data_ptr(), n, sh, sw,
                                     3 * sh * sw if bstride is None else bstride, out.data_ptr(), 0)
    torch.cuda.synchronize()
    return st


def test_out_of_range_arguments_are_refused_on_the_host():
    """argument checks before the launch: VQK_ERR_SHAPE, nothing launched, the canary intact"""
    img = _image(20, 30, seed=6)
    good = ops.ingest_desc([(20, 30)])
    pixels = _pack([img], good)
    out = torch.full((1, 3, 16, 16), CANARY, device=DEV)

    def bad(**fields):
        d = good.copy()
        for k, v in fields.items():
            d[0][k] = v
        return d
    cases = [(good, 1, 0, 16), (good, 1, 16, 0), (good, 1, 4097, 16), (good, 0, 16, 16),
             (bad(h=16385), 1, 16, 16), (bad(w=16385, stride=3 * 16385), 1, 16, 16), (bad(h=0), 1, 16, 16),
             (bad(bw=31), 1, 16, 16), (bad(x0=1), 1, 16, 16), (bad(y0=-1), 1, 16, 16), (bad(bh=0), 1, 16, 16), (bad(y0=5, bh=16), 1, 16, 16),
             (bad(stride=89), 1, 16, 16), (bad(offset=-16), 1, 16, 16), (bad(offset=16), 1, 16, 16), (bad(h=21), 1, 16, 16)]
    for desc, n, sh, sw in cases:
        assert _raw_call(pixels, desc, n, sh, sw, out) == _native.ERR_SHAPE, (desc, n, sh, sw)
    assert _raw_call(pixels, good, 1, 16, 16, out, bstride=3 * 16 * 16 - 1) == _native.ERR_SHAPE
    assert bool((out.cpu() == CANARY).all())
    with pytest.raises(RuntimeError):
        ops.ingest_u8(pixels, bad(h=16385), 16, out=out)
    with pytest.raises(RuntimeError):
        ops.ingest_u8(pixels, bad(x0=10, bw=25), 16, out=out)
    with pytest.raises(RuntimeError):
        ops.ingest_u8(pixels, good, 0)
    with pytest.raises(RuntimeError):
        ops.ingest_u8(pixels, good, 16, out=torch.empty(1, 3, 16, 16))                      # a CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        ops.ingest_u8(pixels.cpu(), good, 16)
    assert bool((out.cpu() == CANARY).all())
    assert _raw_call(pixels, good, 1, 16, 16, out) == 0                                     # and the good call still runs
    _check('after-refusals', out[0], img, 16, None, 0)
