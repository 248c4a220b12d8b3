"""The egress kernel (csrc/egress.hip) through ops.egress_u8 / ops.image_grid_u8, bit for bit against the CPU rule of
tests/egress_reference.py.  No tolerance anywhere: the rule is integer-valued and fully specified (the helper's own checks,
tests/test_egress_cpu.py, show that all 256 levels round-trip in 'unit', in 'sym' and through bf16)."""
import importlib

import pytest
import torch

from tests import egress_reference as R

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
DEV = 'cuda:0'


def _values(shape, seed, lo=-1.3, hi=1.3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def _nhwc(values_nchw, cpad, dtype):
    """the tree's padded NHWC form: [N,cpad,H,W] with channels contiguous; the pad channels hold junk that must not be read"""
    n, _, h, w = values_nchw.shape
    store = torch.full((n, h, w, cpad), 7.5, dtype=dtype, device=DEV)
    store[..., :3] = values_nchw.permute(0, 2, 3, 1).to(device=DEV, dtype=dtype)
    return store.permute(0, 3, 1, 2)


def _check(src, value_range):
    got = ops.egress_u8(src, value_range)
    torch.cuda.synchronize()
    want = R.egress(src, value_range)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape) and got.is_contiguous()
    diff = int((got.cpu() != want).sum())
    print(f'EGRESSMEASURE {tuple(src.shape)} strides {src.stride()} {src.dtype} {value_range}: {diff} bytes differ')
    assert diff == 0


SIZES = [(2, 256, 256), (3, 1, 1), (2, 97, 31), (1, 33, 4096)]


@pytest.mark.parametrize('n,h,w', SIZES)
def test_fp32_nchw_unit(n, h, w):
    _check(_values((n, 3, h, w), 1, -0.2, 1.2).to(DEV), 'unit')


@pytest.mark.parametrize('n,h,w', SIZES)
@pytest.mark.parametrize('cpad', [4, 8])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_nhwc_padded_sym(n, h, w, cpad, dtype):
    src = _nhwc(_values((n, 3, h, w), 2), cpad, dtype)
    assert src.stride(1) == 1 and src.shape[1] == cpad
    _check(src, 'sym')
    _check(src, 'unit')


def test_other_layouts_and_slices():
    x = _values((6, 3, 40, 56), 3).to(DEV)
    _check(x[1:5:2], 'sym')                                             # a strided batch slice of NCHW
    _check(x[:, :, 3:30, 5:41], 'sym')                                  # a window: rows and columns strided
    _check(x.bfloat16(), 'sym')                                         # bf16 NCHW: the scalar bf16 path
    p = _nhwc(_values((6, 3, 40, 56), 4), 8, torch.bfloat16)
    _check(p[2:5], 'sym')
    _check(p[:, :3], 'sym')                                             # what Decoder.forward returns: 3 of 8 channels, in place
    _check(p[:, :, 1:, 1:], 'sym')                                      # a window of the padded form
    flat = torch.full((2 * 6 * 5 * 8 + 1,), 7.5, dtype=torch.bfloat16, device=DEV)
    off = flat[1:].view(2, 6, 5, 8).permute(0, 3, 1, 2)                 # padded NHWC whose pixels are off the vector alignment
    off[:, :3] = _values((2, 3, 6, 5), 7).to(DEV).bfloat16()
    _check(off, 'sym')
    q = _nhwc(_values((2, 3, 8, 8), 5), 4, torch.float32)
    _check(q[:, :, :, 1::2], 'unit')
    dense3 = _values((2, 3, 9, 11), 6).to(DEV).contiguous(memory_format=torch.channels_last)
    _check(dense3, 'unit')                                              # NHWC with exactly 3 channels: no fourth element to read


def test_boundaries_between_levels():
    """inputs one ulp below, at and one ulp above every (k + 0.5) / 255, in both ranges: where a differently rounded
    implementation (a reciprocal, a double-rounded scale, a wrong clip order) lands on the other level.  Measured on the CPU
    while writing this test: a single-rounded t * 255 + 0.5 (what an FMA contraction computes) agrees with the separately
    rounded rule on every one of these inputs, on all floats within 16 ulps of every boundary and on 2e7 random inputs of
    [0,1] -- so this sweep pins the rule; it cannot tell a contraction apart, and the kernel's no-FMA property is a property
    of its build (csrc/Makefile, the pragma in csrc/egress.hip), checked in the ISA."""
    k = torch.arange(256, dtype=torch.float32)
    b = (k + 0.5) / 255
    up, down = torch.nextafter(b, torch.tensor(float('inf'))), torch.nextafter(b, torch.tensor(-float('inf')))
    unit = torch.cat([down, b, up, k / 255])                            # 1024 values
    for name, vals in (('unit', unit), ('sym', torch.cat([unit * 2 - 1, torch.nextafter(unit * 2 - 1, torch.tensor(2.0))]))):
        m = vals.numel() // 3 * 3
        src = vals[:m].view(1, 3, 1, m // 3).to(DEV)
        _check(src, name)
        _check(vals.repeat(3)[: 3 * 1024].view(1, 3, 32, 32).to(DEV), name)
    # the rule against exact arithmetic: both fp32 forms round 128 of the 256 exact boundaries up (b itself is not exact)
    exact = torch.floor(unit.double() * 255 + 0.5).to(torch.uint8)
    print(f'EGRESSMEASURE boundary sweep: {int((exact != R.quantise(unit, "unit")).sum())} of {unit.numel()} inputs differ from real arithmetic')


def test_non_finite_inputs():
    vals = torch.tensor([float('inf'), -float('inf'), float('nan'), 0.25, -0.0, 1.0] * 2).view(1, 3, 2, 2)
    for rng in ('unit', 'sym'):
        _check(vals.to(DEV), rng)
        _check(_nhwc(vals, 4, torch.float32), rng)
        _check(_nhwc(vals, 8, torch.bfloat16), rng)
    got = ops.egress_u8(vals.to(DEV), 'unit').cpu()                     # channel 0 holds +Inf, -Inf, NaN, 0.25
    assert [int(got[0, 0, 0, 0]), int(got[0, 0, 1, 0]), int(got[0, 1, 0, 0]), int(got[0, 1, 1, 0])] == [255, 0, 0, 64]


GUARD = 37                                                              # odd: the canvas starts off every alignment


@pytest.mark.parametrize('nrow', [1, 3, 8])
@pytest.mark.parametrize('pad', [0, 2])
@pytest.mark.parametrize('counts', [(8, 8), (3, 2), (5,), (6, 3, 1)])
def test_grids_define_every_canvas_byte_and_nothing_else(nrow, pad, counts):
    h, w = 13, 10
    cols = max(1, min(nrow, sum(counts)))
    if any(c % cols for c in counts[:-1]):
        with pytest.raises(RuntimeError, match='whole rows'):
            ops.image_grid_u8([torch.zeros(c, 3, h, w, device=DEV) for c in counts], nrow, pad)
        return
    makers = [lambda v: v.to(DEV), lambda v: _nhwc(v, 8, torch.bfloat16), lambda v: _nhwc(v, 4, torch.float32)]
    ranges = ['unit', 'sym', 'sym'][:len(counts)]
    sources = [makers[i]((_values((c, 3, h, w), 10 + i))) for i, c in enumerate(counts)]
    rows, cols2, hg, wg = ops.image_grid_shape(sum(counts), h, w, nrow, pad)
    assert cols2 == cols
    nbytes = hg * wg * 3
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    canvas = buf[GUARD:GUARD + nbytes].view(hg, wg, 3)
    out = ops.image_grid_u8(sources, nrow, pad, pad_value=0, value_ranges=ranges, out=canvas)
    torch.cuda.synchronize()
    assert out.data_ptr() == canvas.data_ptr()
    want = R.image_grid(sources, nrow, pad, 0, ranges)
    host = buf.cpu()
    assert tuple(want.shape) == (hg, wg, 3)
    assert torch.equal(host[GUARD:GUARD + nbytes].view(hg, wg, 3), want)             # images, padding and empty cells
    assert int((host[:GUARD] != 0xA5).sum()) == 0 and int((host[GUARD + nbytes:] != 0xA5).sum()) == 0
    # allocating form, another pad level
    got = ops.image_grid_u8(sources, nrow, pad, pad_value=200, value_ranges=ranges)
    assert torch.equal(got.cpu(), R.image_grid(sources, nrow, pad, 200, ranges))


def test_plain_stack_with_guards_at_every_alignment():
    src = _nhwc(_values((3, 3, 7, 5), 20), 4, torch.float32)
    want = R.egress(src, 'sym')
    nbytes = want.numel()
    for lead in range(0, 17):
        buf = torch.full((64 + nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        ops.egress_u8(src, 'sym', out=buf[lead:lead + nbytes].view(3, 7, 5, 3))
        host = buf.cpu()
        assert torch.equal(host[lead:lead + nbytes].view(3, 7, 5, 3), want), lead
        assert int((host[:lead] != 0xA5).sum()) == 0 and int((host[lead + nbytes:] != 0xA5).sum()) == 0, lead


def test_out_path_under_graph_capture_and_replay():
    """with out= nothing is allocated and nothing synchronises: the calls capture, and a replay follows the inputs"""
    gt = _values((8, 3, 64, 64), 30, 0.0, 1.0).to(DEV)
    rec = _nhwc(_values((8, 3, 64, 64), 31), 8, torch.bfloat16)
    rows, cols, hg, wg = ops.image_grid_shape(16, 64, 64, 8, 2)
    grid = torch.empty(hg, wg, 3, dtype=torch.uint8, device=DEV)
    stack = torch.empty(8, 64, 64, 3, dtype=torch.uint8, device=DEV)
    ops.image_grid_u8([gt, rec], 8, 2, value_ranges=['unit', 'sym'], out=grid)       # (library load, first launch)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
        before = torch.cuda.memory_allocated()                          # (inside: the capture itself allocates its RNG state)
        ops.image_grid_u8([gt, rec], 8, 2, value_ranges=['unit', 'sym'], out=grid)
        ops.egress_u8(rec, 'sym', out=stack)
        assert torch.cuda.memory_allocated() == before
    gt.copy_(_values((8, 3, 64, 64), 32, 0.0, 1.0))
    rec.copy_(_nhwc(_values((8, 3, 64, 64), 33), 8, torch.bfloat16))
    grid.fill_(0xA5), stack.fill_(0xA5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(grid.cpu(), R.image_grid([gt, rec], 8, 2, 0, ['unit', 'sym']))
    assert torch.equal(stack.cpu(), R.egress(rec, 'sym'))


def test_bad_arguments_are_refused():
    x = torch.zeros(2, 3, 4, 4, device=DEV)
    with pytest.raises(RuntimeError):
        ops.egress_u8(x, 'bytes')
    with pytest.raises(RuntimeError):
        ops.egress_u8(x.double(), 'unit')
    with pytest.raises(RuntimeError):
        ops.egress_u8(x[:, :2], 'unit')
    with pytest.raises(RuntimeError):
        ops.egress_u8(x, 'unit', out=torch.empty(2, 4, 4, 3, device=DEV))          # not uint8
    with pytest.raises(RuntimeError):
        ops.image_grid_u8([x, torch.zeros(2, 3, 5, 4, device=DEV)], 2)
    with pytest.raises(RuntimeError):
        ops.image_grid_u8([x], 2, pad_value=300)
