"""Float64 closed forms, input makers and launcher mirrors of the small kernels between the conv / GroupNorm / quantizer families:
csrc/pointwise.hip (pool2x2, unpool2x2, preprocess, sse, mse_tanh_backward, tanh_backward, axpby, pair_stats, ssim_sum) and
csrc/colsum.hip (the seven forms behind vqk_colsum_lead).  Shared by tests/test_pointwise_cpu.py (which keeps this module honest)
and tests/test_gpu_pointwise_forms.py (which holds the kernels to it).

Two kinds of input per kernel:
  ``exact``  dyadic values -- small integers in [-8, 8] for summands and pooled values, multiples of 1/8 inside (-1, 1) for the y of
             the tanh backward, differences in {-1, 0, 1} at the largest sum sizes, power-of-two scales -- chosen so that the
             float64 result is representable in the kernel's output type and every fp32 partial sum is exact in ANY order: the
             kernel must equal the closed form bit for bit, and a dropped, duplicated or misplaced element shows at any size.
  ``real``   random reals, rounded to bf16 first where the kernel reads bf16.  Elementwise kernels are held to
             |got - want| <= R * 2^-24 * S (+ 2^-8 |want| for a bf16 output: one bf16 rounding), S the sum of the absolute values
             of the expression's terms and R the number of fp32 operations of the kernel's expression (``R_OPS``); column sums
             to a relative norm of 5e-6, scalar sums to 1e-6 relative (the bounds the suite already holds them to).

The launcher mirrors (``*_plan``) repeat the host arithmetic of the C launchers -- which form serves, grid, rows per block, row
step, partial count after the workspace halving, trips of the grid-stride loop -- so that a test can assert that a case sits
where its comment says.

SSIM cancels (E[a^2] - E[a]^2), so its bound is not a rounding count: ``ssim_restate`` repeats the kernel's arithmetic in fp32 on the
CPU -- the same fused-multiply-add chain over the window, tap by tap in (ky, kx) order, the same fp32 tail -- and ``TABLE`` holds
its distance to float64 per (kind, ksize), the worst over ``SSIM_SHAPES``, rounded up to two digits.  The GPU test allows 4x an
entry: the kernel makes the same roundings and differs in the order of the cross-lane sum only (the compiler may also contract
``epp - mp * mp`` of the tail into one fma: within the same 4x).  test_pointwise_cpu.py recomputes every entry.
"""
import math
import zlib

import torch

from oracle import vqvae_oracle as O

F32, BF = torch.float32, torch.bfloat16
DT = {'fp32': F32, 'bf16': BF}
DTYPES = ('fp32', 'bf16')
EPS32, BF_EPS = 2.0 ** -24, 2.0 ** -8
OK, ERR_SHAPE, ERR_DTYPE, ERR_ALIGN, ERR_ARG = 0, -1, -2, -3, -5         # include/vqk.h: enum vqk_status
COLSUM_REL, SCALAR_REL = 5e-6, 1e-6                                        # test_gpu_gn_forms._BOUNDS[...]['colsum']; test_metrics.py
# fp32 operations of each elementwise kernel's expression (csrc/pointwise.hip)
R_OPS = {'pool': 4,            # (a + b) + (d + e), * scale
         'unpool': 1,          # * scale
         'axpby': 3,           # a * x, b * y2, +
         'tanh_bwd': 3,        # y * y, 1 - ., dy * .
         'mse_bwd': 5,         # gscale * 2, y - t, *, y * y ... 1 - ., *   (+ 1 with gscale_dev: gscale *= *gs)
         'preprocess': 2}      # v - 0.5, / 0.5 (exact)


def vec(dtype: str) -> int:
    """elements of one 16-byte slot"""
    return 4 if dtype == 'fp32' else 8


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g, shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def reals(g, shape, dtype: str = 'fp32'):
    """standard normal reals as float64 values that the kernel's input type holds exactly"""
    return torch.randn(shape, generator=g).to(DT[dtype]).double()


# ---------------------------------------------------------------------------------------------- launcher mirrors
def grid_1d(items: int, per_block: int, cap: int = 256 * 8) -> int:
    """common.h: vqk_grid_1d"""
    return max(1, min(cdiv(items, per_block), cap))


def plan_1d(items: int, per_block: int, cap: int) -> dict:
    """grid of a grid-stride kernel of 256 threads and the trips its busiest thread makes"""
    g = grid_1d(items, per_block, cap)
    return dict(items=items, grid=g, trips=cdiv(items, g * 256), capped=cdiv(items, per_block) > cap)


def pool_plan(dtype, n, h, w, c):
    return plan_1d(n * (h // 2) * (w // 2) * (c // vec(dtype)), 256, 256 * 16)


def unpool_plan(dtype, n, h, w, c):
    return plan_1d(n * (2 * h) * (2 * w) * (c // vec(dtype)), 256, 256 * 16)


def preprocess_plan(n, h, w):
    return plan_1d(n * h * w, 256, 256 * 16)


SUM_ATOMIC_BLOCKS = 32                    # csrc/pointwise.hip: up to this many blocks add their partials by atomics


def sse_plan(n, scratch=True):
    """vqk_sse and vqk_pair_stats: 8 elements per thread below the cap; ``form``: 'atomic' (block partials added to the one float in
    arrival order) or 'ordered' (more than 32 blocks and a stream scratch: partials stored, added in block order by a second launch)"""
    plan = plan_1d(n, 256 * 8, 256 * 8)
    plan['form'] = 'ordered' if (plan['grid'] > SUM_ATOMIC_BLOCKS and scratch) else 'atomic'
    return plan


def bwd_plan(n):
    """vqk_tanh_backward and vqk_mse_tanh_backward: 4 elements per thread below the cap"""
    return plan_1d(n, 256 * 4, 256 * 8)


def axpby_plan(dtype, n):
    return plan_1d(n // vec(dtype), 256, 256 * 16)


PAST_SSE = (2048 + 1) * 2048 + 3          # cap + 1 blocks' worth plus 3 elements: a 9th trip where 8 is the most below the cap
PAST_BWD = (2048 + 1) * 1024 + 3          # a 5th trip where 4 is the most
PAST_VEC = (4096 + 1) * 256 + 3           # vectors of axpby: a second trip
SMALL_N = (1, 63, 64, 65, 255, 256, 257)
SUM_EDGE_N = (SUM_ATOMIC_BLOCKS * 2048, SUM_ATOMIC_BLOCKS * 2048 + 1)      # 32 blocks: the last atomic size ; 33: the first ordered one
DET_WS_BYTES = 64 << 20                   # ops._DET_WS_BYTES


def colsum_plan(dtype, rows, c, aligned=True, det=False, ws_bytes=DET_WS_BYTES) -> dict:
    """vqk_colsum_lead (csrc/colsum.hip): status, form and launch geometry"""
    if not (rows >= 0 and 0 < c <= 8192):
        return dict(status=ERR_SHAPE)
    if rows == 0:
        return dict(status=OK, form='none')
    v = vec(dtype)
    slots = c // v if c % v == 0 else None
    if det:
        nb = min(cdiv(rows, 64), 512)
        nb0 = nb
        while nb > 1 and nb * c * 4 > ws_bytes:
            nb >>= 1
        if nb * c * 4 > ws_bytes:
            return dict(status=ERR_ARG)
        rb = cdiv(rows, nb)
        halved = nb
        nb = cdiv(rows, rb)
        vecd = slots is not None and slots <= 256 and 256 % slots == 0 and aligned
        return dict(status=OK, form='ordered-vector' if vecd else 'ordered-scalar', nb_first=nb0, nb_halved=halved, blocks=nb, rpb=rb,
                    rstep=256 // slots if vecd else None, reduce_grid=cdiv(c, 8), reduce_trips=cdiv(nb, 32))
    blocks = min(cdiv(rows, 64), 1024)
    rpb = cdiv(rows, blocks)
    blocks = cdiv(rows, rpb)
    if slots is None or not aligned:
        return dict(status=OK, form='column', blocks=blocks, rpb=rpb, rstep=None, idle=0, col_trips=cdiv(c, 64))
    if slots <= 256:
        rstep = 256 // slots
        return dict(status=OK, form='vector', blocks=blocks, rpb=rpb, rstep=rstep, idle=256 - slots * rstep, slots=slots)
    return dict(status=OK, form='wide', blocks=blocks, rpb=rpb, rstep=None, idle=0, slots=slots, slot_trips=cdiv(slots, 256))


def ssim_plan(n, c, h, w, ks) -> dict:
    """vqk_ssim_sum: 16 x 16 output tiles per (image, channel) plane"""
    if ks not in (7, 11):
        return dict(status=ERR_ARG if (h >= ks and w >= ks) else ERR_SHAPE)
    if not (n > 0 and c > 0 and h >= ks and w >= ks and n * c <= 65535):
        return dict(status=ERR_SHAPE)
    oh, ow = h - ks + 1, w - ks + 1
    return dict(status=OK, grid=(cdiv(ow, 16), cdiv(oh, 16), n * c), oh=oh, ow=ow, last_rows=oh - 16 * (cdiv(oh, 16) - 1),
                last_cols=ow - 16 * (cdiv(ow, 16) - 1))


# ---------------------------------------------------------------------------------------------- float64 closed forms (NHWC)
def pool(x, scale):
    """x [N, H, W, C] -> [N, H/2, W/2, C]"""
    return ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])) * scale


def pool_terms(x, scale):
    a = x.abs()
    return ((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + (a[:, 1::2, 0::2] + a[:, 1::2, 1::2])) * abs(scale)


def unpool(x, scale):
    """x [N, H, W, C] -> [N, 2H, 2W, C]"""
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * scale


def preprocess(img, cpad):
    """img [N, 3, H, W] -> ([N, H, W, cpad], S: the terms of (clamp(v) - 0.5) / 0.5)"""
    v = img.clamp(0.0, 1.0).permute(0, 2, 3, 1)
    out = torch.zeros(*v.shape[:3], cpad, dtype=torch.float64)
    terms = torch.zeros_like(out)
    out[..., :3] = (v - 0.5) / 0.5
    terms[..., :3] = (v + 0.5) / 0.5
    return out, terms


def sse(r, t):
    return ((r - t) ** 2).sum()


def mse_bwd(r, t, gscale, gs, through_tanh):
    """-> (d, S)"""
    s = (1.0 if gs is None else gs) * gscale * 2.0
    d, terms = s * (r - t), abs(s) * (r.abs() + t.abs())
    if through_tanh:
        d, terms = d * (1.0 - r * r), terms * (1.0 + r * r)
    return d, terms


def tanh_bwd(dy, y):
    return dy * (1.0 - y * y), dy.abs() * (1.0 + y * y)


def axpby(x, y2, a, b):
    if y2 is None:
        return a * x, (a * x).abs()
    return a * x + b * y2, (a * x).abs() + (b * y2).abs()


def colsum(x, lead, scale, prefill):
    """x [rows, c] -> prefill + scale * the sums of the first ``lead`` columns"""
    return prefill + scale * x[:, :lead].sum(0)


def pair_stats(p, t, prev=None):
    """-> the record [sse, min t, max t, min p, max p], folded into ``prev``"""
    rec = torch.stack([((p - t) ** 2).sum(), t.min(), t.max(), p.min(), p.max()])
    if prev is not None:
        rec = torch.stack([prev[0] + rec[0], torch.minimum(prev[1], rec[1]), torch.maximum(prev[2], rec[2]),
                           torch.minimum(prev[3], rec[3]), torch.maximum(prev[4], rec[4])])
    return rec


def ssim_per_image(p, t, sigma):
    """the oracle's torchmetrics restatement in float64 (tests/test_metrics.py pins it to scipy for sigma 1.5, test_pointwise_cpu for
    both windows): mean SSIM per image"""
    return O.metric_ssim_per_image(p.double(), t.double(), sigma=sigma)


def ssim_window(sigma):
    ks = int(3.5 * sigma + 0.5) * 2 + 1
    return O.metric_gaussian_window(ks, sigma)


# ---------------------------------------------------------------------------------------------- elementwise bound
def elem_ratio(got, want, terms, r_ops, out_dtype):
    """worst |got - want| / (R 2^-24 S (+ 2^-8 |want| for bf16)) over the elements, and the worst |got - want|"""
    err = (got.double() - want).abs()
    bound = r_ops * EPS32 * terms + (BF_EPS * want.abs() if out_dtype == 'bf16' else 0.0)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(ratio.max()), float(err.max())


def representable(want, out_dtype) -> bool:
    """premise of an ``exact`` case: the float64 result is a value of the kernel's output type"""
    return bool((want.to(DT[out_dtype]).double() == want).all())


# ---------------------------------------------------------------------------------------------- input makers
def pool_input(kind, dtype, n, h, w, c, tag='pool'):
    """[N, H, W, C] float64, values of ``dtype``"""
    g = gen(tag, kind, dtype, n, h, w, c)
    return ints(g, (n, h, w, c)) if kind == 'exact' else reals(g, (n, h, w, c), dtype)


# (n, h, w, c per 16-byte slot count) of the INPUT of pool; unpool runs on the pooled size.  c is given in slots.
POOL_SHAPES = [
    ('one-slot', 1, 4, 4, 1),               # smallest c: 4 (fp32) / 8 (bf16)
    ('c24', 1, 4, 6, None),                 # c = 24: 6 / 3 slots, no power of two
    ('2x2', 1, 2, 2, 2),                    # smallest map: 2 x 2 -> 1 x 1
    ('6x10', 1, 6, 10, 2),                  # non-square
    ('n3', 3, 6, 10, 1),                    # several images
    ('past-cap', 1, 1448, 1460, 2),         # 724 * 730 * 2 = 1057040 > 4096 * 256 work items: a second trip
]
POOL_SCALES = (0.25, 1.0)


def pool_shape(case, dtype):
    name, n, h, w, slots = case
    return n, h, w, (24 if slots is None else slots * vec(dtype))


def unpool_shape(case, dtype):
    """input of unpool: the pooled size of the pool case; past the cap the OUTPUT counts (362 x 365 -> 724 x 730, 1057040 items)"""
    n, h, w, c = pool_shape(case, dtype)
    return (n, 362, 365, c) if case[0] == 'past-cap' else (n, h // 2, w // 2, c)


PRE_SHAPES = [('1x1', 2, 1, 1), ('3x5', 2, 3, 5), ('past-cap', 1, 1024, 1025)]      # 1049600 > 4096 * 256 pixels
PRE_SPECIAL = (-0.75, 1.5, 0.0, 0.5, 1.0, 0.1, 0.2499999, 1e-3)                      # < 0, > 1, 0, 0.5, 1, below 0.25 (v - 0.5 rounds)


def preprocess_input(kind, n, h, w):
    """[N, 3, H, W] float64 holding fp32 values"""
    g = gen('pre', kind, n, h, w)
    if kind == 'exact':
        return torch.randint(-32, 97, (n, 3, h, w), generator=g).double() / 64.0        # multiples of 1/64 in [-0.5, 1.5]
    x = (torch.rand((n, 3, h, w), generator=g) * 1.4 - 0.2).float()
    flat = x.view(-1)
    k = min(flat.numel(), len(PRE_SPECIAL))
    pos = torch.randperm(flat.numel(), generator=g)[:k]
    flat[pos] = torch.tensor(PRE_SPECIAL[:k], dtype=torch.float32)
    return x.double()


def sse_input(kind, dtype, n, tag='sse'):
    """(r of ``dtype``, t fp32) as float64"""
    g = gen(tag, kind, dtype, n)
    if kind == 'exact':
        r = ints(g, (n,))
        d = ints(g, (n,)) if n <= 257 else ints(g, (n,), -1, 1)
        return r, r - d
    return reals(g, (n,), dtype), reals(g, (n,))


POW2 = (1.0, 2.0, 4.0, 8.0)


def _signed_pow2(g, n):
    """0, +-1, +-2, +-4, +-8: products with (64 - j^2) / 64 stay within 8 significant bits"""
    mag = torch.tensor(POW2, dtype=torch.float64)[torch.randint(0, 4, (n,), generator=g)]
    return mag * torch.randint(-1, 2, (n,), generator=g).double()


def tanh_y(g, kind, dtype, n):
    if kind == 'exact':
        y = torch.randint(-7, 8, (n,), generator=g).double() / 8.0
    else:
        y = torch.tanh(torch.randn(n, generator=g).double()).to(DT[dtype]).double()
    if n >= 3:
        y[n // 2], y[n - 1] = 1.0, -1.0                    # |y| exactly 1: the gradient is exactly 0
    return y


def tanh_bwd_input(kind, dtype, n):
    g = gen('tanh', kind, dtype, n)
    y = tanh_y(g, kind, dtype, n)
    return (_signed_pow2(g, n) if kind == 'exact' else reals(g, (n,), dtype)), y


def mse_bwd_input(kind, dtype, n):
    """(r = y of the tanh head, of ``dtype``; t fp32)"""
    g = gen('msebwd', kind, dtype, n)
    y = tanh_y(g, kind, dtype, n)
    if kind == 'exact':
        return y, y - _signed_pow2(g, n) / 2.0             # y - t in {0, +-.5, +-1, +-2, +-4}
    return y, reals(g, (n,))


MSE_GSCALE = 2.0 ** -4
AXPBY_AB = ((-2.0, 1.0), (0.5, 0.25))


def axpby_input(kind, dtype, n):
    g = gen('axpby', kind, dtype, n)
    mk = (lambda: ints(g, (n,))) if kind == 'exact' else (lambda: reals(g, (n,), dtype))
    return mk(), mk()


def colsum_input(kind, dtype, rows, c, lead):
    """(x [rows, c] of ``dtype``, prefill [lead]) as float64"""
    g = gen('colsum', kind, dtype, rows, c)
    if kind == 'exact':
        return ints(g, (rows, c)), ints(g, (lead,))
    return reals(g, (rows, c), dtype), reals(g, (lead,))


# name, dtype, rows, c, lead (None = c), scale, element offset of x from a 16-byte boundary,
#   atomic (form, blocks, rows per block, rstep), deterministic (form, blocks = partials, rows per block)  -- derived by hand
COLSUM_CASES = [
    ('vec-c128', 'bf16', 130, 128, None, 1.0, 0, ('vector', 3, 44, 16), ('ordered-vector', 3, 44)),           # last block: 42 rows
    ('idle-c96', 'fp32', 130, 96, None, 1.0, 0, ('vector', 3, 44, 10), ('ordered-scalar', 3, 44)),            # 24 slots: 16 idle lanes
    ('idle-c24', 'bf16', 130, 24, None, 1.0, 0, ('vector', 3, 44, 85), ('ordered-scalar', 3, 44)),            # 3 slots: 1 idle lane
    ('slots256-c1024', 'fp32', 70, 1024, None, 1.0, 0, ('vector', 2, 35, 1), ('ordered-vector', 2, 35)),
    ('slots256-c2048', 'bf16', 70, 2048, None, 1.0, 0, ('vector', 2, 35, 1), ('ordered-vector', 2, 35)),
    ('wide-c1028', 'fp32', 70, 1028, None, 1.0, 0, ('wide', 2, 35, None), ('ordered-scalar', 2, 35)),         # 257 slots: thread 0 twice
    ('wide-c8192', 'bf16', 70, 8192, None, 1.0, 0, ('wide', 2, 35, None), ('ordered-scalar', 2, 35)),
    ('wide-c8192', 'fp32', 70, 8192, None, 1.0, 0, ('wide', 2, 35, None), ('ordered-scalar', 2, 35)),
    ('col-c3', 'fp32', 130, 3, None, 1.0, 0, ('column', 3, 44, None), ('ordered-scalar', 3, 44)),
    ('col-c1', 'fp32', 130, 1, None, 1.0, 0, ('column', 3, 44, None), ('ordered-scalar', 3, 44)),
    ('col-c65', 'bf16', 130, 65, None, 1.0, 0, ('column', 3, 44, None), ('ordered-scalar', 3, 44)),           # column 64: lane 0 again
    ('col-c100', 'bf16', 130, 100, None, 1.0, 0, ('column', 3, 44, None), ('ordered-scalar', 3, 44)),
    ('col-misaligned-c128', 'bf16', 130, 128, None, 1.0, 1, ('column', 3, 44, None), ('ordered-scalar', 3, 44)),
    ('rows1', 'fp32', 1, 8, None, 1.0, 0, ('vector', 1, 1, 128), ('ordered-vector', 1, 1)),
    ('rows63', 'fp32', 63, 8, None, 1.0, 0, ('vector', 1, 63, 128), ('ordered-vector', 1, 63)),
    ('rows64', 'bf16', 64, 8, None, 1.0, 0, ('vector', 1, 64, 256), ('ordered-vector', 1, 64)),
    ('rows65', 'bf16', 65, 8, None, 1.0, 0, ('vector', 2, 33, 256), ('ordered-vector', 2, 33)),
    ('rows66000', 'fp32', 66000, 8, None, 1.0, 0, ('vector', 1016, 65, 128), ('ordered-vector', 512, 129)),   # past the 1024-block cap
    ('rows66000', 'bf16', 66000, 8, None, 1.0, 0, ('vector', 1016, 65, 256), ('ordered-vector', 512, 129)),
    ('lead3', 'fp32', 130, 8, 3, 0.25, 0, ('vector', 3, 44, 128), ('ordered-vector', 3, 44)),
    ('lead3', 'bf16', 130, 8, 3, 0.25, 0, ('vector', 3, 44, 256), ('ordered-vector', 3, 44)),
    ('reduce35-c128', 'bf16', 2200, 128, None, 1.0, 0, ('vector', 35, 63, 16), ('ordered-vector', 35, 63)),   # 35 partials: 2 trips
    ('reduce35-c4', 'fp32', 2200, 4, None, 1.0, 0, ('vector', 35, 63, 256), ('ordered-vector', 35, 63)),      # c % 8 != 0, vector
    ('reduce35-c100', 'bf16', 2200, 100, None, 1.0, 0, ('column', 35, 63, None), ('ordered-scalar', 35, 63)),  # c % 8 != 0, scalar
    ('reduce35-c12', 'fp32', 2200, 12, 5, 0.5, 0, ('vector', 35, 63, 85), ('ordered-scalar', 35, 63)),
]
# deterministic mode with a workspace of exactly ``room`` partial rows: name, dtype, rows, c, room, (form, nb first, halved, final, rpb)
HALVING_CASES = [
    ('halve-c128', 'bf16', 1000, 128, 4, ('ordered-vector', 16, 4, 4, 250)),
    ('halve-c96', 'fp32', 1000, 96, 4, ('ordered-scalar', 16, 4, 4, 250)),
    ('halve-c8-room5', 'fp32', 1000, 8, 5, ('ordered-vector', 16, 4, 4, 250)),        # room for 5: 16 -> 8 -> 4, not 5
    ('halve-to-1', 'bf16', 1000, 24, 1, ('ordered-scalar', 16, 1, 1, 1000)),
]


def colsum_id(case):
    return f'{case[0]}-{case[1]}'


# ---------------------------------------------------------------------------------------------- pair_stats / SSIM
def pair_input(kind, n, negative=False, tag='pair'):
    """(p, t) fp32 values as float64"""
    g = gen(tag, kind, n, negative)
    if kind == 'exact':
        t = ints(g, (n,), -8, -2) if negative else ints(g, (n,))
        d = ints(g, (n,)) if (n <= 257 and not negative) else ints(g, (n,), -1, 1)
        return t + d, t
    t = torch.rand(n, generator=g) - (3.0 if negative else 0.0)
    p = t + 0.1 * torch.randn(n, generator=g)
    return p.double(), t.double()


SSIM_SIGMA = {11: 1.5, 7: 0.8}
SSIM_KINDS = ('noisy', 'prange', 'same')
SSIM_NOISE = (0.02, 0.1, 0.4)             # per image: very different SSIM values in one batch
# (b, c, h, w) per window size: h == ks (one output row) ; output exactly 16 ; 17 (a second tile with one live row) ; non-square
SSIM_SHAPES = {11: [(3, 1, 11, 30), (3, 3, 26, 26), (3, 3, 27, 27), (3, 1, 27, 43)],
               7: [(3, 1, 7, 25), (3, 3, 22, 22), (3, 3, 23, 23), (3, 1, 23, 39)]}
# where each shape sits, derived by hand: (ks, shape) -> (grid, live rows of the last tile row, live columns of the last tile column)
SSIM_EXPECT = {
    (11, (3, 1, 11, 30)): ((2, 1, 3), 1, 4), (11, (3, 3, 26, 26)): ((1, 1, 9), 16, 16),
    (11, (3, 3, 27, 27)): ((2, 2, 9), 1, 1), (11, (3, 1, 27, 43)): ((3, 2, 3), 1, 1),
    (7, (3, 1, 7, 25)): ((2, 1, 3), 1, 3), (7, (3, 3, 22, 22)): ((1, 1, 9), 16, 16),
    (7, (3, 3, 23, 23)): ((2, 2, 9), 1, 1), (7, (3, 1, 23, 39)): ((3, 2, 3), 1, 1),
}


def ssim_input(kind, shape):
    """(p, t) fp32 in [0, 1].  ``noisy``: the TARGET has the wider range (t spans [0, 1], p stays inside [0.05, 0.95]); ``prange``:
    the roles swapped, the PREDICTION has the wider range; ``same``: p == t"""
    g = gen('ssim', shape)
    b = shape[0]
    wide = torch.rand(shape, generator=g)
    wide.view(-1)[0], wide.view(-1)[-1] = 0.0, 1.0
    noise = torch.tensor([SSIM_NOISE[i % 3] for i in range(b)]).view(b, 1, 1, 1)
    narrow = (0.2 + 0.6 * wide + noise * torch.randn(shape, generator=g)).clamp(0.05, 0.95)
    if kind == 'same':
        return wide, wide.clone()
    return (narrow, wide) if kind == 'noisy' else (wide, narrow)


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values and its sum with a third are formed in float64 (the product exactly)
    and rounded to fp32 once (a double rounding can differ from the fused result by one ulp in about 2^-29 of the cases)"""
    return (a.double() * b.double() + c.double()).float()


def ssim_restate(p, t, window, k1=0.01, k2=0.03):
    """ssim_sum_kernel's arithmetic in fp32 on the CPU: per-image SUMS of the SSIM map [B] (fp32)"""
    ks = window.shape[0]
    b, c, h, w = p.shape
    oh, ow = h - ks + 1, w - ks + 1
    p, t, window = p.float(), t.float(), window.float()
    mp, mt, epp, ett, ept = (torch.zeros(b, c, oh, ow, dtype=torch.float32) for _ in range(5))
    for ky in range(ks):
        for kx in range(ks):
            wv, a, q = window[ky, kx], p[..., ky:ky + oh, kx:kx + ow], t[..., ky:ky + oh, kx:kx + ow]
            mp, mt = fma32(wv, a, mp), fma32(wv, q, mt)
            epp, ett, ept = fma32(wv, a * a, epp), fma32(wv, q * q, ett), fma32(wv, a * q, ept)
    rng = torch.maximum(p.max() - p.min(), t.max() - t.min())
    k1, k2 = torch.tensor(k1, dtype=torch.float32), torch.tensor(k2, dtype=torch.float32)
    c1, c2 = (k1 * rng) * (k1 * rng), (k2 * rng) * (k2 * rng)
    mpp, mtt, mpt = mp * mp, mt * mt, mp * mt
    spp, stt, spt = epp - mpp, ett - mtt, ept - mpt
    v = ((2.0 * mpt + c1) * (2.0 * spt + c2)) / ((mpp + mtt + c1) * (spp + stt + c2))
    return v.reshape(b, -1).sum(-1)


def ssim_figure(sums, want, shape, ks) -> float:
    """worst |per-image mean - float64| over the images of the batch (SSIM values are O(1): an absolute figure)"""
    valid = shape[1] * (shape[2] - ks + 1) * (shape[3] - ks + 1)
    return float((sums.double().cpu() / valid - want).abs().max())


# figure of ssim_restate against float64, worst over SSIM_SHAPES[ks]; ``same`` is 1 exactly in fp32 (both factors of the numerator
# equal those of the denominator bit for bit, and the sum of ones is exact): its entry is the float64 reference's own rounding
TABLE = {
    ('noisy', 11): 4.0e-07, ('prange', 11): 4.0e-07, ('same', 11): 1e-15,       # SSIM is symmetric in (p, t): ``prange`` is ``noisy``
    ('noisy', 7): 6.0e-07, ('prange', 7): 6.0e-07, ('same', 7): 1e-15,          # with the operands swapped, the same value
}                                                                               # (worst: the one-output-row shapes, 20 / 19 pixels)
