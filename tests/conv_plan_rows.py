"""The forward-conv dispatch table shared by tests/test_conv_plan.py (CPU: the plan query) and tests/test_gpu_conv_plan.py (GPU:
every form launched once).

Each row is a problem, the state it is planned under, and the kernel form csrc/conv.hip::launch_fprop takes for it.  The
expectations were derived by READING the launcher's cascade as it stood before the plan function existed (one ``if`` per form,
in this order of precedence):

  fp32 -> fp32, layout 0, plain 3x3, variant != 0:  cout == 4, cin % 16, h % 8, w % 32 -> fp32 thin-out;  cin == 4, cout in
      {64, 128, 256}, no residual, act 0, w % 4, 10 * (w + 2) * 16 <= 64 KiB -> fp32 thin-in
  tw = halo_twlog: 0 unless (3x3, or 1x1 served by the matrix/auxiliary-wave kernel), whole 128-byte cin chunks, variant != 0;
      5 when w % 32 == 0 and h % 8 == 0, else 4 when w % 16 == 0 and h % 16 == 0, else 0
  layout 1, bf16 input, variant != 3:  tw == 0 -> VQK_ERR_SHAPE;  bf16 output, MX slot on, variant != 5, act 0 (or 2 / 3 without
      pooling and GroupNorm sums), cout % 128 == 0, cin >= 64, 32-bit offsets, tiles >= MX_MIN_TILES -> matrix/auxiliary-wave
      (1x1 with pooling: its launcher answers VQK_ERR_ARG);  GroupNorm sums or 1x1 -> VQK_ERR_SHAPE;  cout <= 32 -> stream,
      thin;  tiles < 256, h % 4 (tw 5) or h % 8 (tw 4), no pooling, bf16 output, variant != 4 -> stream, half tiles;  else
      stream, full tiles            (tiles = n * (h / (256 >> tw)) * (w >> tw) * ceil(cout / 128))
  layout 1 otherwise:  tw == 0 or 1x1 -> VQK_ERR_SHAPE;  else register-weight halo
  layout 0:  tw and 3x3 -> LDS-weight halo;  bf16 -> bf16, 3x3, cin == 8, no residual, plain, w % 32, cout % 8, variant != 0 ->
      bf16 thin-in, one launch per 128 output channels;  else im2col, with split-K when a scratch is set, cout % 4 == 0 and
      min(SK_BLOCKS / grid if 2 * grid <= SK_BLOCKS else 1, ksteps / SK_MINSTEPS, SK_MAXMB and scratch bytes / output bytes) >= 2
      (grid = ceil(m / 128) * ceil(cout / 128), ksteps = ceil(k * k * cin_chunks / 8))
  layout 5 (vqk_conv2d_fprop's own branch): fp32 -> fp32 else VQK_ERR_ARG; cin % 32, h % 8, w % 16, cout % 4, no upsampled 1x1,
      else VQK_ERR_SHAPE -> split-product kernel
"""
import collections

F32, BF16 = 0, 1                                                 # include/vqk.h dtype codes
ERR_SHAPE, ERR_ARG = -1, -5
# include/vqk.h: form ids of vqk_conv_fprop_plan
(THIN_OUT_F32, THIN_IN_F32, MX, MX_1X1, STREAM_THIN, STREAM_HALF, STREAM_FULL, HALO_BREG, HALO_LDS, THIN_IN_BF16, IM2COL,
 IM2COL_SPLITK, X3, X3_1X1) = range(14)
RESIDUAL, POOL, GNSTATS, GENERAL = 1, 2, 4, 8                    # flags

Row = collections.namedtuple('Row', 'name dtype out_dtype n h w cin cout ksize ups act wlayout flags variant tuning scratch '
                                    'form tw launches splits')


def _row(name, dtype, out_dtype, h, w, cin, cout, wlayout, form, tw=None, n=1, ksize=3, ups=0, act=0, flags=0, variant=-1,
         tuning=None, scratch=0, launches=1, splits=1):
    return Row(name, dtype, out_dtype, n, h, w, cin, cout, ksize, ups, act, wlayout, flags, variant, tuning or {}, scratch,
               form, tw, launches, splits)


ROWS = [
    # ---- the issue's anchor rows
    _row('mx', BF16, BF16, 256, 256, 128, 128, 1, MX, 5),
    _row('mx-off-v5', BF16, BF16, 256, 256, 128, 128, 1, STREAM_FULL, 5, variant=5),
    _row('half-v5', BF16, BF16, 128, 128, 128, 128, 1, STREAM_HALF, 5, variant=5),
    # variant 4 alone does not keep the matrix/auxiliary-wave kernel away (its test comes first in the cascade): the stream
    # kernel with full tiles is what variant 4 gives once that kernel is off (MX slot 0) ...
    _row('no-half-v4-mx-off', BF16, BF16, 128, 128, 128, 128, 1, STREAM_FULL, 5, variant=4, tuning={'MX': 0}),
    # ... and at the default tuning the same problem stays on the matrix/auxiliary-wave kernel
    _row('no-half-v4', BF16, BF16, 128, 128, 128, 128, 1, MX, 5, variant=4),
    _row('stream-thin', BF16, BF16, 32, 32, 128, 32, 1, STREAM_THIN, 5),
    _row('stream-f32-out', BF16, F32, 32, 32, 128, 128, 1, STREAM_FULL, 5),
    _row('cin32-refused', BF16, BF16, 32, 32, 32, 128, 1, ERR_SHAPE),
    _row('tw4', BF16, BF16, 48, 48, 128, 128, 1, MX, 4),
    _row('im2col', BF16, BF16, 24, 24, 128, 128, 0, IM2COL, 0),
    _row('mx-1x1', BF16, BF16, 64, 64, 256, 128, 1, MX_1X1, 5, ksize=1),
    _row('1x1-f32-out-refused', BF16, F32, 64, 64, 256, 128, 1, ERR_SHAPE, ksize=1),
    _row('breg-f32', F32, F32, 32, 32, 64, 64, 1, HALO_BREG, 5),
    _row('halo-lds-f32', F32, F32, 32, 32, 64, 64, 0, HALO_LDS, 5),
    _row('im2col-f32-v0', F32, F32, 32, 32, 64, 64, 0, IM2COL, 0, variant=0),
    _row('thin-out-f32', F32, F32, 32, 32, 64, 4, 0, THIN_OUT_F32, 0),
    _row('thin-in-f32', F32, F32, 32, 32, 4, 128, 0, THIN_IN_F32, 0),
    _row('thin-in-bf16', BF16, BF16, 32, 32, 8, 128, 0, THIN_IN_BF16, 0),
    _row('thin-in-bf16-x2', BF16, BF16, 32, 32, 8, 256, 0, THIN_IN_BF16, 0, launches=2),
    # ---- split-K: n 2, 256 -> 256 @ 4x4: grid 1 x 2, ksteps 36 -> min(2048 / 2, 36 / 4 = 9, 32 MiB / 32 KiB) = 9 parts of 4 steps
    _row('split-k', BF16, BF16, 4, 4, 256, 256, 0, IM2COL_SPLITK, 0, n=2, scratch=1 << 20, launches=2, splits=9),
    _row('split-k-no-scratch', BF16, BF16, 4, 4, 256, 256, 0, IM2COL, 0, n=2),
    # ---- the remaining forms, variants and refusals
    _row('half-tw4', BF16, BF16, 16, 16, 64, 64, 1, STREAM_HALF, 4),                       # cout 64: no whole 128-cout tile
    _row('breg-bf16-v3', BF16, BF16, 32, 32, 128, 128, 1, HALO_BREG, 5, variant=3),
    _row('halo-lds-bf16', BF16, BF16, 32, 32, 128, 128, 0, HALO_LDS, 5),
    _row('halo-lds-tw4', BF16, BF16, 16, 48, 128, 128, 0, HALO_LDS, 4),
    _row('mx-min-tiles', BF16, BF16, 32, 32, 128, 128, 1, STREAM_HALF, 5, tuning={'MX_MIN_TILES': 8}),      # 4 tiles < 8
    _row('mx-v6', BF16, BF16, 32, 32, 128, 128, 1, MX, 5, variant=6, tuning={'MX_MIN_TILES': 8}),
    _row('mx-relu', BF16, BF16, 32, 32, 128, 128, 1, MX, 5, act=2),
    _row('stream-tanh', BF16, BF16, 32, 32, 128, 128, 1, STREAM_HALF, 5, act=1),            # act 1 is no epilogue of conv_mx.hip
    _row('mx-ups', BF16, BF16, 16, 16, 128, 128, 1, MX, 5, ups=1),
    # the pooled epilogue is the ResBlock + Downsample pair: it always adds a residual (and parks the conv sums as bf16 before the
    # 2x2 sum -- without the residual's magnitude four roundings of unpooled values overrun a bound relative to the pooled value)
    _row('mx-pooled', BF16, BF16, 32, 32, 128, 128, 1, MX, 5, flags=POOL | RESIDUAL),
    _row('mx-gnstats', BF16, BF16, 32, 32, 128, 128, 1, MX, 5, flags=GNSTATS | RESIDUAL),
    _row('stream-pooled-v5', BF16, BF16, 32, 32, 128, 128, 1, STREAM_FULL, 5, flags=POOL | RESIDUAL, variant=5),     # pooling: no half tiles
    _row('gnstats-refused-v5', BF16, BF16, 32, 32, 128, 128, 1, ERR_SHAPE, flags=GNSTATS, variant=5),
    _row('pooled-refused-v2', BF16, BF16, 32, 32, 128, 128, 1, ERR_SHAPE, flags=POOL, variant=2),
    _row('pooled-1x1-refused', BF16, BF16, 64, 64, 256, 128, 1, ERR_ARG, ksize=1, flags=POOL),
    _row('1x1-ups-refused', BF16, BF16, 32, 32, 256, 128, 1, ERR_SHAPE, ksize=1, ups=1),
    _row('1x1-im2col', BF16, BF16, 64, 64, 256, 128, 0, IM2COL, 0, ksize=1),
    _row('breg-f32-shape-refused', F32, F32, 24, 24, 64, 64, 1, ERR_SHAPE),
    _row('breg-f32-1x1-refused', F32, F32, 32, 32, 64, 64, 1, ERR_SHAPE, ksize=1),
    _row('thin-in-f32-residual', F32, F32, 32, 32, 4, 128, 0, IM2COL, 0, flags=RESIDUAL),
    _row('thin-in-bf16-v0', BF16, BF16, 32, 32, 8, 128, 0, IM2COL, 0, variant=0),
    _row('general-strided', BF16, BF16, 32, 32, 128, 128, 0, IM2COL, 0, flags=GENERAL),
    _row('x3', F32, F32, 32, 32, 64, 64, 5, X3, 0),
    _row('x3-1x1', F32, F32, 32, 32, 64, 128, 5, X3_1X1, 0, ksize=1),
    _row('x3-cin-refused', F32, F32, 32, 32, 16, 64, 5, ERR_SHAPE),
    _row('x3-bf16-refused', BF16, BF16, 32, 32, 64, 64, 5, ERR_ARG),
]
