"""The weight-gradient dispatch table shared by tests/test_wgrad_plan.py (CPU: the plan query) and tests/test_gpu_wgrad_plan.py
(GPU: every launchable row through its entry point).

Each row is a problem, the entry point it goes through (``op``), the state it is planned under, and what the one-layer
launcher takes for it.  The expectations were derived by READING the launcher as it stood before the plan function existed
(csrc/conv_wgrad.hip::wgrad_general and the entry points around it, csrc/conv_x3.hip::launch_conv3x3_wgrad_x3), in this order:

  pooled-dy / ups-phase / pooled-dy-phase entries: bf16, h % 8, w % 16, cin % 64, cout % 64, WGMX slot on, no variant 0,
      WGRAD_BLOCKS == 0, WGRAD_NO_PW16 == 0 (the two phase entries: not in deterministic mode; pooled-dy-phase: UPS_MERGE on), else
      VQK_ERR_SHAPE.  pair-operand entry (fold): ups in {0, 1} else VQK_ERR_ARG, cin % 64, cout % 64 else VQK_ERR_SHAPE, and
      behind the geometry the same list with the map's h % 8, w % 16, never in deterministic mode.
  mode in {0, 1}, stride in {1, 2}, pad >= 0 else VQK_ERR_ARG; dtype, n, map, ksize in {1, 3}, cin % (4 fp32 | 8 bf16): the
      geometry builder's statuses; cout % (4 | 8) else VQK_ERR_SHAPE.  plain = stride 1, pad ksize / 2, output map = input << ups.
  plain bf16 3x3, h % 8, w % 8, no variant 0:
      patches 8x16 when w % 16 and WGRAD_NO_PW16 == 0, else 8x8; tiles = ceil(cout / 64) * ceil(cin / 64) (fold: 3 * (cout / 64) *
      (cin / 64) of the true channels);  halo rule: s = WGRAD_BLOCKS > 0 ? ceil(WGRAD_BLOCKS / tiles)
      : min(round(sqrt(0.16 * pixels / tiles)), ceil(cap / tiles)), cap = the thread's block cap or 512; s <= ceil(patches / (2 for
      8x16 | 4 for 8x8)); deterministic: s = 1; pps = ceil(patches / s), s = ceil(patches / pps).
      8x16 patches, cin % 64, cout % 64, WGMX on, WGRAD_BLOCKS == 0 -> matrix/auxiliary-wave kernel with its own rule:
      s = min(round(sqrt(0.08 * pixels / tiles)), ceil(capm / tiles), ceil(patches / 4)), capm = max((cap / 2 - COMM_CUS) / nph,
      tiles), nph = 4 for the merged phase launch; deterministic: s <= workspace bytes / (tiles * 64*9*64*4), and >= 2 splits go
      through the workspace (ordered); pps, s as above.  UPS_MERGE = 0: four launches, nph = 1.
      an op other than plain that got here -> VQK_ERR_SHAPE;  8x16, cin % 64, cout % 64, WGRAD_NO_P16K == 0 -> p16;  8x16 -> halo16;
      else halo8.
  plain fp32 3x3, no upsample, not deterministic, no variant 0, w % 4, a staged row block fits 64 KiB of LDS (rows = the largest of
      8, 4, 2, 1 dividing h with (rows + 2) * (w + 2) * 16 <= 65536): cin == 4, cout in {64, 128, 256} -> thin cin-4; cout == 4, cin
      in {64, 128, 256} -> thin cout-4; blocks = n * h / rows.
  else the general kernels: tiles = ceil(cout / 128) * ceil(cin / 128) * k * k, kp = 32 fp32 | 64 bf16, s = min(ceil((512 =
      WGRAD_GEN_BLOCKS for the bf16 1x1 double-buffered form | 2048) / tiles), ceil(pixels / (4 * kp))); deterministic: s <=
      workspace bytes / (4 * dW elements), and >= 2 splits use private copies + an ordered reduce; pps = ceil(pixels / s) rounded up
      to kp, s = ceil(pixels / pps).
  fp32 split-product entry (x3): ups in {0, 1, 2} else VQK_ERR_ARG; deterministic or variant 0 -> VQK_ERR_SHAPE; phase form for ups
      2 (h_in % 16, w_in % 16 else VQK_ERR_SHAPE; grid = the pooled map) and for ups 1 with X3_WGRAD_PHASE on, h_in % 8, w_in % 8
      (grid = the input map); else the tap form on the output map; cin % 64, cout % 64, grid h % 8, w % 8 else VQK_ERR_SHAPE;
      tiles = (cout / 64) * (cin / 64), 8x8 patches, phases P = 4 | 1: s = min(floor(sqrt(0.32 * pixels * P / tiles) / P + 0.5),
      ceil(cap' / (tiles * P)), ceil(patches / 4)), cap' = cap * 150 / 100 in phase form; pps, s as above.

None of the issue's anchor rows (the first four) contradicts that reading.
"""
import collections

F32, BF16 = 0, 1                                                 # include/vqk.h dtype codes
ERR_SHAPE, ERR_DTYPE, ERR_ARG = -1, -2, -5
PLAIN, POOLED_DY, UPS_PHASE, POOLED_DY_PHASE, FOLD, X3_OP = range(6)     # include/vqk.h: ops of vqk_conv_wgrad_plan
# ... and its form ids
(MX, MX_POOLED_DY, MX_UPS_PHASE, MX_POOLED_DY_PHASE, MX_FOLD, P16, HALO16, HALO8, THIN_CIN4, THIN_COUT4, GENERAL_F32, GENERAL_BF16,
 GENERAL_DB, X3, X3_UPS_PHASE, X3_POOLED_PHASE) = range(16)
NAMES = {MX: 'conv3x3_wgrad_mx_kernel<bf16>', MX_POOLED_DY: 'conv3x3_wgrad_mx_kernel<bf16>', MX_UPS_PHASE: 'conv3x3_wgrad_mx_kernel<bf16>',
         MX_POOLED_DY_PHASE: 'conv3x3_wgrad_mx_kernel<bf16>', MX_FOLD: 'conv3x3_wgrad_mx_kernel<f32 as 3 x bf16>',
         P16: 'conv3x3_wgrad_p16_kernel<bf16>', HALO16: 'conv3x3_wgrad_halo_kernel<bf16>', HALO8: 'conv3x3_wgrad_halo_kernel<bf16>',
         THIN_CIN4: 'conv3x3_wgrad_thin_f32_kernel (HBM)', THIN_COUT4: 'conv3x3_wgrad_thin_f32_kernel (HBM)',
         GENERAL_F32: 'conv_wgrad_kernel<f32>', GENERAL_BF16: 'conv_wgrad_kernel<bf16>', GENERAL_DB: 'conv_wgrad_db_kernel<bf16>',
         X3: 'conv3x3_wgrad_x3_kernel<f32 as 3 x bf16>', X3_UPS_PHASE: 'conv3x3_wgrad_x3_kernel<f32 as 3 x bf16>',
         X3_POOLED_PHASE: 'conv3x3_wgrad_x3_kernel<f32 as 3 x bf16>'}
WS = 1 << 20                                                     # the deterministic workspace of the rows that have one: 1 MiB

Row = collections.namedtuple('Row', 'name op dtype n h w cin cout ksize stride pad ups h_out w_out variant tuning det cap '
                                    'form tiles splits pps launches ordered')


def _row(name, op, dtype, n, h, w, cin, cout, form, tiles=0, splits=1, pps=0, launches=1, ordered=0, ksize=3, stride=1, pad=None,
         ups=0, h_out=None, w_out=None, variant=-1, tuning=None, det=None, cap=0):
    """h, w: the entry point's own (the input map); det: None = default mode, else the deterministic workspace's bytes"""
    return Row(name, op, dtype, n, h, w, cin, cout, ksize, stride, ksize >> 1 if pad is None else pad, ups,
               h << (ups == 1) if h_out is None else h_out, w << (ups == 1) if w_out is None else w_out, variant, tuning or {}, det, cap,
               form, tiles, splits, pps, launches, ordered)


ROWS = [
    # ---- the issue's anchor rows: bf16 (the last: fp32 tensors), plain 3x3, n = 2, 64 -> 64
    # 16x32: 8 patches of 8x16, 1024 pixels; mx: min(round(sqrt(81.9)) = 9, 256, ceil(8 / 4) = 2) = 2 splits of 4
    _row('mx', PLAIN, BF16, 2, 16, 32, 64, 64, MX, 1, 2, 4),
    # the same with the WGMX slot off: halo rule min(round(sqrt(163.8)) = 13, 512, ceil(8 / 2) = 4) = 4 splits of 2
    _row('p16-wgmx-off', PLAIN, BF16, 2, 16, 32, 64, 64, P16, 1, 4, 2, tuning={'WGMX': 0}),
    # 16x24: no 8x16 patches; 12 patches of 8x8, 768 pixels: min(round(sqrt(122.9)) = 11, 512, ceil(12 / 4) = 3) = 3 splits of 4
    _row('halo8', PLAIN, BF16, 2, 16, 24, 64, 64, HALO8, 1, 3, 4),
    # fp32 tensors 16x24: 12 patches of 8x8: min(round(sqrt(245.8)) = 16, 512, 3) = 3 splits of 4
    _row('x3', X3_OP, F32, 2, 16, 24, 64, 64, X3, 1, 3, 4),
    # ---- the matrix/auxiliary-wave kernel and its operand modes, split and unsplit (n = 1: 4 patches -> ceil(4 / 4) = 1 split)
    _row('mx-unsplit', PLAIN, BF16, 1, 16, 32, 64, 64, MX, 1, 1, 4),
    _row('mx-8-tiles', PLAIN, BF16, 2, 16, 32, 128, 256, MX, 8, 2, 4),                   # round(sqrt(10.2)) = 3 > 2
    # 64x64: 64 patches, 8192 pixels, 16 tiles: min(round(sqrt(41)) = 6, ceil(256 / 16) = 16, 16) = 6 -> pps 11, 6 splits
    _row('mx-model-rule', PLAIN, BF16, 2, 64, 64, 256, 256, MX, 16, 6, 11),
    _row('mx-ups-tap', PLAIN, BF16, 2, 8, 16, 64, 64, MX, 1, 2, 4, ups=1),               # output map 16x32: the tap form
    # block cap 2: capm = max((2 / 2) / 1, 1 tile) = 1 -> one split of all 8 patches
    _row('mx-block-cap', PLAIN, BF16, 2, 16, 32, 64, 64, MX, 1, 1, 8, cap=2),
    _row('mx-pooled-dy', POOLED_DY, BF16, 2, 16, 32, 64, 64, MX_POOLED_DY, 1, 2, 4),
    _row('mx-pooled-dy-unsplit', POOLED_DY, BF16, 1, 16, 32, 64, 64, MX_POOLED_DY, 1, 1, 4),
    # merged phases: capm = (256 / 4) = 64; min(9, 64, 2) = 2 splits per phase
    _row('mx-ups-phase', UPS_PHASE, BF16, 2, 16, 32, 64, 64, MX_UPS_PHASE, 1, 2, 4),
    _row('mx-ups-phase-unsplit', UPS_PHASE, BF16, 1, 16, 32, 64, 64, MX_UPS_PHASE, 1, 1, 4),
    _row('mx-ups-phase-unmerged', UPS_PHASE, BF16, 2, 16, 32, 64, 64, MX_UPS_PHASE, 1, 2, 4, launches=4, tuning={'UPS_MERGE': 0}),
    # roles swapped, 64 -> 128 on the pooled 16x32 grid: 2 tiles; min(round(sqrt(41)) = 6, ceil(64 / 2), 2) = 2
    _row('mx-pooled-dy-phase', POOLED_DY_PHASE, BF16, 2, 16, 32, 64, 128, MX_POOLED_DY_PHASE, 2, 2, 4),
    _row('mx-pooled-dy-phase-unsplit', POOLED_DY_PHASE, BF16, 1, 16, 32, 64, 128, MX_POOLED_DY_PHASE, 2, 1, 4),
    # pair operands: 3 tile classes; min(round(sqrt(27.3)) = 5, ceil(256 / 3), 2) = 2
    _row('mx-fold', FOLD, F32, 2, 16, 32, 64, 64, MX_FOLD, 3, 2, 4),
    _row('mx-fold-unsplit', FOLD, F32, 1, 16, 32, 64, 64, MX_FOLD, 3, 1, 4),
    _row('mx-fold-ups', FOLD, F32, 2, 8, 16, 64, 64, MX_FOLD, 3, 2, 4, ups=1),
    # ---- p16 / halo kernels
    _row('p16-unsplit', PLAIN, BF16, 1, 8, 32, 64, 64, P16, 1, 1, 2, tuning={'WGMX': 0}),                   # 2 patches: ceil(2 / 2) = 1
    _row('p16-wgrad-blocks', PLAIN, BF16, 2, 16, 32, 64, 64, P16, 1, 2, 4, tuning={'WGRAD_BLOCKS': 2}),     # 2 blocks / 1 tile
    _row('halo16', PLAIN, BF16, 2, 16, 32, 32, 64, HALO16, 1, 4, 2),                                        # cin 32: no whole tile
    _row('halo16-unsplit', PLAIN, BF16, 1, 8, 32, 32, 64, HALO16, 1, 1, 2),
    _row('halo16-no-p16k', PLAIN, BF16, 2, 16, 32, 64, 64, HALO16, 1, 4, 2, tuning={'WGMX': 0, 'WGRAD_NO_P16K': 1}),
    _row('halo8-unsplit', PLAIN, BF16, 1, 8, 24, 64, 64, HALO8, 1, 1, 3),                                   # 3 patches: ceil(3 / 4) = 1
    # WGRAD_NO_PW16: 16 patches of 8x8: min(13, 512, ceil(16 / 4) = 4) = 4 splits of 4 (and no matrix/auxiliary-wave kernel)
    _row('halo8-no-pw16', PLAIN, BF16, 2, 16, 32, 64, 64, HALO8, 1, 4, 4, tuning={'WGRAD_NO_PW16': 1}),
    # ---- fp32 thin forms: rows = 8, 2 * 16 / 8 = 4 blocks
    _row('thin-cin4', PLAIN, F32, 2, 16, 32, 4, 64, THIN_CIN4, 4, 1, 8),
    _row('thin-cout4', PLAIN, F32, 2, 16, 32, 64, 4, THIN_COUT4, 4, 1, 8),
    # the LDS bound: w = 404: 10 * 406 * 16 = 64960 <= 65536, 8 rows; w = 408: 10 * 410 * 16 = 65600 > 65536, 4 rows (39360)
    _row('thin-cin4-w404', PLAIN, F32, 1, 8, 404, 4, 64, THIN_CIN4, 1, 1, 8),
    _row('thin-cin4-w408', PLAIN, F32, 1, 8, 408, 4, 64, THIN_CIN4, 2, 1, 4),
    # ... excluded in deterministic mode and by the hook: general fp32, 9 tiles, min(ceil(2048 / 9), ceil(1024 / 128) = 8) = 8 x 128
    # pixels; deterministic: 1 MiB / (2304 * 4) = 113 copies fit
    _row('thin-cin4-det', PLAIN, F32, 2, 16, 32, 4, 64, GENERAL_F32, 9, 8, 128, launches=2, ordered=1, det=WS),
    _row('thin-cin4-v0', PLAIN, F32, 2, 16, 32, 4, 64, GENERAL_F32, 9, 8, 128, variant=0),
    _row('thin-ups-general', PLAIN, F32, 2, 8, 16, 4, 64, GENERAL_F32, 9, 8, 128, ups=1),
    # ---- general kernels
    _row('general-f32', PLAIN, F32, 2, 16, 16, 64, 64, GENERAL_F32, 9, 4, 128),                             # ceil(512 / 128) = 4
    _row('general-f32-unsplit', PLAIN, F32, 1, 8, 16, 64, 64, GENERAL_F32, 9, 1, 128),
    _row('general-bf16-v0', PLAIN, BF16, 2, 16, 32, 64, 64, GENERAL_BF16, 9, 4, 256, variant=0),            # ceil(1024 / 256) = 4
    _row('general-bf16-unsplit', PLAIN, BF16, 1, 16, 16, 64, 64, GENERAL_BF16, 9, 1, 256, variant=0),
    # 12x12: no 8-row patches; 288 pixels: ceil(288 / 256) = 2 splits, pps ceil(144 / 64) * 64 = 192
    _row('general-bf16-12x12', PLAIN, BF16, 2, 12, 12, 64, 64, GENERAL_BF16, 9, 2, 192),
    # stride 2, pad 1: 16x16 -> 8x8, 128 pixels: one split
    _row('general-bf16-strided', PLAIN, BF16, 2, 16, 16, 64, 64, GENERAL_BF16, 9, 1, 128, stride=2, h_out=8, w_out=8),
    _row('general-db', PLAIN, BF16, 2, 16, 32, 64, 64, GENERAL_DB, 1, 4, 256, ksize=1),                     # min(512, ceil(1024 / 256))
    _row('general-db-unsplit', PLAIN, BF16, 1, 16, 16, 64, 64, GENERAL_DB, 1, 1, 256, ksize=1),
    _row('general-db-gen-blocks', PLAIN, BF16, 2, 16, 32, 64, 64, GENERAL_DB, 1, 2, 512, ksize=1, tuning={'WGRAD_GEN_BLOCKS': 2}),
    # ---- deterministic mode.  mx: 1 MiB / (1 tile * 147456) = 7 partial tiles fit: 2 splits through the workspace + reduce
    _row('mx-det', PLAIN, BF16, 2, 16, 32, 64, 64, MX, 1, 2, 4, launches=2, ordered=1, det=WS),
    _row('mx-det-one-split', PLAIN, BF16, 1, 16, 32, 64, 64, MX, 1, 1, 4, det=WS),                          # no workspace use
    _row('mx-det-small-ws', PLAIN, BF16, 2, 16, 32, 64, 64, MX, 1, 1, 8, det=147456),                       # one partial tile fits
    _row('mx-pooled-dy-det', POOLED_DY, BF16, 2, 16, 32, 64, 64, MX_POOLED_DY, 1, 2, 4, launches=2, ordered=1, det=WS),
    _row('p16-det', PLAIN, BF16, 2, 16, 32, 64, 64, P16, 1, 1, 8, tuning={'WGMX': 0}, det=WS),              # one block per tile
    # general: private copies of dW (4096 * 4 bytes each: 64 fit) + ordered reduce; without a workspace: unsplit
    _row('general-db-det', PLAIN, BF16, 2, 16, 32, 64, 64, GENERAL_DB, 1, 4, 256, launches=2, ordered=1, ksize=1, det=WS),
    _row('general-db-det-no-ws', PLAIN, BF16, 2, 16, 32, 64, 64, GENERAL_DB, 1, 1, 1024, ksize=1, det=0),
    _row('general-bf16-v0-det', PLAIN, BF16, 2, 16, 32, 64, 64, GENERAL_BF16, 9, 4, 256, launches=2, ordered=1, variant=0, det=WS),
    _row('ups-phase-det-refused', UPS_PHASE, BF16, 2, 16, 32, 64, 64, ERR_SHAPE, det=WS),
    _row('pooled-dy-phase-det-refused', POOLED_DY_PHASE, BF16, 2, 16, 32, 64, 128, ERR_SHAPE, det=WS),
    _row('fold-det-refused', FOLD, F32, 2, 16, 32, 64, 64, ERR_SHAPE, det=WS),
    _row('x3-det-refused', X3_OP, F32, 2, 16, 24, 64, 64, ERR_SHAPE, det=WS),
    # ---- the split-product kernel.  n = 1 16x16: 4 patches -> 1 split
    _row('x3-unsplit', X3_OP, F32, 1, 16, 16, 64, 64, X3, 1, 1, 4),
    # ups 1 in phase form on the 16x32 input grid: 16 patches, 1024 pixels: min(floor(sqrt(1310.7) / 4 + .5) = 9, 192, 4) = 4
    _row('x3-ups-phase', X3_OP, F32, 2, 16, 32, 64, 64, X3_UPS_PHASE, 1, 4, 4, ups=1),
    _row('x3-ups-phase-unsplit', X3_OP, F32, 2, 8, 16, 64, 64, X3_UPS_PHASE, 1, 1, 4, ups=1),               # 4 patches
    # X3_WGRAD_PHASE = 0: the tap form on the 16x32 output map: min(round(sqrt(327.7)) = 18, 512, ceil(16 / 4)) = 4
    _row('x3-ups-tap', X3_OP, F32, 2, 8, 16, 64, 64, X3, 1, 4, 4, ups=1, tuning={'X3_WGRAD_PHASE': 0}),
    # h_in = 12 is no multiple of 8: tap form on the 24x32 output map, 24 patches: min(round(sqrt(491.5)) = 22, 512, 6) = 6
    _row('x3-ups-tap-12x16', X3_OP, F32, 2, 12, 16, 64, 64, X3, 1, 6, 4, ups=1),
    # ups 2: the pooled 16x16 grid of a 32x32 conv: 8 patches, 512 pixels: min(floor(sqrt(655.4) / 4 + .5) = 6, 192, 2) = 2
    _row('x3-pooled-phase', X3_OP, F32, 2, 32, 32, 64, 64, X3_POOLED_PHASE, 1, 2, 4, ups=2),
    _row('x3-pooled-phase-unsplit', X3_OP, F32, 1, 32, 32, 64, 64, X3_POOLED_PHASE, 1, 1, 4, ups=2),
    # ---- refusals
    _row('pooled-dy-f32-refused', POOLED_DY, F32, 2, 16, 32, 64, 64, ERR_SHAPE),
    _row('pooled-dy-w24-refused', POOLED_DY, BF16, 2, 16, 24, 64, 64, ERR_SHAPE),
    _row('pooled-dy-cin32-refused', POOLED_DY, BF16, 2, 16, 32, 32, 64, ERR_SHAPE),
    _row('pooled-dy-wgmx-off-refused', POOLED_DY, BF16, 2, 16, 32, 64, 64, ERR_SHAPE, tuning={'WGMX': 0}),
    _row('pooled-dy-v0-refused', POOLED_DY, BF16, 2, 16, 32, 64, 64, ERR_SHAPE, variant=0),
    _row('ups-phase-wgrad-blocks-refused', UPS_PHASE, BF16, 2, 16, 32, 64, 64, ERR_SHAPE, tuning={'WGRAD_BLOCKS': 8}),
    _row('ups-phase-no-pw16-refused', UPS_PHASE, BF16, 2, 16, 32, 64, 64, ERR_SHAPE, tuning={'WGRAD_NO_PW16': 1}),
    _row('pooled-dy-phase-unmerged-refused', POOLED_DY_PHASE, BF16, 2, 16, 32, 64, 128, ERR_SHAPE, tuning={'UPS_MERGE': 0}),
    _row('fold-ups2-refused', FOLD, F32, 2, 16, 32, 64, 64, ERR_ARG, ups=2),
    _row('fold-cin32-refused', FOLD, F32, 2, 16, 32, 32, 64, ERR_SHAPE),
    _row('fold-w24-refused', FOLD, F32, 2, 16, 24, 64, 64, ERR_SHAPE),
    _row('fold-wgmx-off-refused', FOLD, F32, 2, 16, 32, 64, 64, ERR_SHAPE, tuning={'WGMX': 0}),
    _row('x3-ups3-refused', X3_OP, F32, 2, 16, 24, 64, 64, ERR_ARG, ups=3),
    _row('x3-v0-refused', X3_OP, F32, 2, 16, 24, 64, 64, ERR_SHAPE, variant=0),
    _row('x3-cin32-refused', X3_OP, F32, 2, 16, 24, 32, 64, ERR_SHAPE),
    _row('x3-h12-refused', X3_OP, F32, 2, 12, 24, 64, 64, ERR_SHAPE),
    _row('x3-pooled-24x32-refused', X3_OP, F32, 2, 24, 32, 64, 64, ERR_SHAPE, ups=2),
    _row('stride3-refused', PLAIN, BF16, 2, 16, 32, 64, 64, ERR_ARG, stride=3, h_out=6, w_out=11),
    _row('mode2-refused', PLAIN, BF16, 2, 16, 32, 64, 64, ERR_ARG, ups=2, h_out=16, w_out=32),
    _row('ksize5-refused', PLAIN, BF16, 2, 16, 32, 64, 64, ERR_SHAPE, ksize=5),
    _row('dtype-refused', PLAIN, 7, 2, 16, 32, 64, 64, ERR_DTYPE),
    _row('cin-chunk-refused', PLAIN, BF16, 2, 16, 32, 12, 64, ERR_SHAPE),
    _row('cout-chunk-refused', PLAIN, F32, 2, 16, 32, 64, 6, ERR_SHAPE),
    _row('empty-output-refused', PLAIN, BF16, 2, 16, 32, 64, 64, ERR_SHAPE, stride=2, h_out=0, w_out=16),
]
