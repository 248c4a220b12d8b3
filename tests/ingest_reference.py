"""The yardstick of the ingest tests: ATen's antialiased bilinear resize on the CPU (what torchvision's
``Resize(antialias=True)`` runs on a tensor), applied per image to the cropped (and flipped) ``u8 / 255``.

The bound is not a constant.  It is the reference's OWN fp32 error on the same input -- ``max |interpolate_fp32 -
interpolate_fp64|``, which grows with the number of taps (2.7e-8 for 1x1 -> 16, 1e-7..3e-7 at photo sizes, 1.2e-6 at a 2048x
reduction) -- times 4 (the kernel sums in another order and computes its weights in registers: both a handful of fp32 roundings
on values <= 1), with an absolute floor of 2e-7."""
import numpy as np
import torch
import torch.nn.functional as F

FACTOR, FLOOR = 4.0, 2e-7


def resize(u8_hwc: np.ndarray, size, box=None, flip=False, dtype=torch.float64) -> torch.Tensor:
    """[3, S_h, S_w] of one uint8 HWC image: crop ``box`` (x0, y0, bw, bh), / 255, antialiased bilinear, mirror"""
    sh, sw = (size, size) if isinstance(size, int) else size
    x0, y0, bw, bh = box if box is not None else (0, 0, u8_hwc.shape[1], u8_hwc.shape[0])
    x = torch.from_numpy(np.ascontiguousarray(u8_hwc[y0:y0 + bh, x0:x0 + bw])).permute(2, 0, 1)[None].to(dtype) / 255
    y = F.interpolate(x, size=(sh, sw), mode='bilinear', align_corners=False, antialias=True)[0]
    return y.flip(-1) if flip else y


def reference_and_bound(u8_hwc, size, box=None, flip=False):
    """(fp64 reference [3, S_h, S_w], allowed max abs error of an fp32 implementation, the reference's own fp32 error)"""
    r64 = resize(u8_hwc, size, box, flip, torch.float64)
    own = float((resize(u8_hwc, size, box, flip, torch.float32).double() - r64).abs().max())
    return r64, max(FACTOR * own, FLOOR), own
