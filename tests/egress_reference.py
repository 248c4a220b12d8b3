"""The yardstick of the egress tests: the uint8 rule of ``torchvision.utils.save_image`` and the layout of
``torchvision.utils.make_grid``, restated from their documentation (torchvision is not a dependency) in CPU torch and plain
loops.

The rule is integer-valued and fully specified in fp32 with every operation rounded on its own, so an implementation is
compared bit for bit, with no tolerance:
    'sym'  (the model's (-1,1)):  t = clip(x * 0.5 + 0.5, 0, 1)
    'unit' ([0,1]):               t = clip(x, 0, 1)
    q = uint8(floor(t * 255 + 0.5))
bf16 is widened exactly first; NaN gives 0 (stated here: ``torch.clip`` passes NaN on and its conversion to uint8 is undefined)."""
import torch


def quantise(x: torch.Tensor, value_range: str) -> torch.Tensor:
    """uint8 of a tensor of any shape, on the CPU, separate fp32 ops"""
    x = x.detach().cpu().float()
    if value_range == 'sym':
        t = torch.clip(x * 0.5 + 0.5, 0, 1)
    elif value_range == 'unit':
        t = torch.clip(x, 0, 1)
    else:
        raise ValueError(value_range)
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t)
    return t.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)


def egress(src: torch.Tensor, value_range: str) -> torch.Tensor:
    """[N,C>=3,H,W] (any layout) -> uint8 [N,H,W,3]"""
    return quantise(src[:, :3], value_range).permute(0, 2, 3, 1).contiguous()


def make_grid(images_u8: torch.Tensor, nrow: int, padding: int = 2, pad_value: int = 0) -> torch.Tensor:
    """``make_grid`` of uint8 [K,H,W,3] images -> uint8 [H_g,W_g,3], by plain loops: cols = min(nrow, K), rows = ceil(K / cols),
    image k at cell (k // cols, k % cols), a cell's top-left pixel at (padding + cell_y * (H + padding), padding + cell_x *
    (W + padding)); everything else is ``pad_value``."""
    k, h, w, _ = images_u8.shape
    cols = min(nrow, k)
    rows = -(-k // cols)
    grid = torch.full((rows * (h + padding) + padding, cols * (w + padding) + padding, 3), pad_value, dtype=torch.uint8)
    i = 0
    for cy in range(rows):
        for cx in range(cols):
            if i >= k:
                break
            y0, x0 = padding + cy * (h + padding), padding + cx * (w + padding)
            for y in range(h):
                grid[y0 + y, x0:x0 + w] = images_u8[i, y]
            i += 1
    return grid


def image_grid(sources, nrow: int, padding: int = 2, pad_value: int = 0, value_ranges='sym') -> torch.Tensor:
    """the grid of batches concatenated in order (the reference's ``pack(..., '* c h w')`` + ``make_grid``)"""
    ranges = [value_ranges] * len(sources) if isinstance(value_ranges, str) else list(value_ranges)
    return make_grid(torch.cat([egress(s, r) for s, r in zip(sources, ranges)]), nrow, padding, pad_value)
