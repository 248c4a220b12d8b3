"""Float64 restatement of the FID Inception-v3 (the spec in the header of vqvae-vqgan-pytorch-lightning_amd/fid.py), in plain
torch, independent of the package: the input transform, the layer table with BatchNorm as written (not folded), and the
Frechet distance in the two published forms (pytorch-fid: ``scipy.linalg.sqrtm``; torchmetrics: ``eigvals(S1 S2)``).
``walk`` gives the shape of every conv of the table for a given input size (the counts of tests/test_fid_cpu.py)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

C7 = (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192))
PF = (('Mixed_5b', 32), ('Mixed_5c', 64), ('Mixed_5d', 64))


# ---------------------------------------------------------------------------------------------- table
class _Walker:
    """runs the table either on tensors (``run``) or on shapes only (``walk``): both share the block definitions below"""

    def __init__(self, sd=None):
        self.sd = sd
        self.convs = []

    # a "map" is either an NCHW float64 tensor or a (c, h, w) shape
    def conv(self, name, x, cin, cout, k=(1, 1), stride=1, pad=(0, 0)):
        if isinstance(x, tuple):
            c, h, w = x
            assert c == cin, (name, c, cin)
            oh, ow = (h + 2 * pad[0] - k[0]) // stride + 1, (w + 2 * pad[1] - k[1]) // stride + 1
            self.convs.append(dict(name=name, cin=cin, cout=cout, kh=k[0], kw=k[1], stride=stride, ph=pad[0], pw=pad[1],
                                   h=h, w=w, oh=oh, ow=ow))
            return (cout, oh, ow)
        sd = self.sd
        y = F.conv2d(x, sd[f'{name}.conv.weight'].to(x), stride=stride, padding=pad)
        mean, var = sd[f'{name}.bn.running_mean'].to(x), sd[f'{name}.bn.running_var'].to(x)
        gamma, beta = sd[f'{name}.bn.weight'].to(x), sd[f'{name}.bn.bias'].to(x)
        y = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + 1e-3) * gamma[None, :, None, None] \
            + beta[None, :, None, None]
        return F.relu(y)

    @staticmethod
    def maxpool(x, stride=2, pad=0):
        if isinstance(x, tuple):
            c, h, w = x
            return (c, (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1)
        return F.max_pool2d(x, 3, stride, pad)

    @staticmethod
    def avgpool(x):
        if isinstance(x, tuple):
            return x
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)

    @staticmethod
    def cat(parts):
        if isinstance(parts[0], tuple):
            assert all(p[1:] == parts[0][1:] for p in parts)
            return (sum(p[0] for p in parts),) + parts[0][1:]
        return torch.cat(parts, 1)

    def network(self, x):
        """input (3 or 4 channels, 299 x 299) -> the last 2048-channel map; ``self.totals`` records each block's channels"""
        cv, cat = self.conv, self.cat
        c_in = x[0] if isinstance(x, tuple) else x.shape[1]
        x = cv('Conv2d_1a_3x3', x, c_in, 32, (3, 3), 2)
        x = cv('Conv2d_2a_3x3', x, 32, 32, (3, 3))
        x = cv('Conv2d_2b_3x3', x, 32, 64, (3, 3), 1, (1, 1))
        x = self.maxpool(x)
        x = cv('Conv2d_3b_1x1', x, 64, 80)
        x = cv('Conv2d_4a_3x3', x, 80, 192, (3, 3))
        x = self.maxpool(x)
        self.totals = [192]
        c = 192
        for blk, pf in PF:
            b1 = cv(f'{blk}.branch1x1', x, c, 64)
            b5 = cv(f'{blk}.branch5x5_2', cv(f'{blk}.branch5x5_1', x, c, 48), 48, 64, (5, 5), 1, (2, 2))
            b3 = cv(f'{blk}.branch3x3dbl_1', x, c, 64)
            b3 = cv(f'{blk}.branch3x3dbl_2', b3, 64, 96, (3, 3), 1, (1, 1))
            b3 = cv(f'{blk}.branch3x3dbl_3', b3, 96, 96, (3, 3), 1, (1, 1))
            bp = cv(f'{blk}.branch_pool', self.avgpool(x), c, pf)
            x = cat([b1, b5, b3, bp])
            c = 224 + pf
            self.totals.append(c)
        b3 = cv('Mixed_6a.branch3x3', x, 288, 384, (3, 3), 2)
        bd = cv('Mixed_6a.branch3x3dbl_1', x, 288, 64)
        bd = cv('Mixed_6a.branch3x3dbl_2', bd, 64, 96, (3, 3), 1, (1, 1))
        bd = cv('Mixed_6a.branch3x3dbl_3', bd, 96, 96, (3, 3), 2)
        x = cat([b3, bd, self.maxpool(x)])
        self.totals.append(768)
        for blk, c7 in C7:
            b1 = cv(f'{blk}.branch1x1', x, 768, 192)
            b7 = cv(f'{blk}.branch7x7_1', x, 768, c7)
            b7 = cv(f'{blk}.branch7x7_2', b7, c7, c7, (1, 7), 1, (0, 3))
            b7 = cv(f'{blk}.branch7x7_3', b7, c7, 192, (7, 1), 1, (3, 0))
            bd = cv(f'{blk}.branch7x7dbl_1', x, 768, c7)
            bd = cv(f'{blk}.branch7x7dbl_2', bd, c7, c7, (7, 1), 1, (3, 0))
            bd = cv(f'{blk}.branch7x7dbl_3', bd, c7, c7, (1, 7), 1, (0, 3))
            bd = cv(f'{blk}.branch7x7dbl_4', bd, c7, c7, (7, 1), 1, (3, 0))
            bd = cv(f'{blk}.branch7x7dbl_5', bd, c7, 192, (1, 7), 1, (0, 3))
            bp = cv(f'{blk}.branch_pool', self.avgpool(x), 768, 192)
            x = cat([b1, b7, bd, bp])
            self.totals.append(768)
        b3 = cv('Mixed_7a.branch3x3_2', cv('Mixed_7a.branch3x3_1', x, 768, 192), 192, 320, (3, 3), 2)
        b7 = cv('Mixed_7a.branch7x7x3_1', x, 768, 192)
        b7 = cv('Mixed_7a.branch7x7x3_2', b7, 192, 192, (1, 7), 1, (0, 3))
        b7 = cv('Mixed_7a.branch7x7x3_3', b7, 192, 192, (7, 1), 1, (3, 0))
        b7 = cv('Mixed_7a.branch7x7x3_4', b7, 192, 192, (3, 3), 2)
        x = cat([b3, b7, self.maxpool(x)])
        self.totals.append(1280)
        c = 1280
        for blk in ('Mixed_7b', 'Mixed_7c'):
            b1 = cv(f'{blk}.branch1x1', x, c, 320)
            b3 = cv(f'{blk}.branch3x3_1', x, c, 384)
            b3 = cat([cv(f'{blk}.branch3x3_2a', b3, 384, 384, (1, 3), 1, (0, 1)),
                      cv(f'{blk}.branch3x3_2b', b3, 384, 384, (3, 1), 1, (1, 0))])
            bd = cv(f'{blk}.branch3x3dbl_1', x, c, 448)
            bd = cv(f'{blk}.branch3x3dbl_2', bd, 448, 384, (3, 3), 1, (1, 1))
            bd = cat([cv(f'{blk}.branch3x3dbl_3a', bd, 384, 384, (1, 3), 1, (0, 1)),
                      cv(f'{blk}.branch3x3dbl_3b', bd, 384, 384, (3, 1), 1, (1, 0))])
            pooled = self.avgpool(x) if blk == 'Mixed_7b' else self.maxpool(x, 1, 1)
            bp = cv(f'{blk}.branch_pool', pooled, c, 192)
            x = cat([b1, b3, bd, bp])
            c = 2048
            self.totals.append(2048)
        return x


def walk(size: int = 299, cin: int = 3):
    """(list of conv dicts with their map sizes, final (c, h, w), channel totals after the stem and each block)"""
    w = _Walker()
    out = w.network((cin, size, size))
    return w.convs, out, w.totals


def state_dict_shapes():
    """key -> shape of every key the table reads, in the published (torchvision Inception3) naming"""
    convs, _, _ = walk()
    out = {}
    for c in convs:
        out[f'{c["name"]}.conv.weight'] = (c['cout'], c['cin'], c['kh'], c['kw'])
        for p in ('weight', 'bias', 'running_mean', 'running_var'):
            out[f'{c["name"]}.bn.{p}'] = (c['cout'],)
    return out


def random_state_dict(seed: int = 0, extras: bool = True):
    """He-scaled conv weights and random BatchNorm statistics in the published naming (plus fc / AuxLogits /
    num_batches_tracked keys the loader must ignore).  The BN scale keeps activations of order one through the 94 layers."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for c in walk()[0]:
        fan_in = c['cin'] * c['kh'] * c['kw']
        n = c['name']
        sd[f'{n}.conv.weight'] = torch.randn(c['cout'], c['cin'], c['kh'], c['kw'], generator=g) * (2.0 / fan_in) ** 0.5
        sd[f'{n}.bn.weight'] = 0.8 + 0.4 * torch.rand(c['cout'], generator=g)
        sd[f'{n}.bn.bias'] = 0.2 * torch.randn(c['cout'], generator=g)
        sd[f'{n}.bn.running_mean'] = 0.1 * torch.randn(c['cout'], generator=g)
        sd[f'{n}.bn.running_var'] = 0.5 + torch.rand(c['cout'], generator=g)
        if extras:
            sd[f'{n}.bn.num_batches_tracked'] = torch.tensor(7)
    if extras:
        sd['fc.weight'] = torch.randn(1008, 2048, generator=g) * 0.01
        sd['fc.bias'] = torch.zeros(1008)
        sd['AuxLogits.conv0.conv.weight'] = torch.zeros(128, 768, 1, 1)
    return sd


# ---------------------------------------------------------------------------------------------- input transform
def quantize(x: torch.Tensor) -> torch.Tensor:
    """ConvertImageDtype(torch.uint8) after a clamp: trunc(x * 255.999f), computed in fp32 exactly as the spec says"""
    q = x.float().clamp(0, 1) * np.float32(255.999)
    return q.trunc()


def resize_tf1(q: torch.Tensor, size: int = 299) -> torch.Tensor:
    """TF1 bilinear resize of [B, C, H, W]: source coordinates in fp32 (dst * fp32(in / out)), interpolation in float64"""
    def grid(n_in):
        src = torch.arange(size, dtype=torch.float32) * np.float32(n_in / size)
        i0 = src.floor().long().clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
        return i0, i1, (src - i0.float()).double()
    h, w = q.shape[-2:]
    y0, y1, ty = grid(h)
    x0, x1, tx = grid(w)
    q = q.double()
    tl, tr = q[..., y0, :][..., x0], q[..., y0, :][..., x1]
    bl, br = q[..., y1, :][..., x0], q[..., y1, :][..., x1]
    tx, ty = tx.to(q.device), ty.to(q.device)[:, None]
    top = tl + (tr - tl) * tx
    bot = bl + (br - bl) * tx
    return top + (bot - top) * ty


def preprocess(x: torch.Tensor) -> torch.Tensor:
    """[B, 3, H, W] in [0, 1] -> [B, 3, 299, 299] float64"""
    return (resize_tf1(quantize(x)) - 128.0) / 128.0


def features(images: torch.Tensor, sd: dict, device='cpu') -> torch.Tensor:
    """[B, 3, H, W] -> [B, 2048] float64 features of the whole network"""
    x = preprocess(images.to(device))
    w = _Walker({k: v.to(device, torch.float64) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()})
    return w.network(x).mean(dim=(2, 3))


# ---------------------------------------------------------------------------------------------- Frechet distance
def stats(f):
    f = np.asarray(f, dtype=np.float64)
    return f.mean(0), np.cov(f, rowvar=False)


def fid_sqrtm(mu1, s1, mu2, s2):
    """pytorch-fid ``calculate_frechet_distance``: scipy.linalg.sqrtm of S1 S2, its real part"""
    import scipy.linalg
    diff = mu1 - mu2
    covmean, _ = scipy.linalg.sqrtm(s1.dot(s2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(s1.shape[0]) * 1e-6
        covmean = scipy.linalg.sqrtm((s1 + offset).dot(s2 + offset))
    covmean = np.real(covmean)
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))


def fid_eigvals(mu1, s1, mu2, s2):
    """torchmetrics ``_compute_fid``: the square roots of the eigenvalues of S1 S2, real part summed"""
    mu1, s1, mu2, s2 = (torch.as_tensor(t, dtype=torch.float64) for t in (mu1, s1, mu2, s2))
    a = (mu1 - mu2).square().sum()
    b = s1.trace() + s2.trace()
    c = torch.linalg.eigvals(s1 @ s2).sqrt().real.sum()
    return float(a + b - 2 * c)
