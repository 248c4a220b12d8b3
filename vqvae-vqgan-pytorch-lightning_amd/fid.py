"""rFID of the reference's test loop (vqvae/model.py:491-553: torchmetrics ``FrechetInceptionDistance`` fed
``ConvertImageDtype(torch.uint8)`` images) on the HIP kernels of ``csrc/fid.hip``.

Restated here, not imported: the FID variant of Inception-v3 as pytorch-fid (``FIDInceptionA/C/E_1/E_2``) and
torch-fidelity (``FeatureExtractorInceptionV3``) define it, the 2048-feature tap, torch-fidelity's input transform, the
torchvision ``Inception3`` state-dict naming of the published weights file (``pt_inception-2015-12-05-6726825d.pth``) and
torchmetrics' Frechet statistics.  None of those libraries is a dependency: parity on the pretrained weights is UNPINNED
here, as it is for the torchmetrics metrics of ``metrics.py``.  tests/fid_reference.py restates the same spec in float64.

Input: float images [B, 3, H, W] in [0, 1], any H x W, possibly a strided view.
  1. q = trunc(clamp(x, 0, 1) * 255.999f) in fp32 (ConvertImageDtype(torch.uint8); the clamp is a departure that only
     matters for out-of-range input);
  2. TF1 bilinear resize to 299 x 299 (torch-fidelity ``interpolate_bilinear_2d_like_tensorflow1x``, align_corners=False):
     scale = in / out, src = dst * scale, i0 = floor(src), i1 = min(i0 + 1, in - 1), t = src - i0;
     top = tl + (tr - tl) tx, bot = bl + (br - bl) tx, out = top + (bot - top) ty;
  3. (v - 128) / 128.
BasicConv(cin, cout, (kh, kw), stride, (ph, pw)) = conv without bias -> BatchNorm(eps 1e-3, running stats) -> ReLU, the
BatchNorm folded into weight and bias (float64 on the host, then fp32).  avgX = avg_pool2d(3, 1, 1, count_include_pad=False).

  stem       Conv2d_1a_3x3 3->32 3x3 s2, Conv2d_2a_3x3 32->32 3x3, Conv2d_2b_3x3 32->64 3x3 p1, maxpool 3 s2,
             Conv2d_3b_1x1 64->80, Conv2d_4a_3x3 80->192 3x3, maxpool 3 s2                     299->149->147->73->71->35
  Mixed_5b/c/d (A, pool_features 32/64/64): branch1x1 c->64 | branch5x5_1 c->48, _2 48->64 5x5 p2 |
             branch3x3dbl_1 c->64, _2 64->96 3x3 p1, _3 96->96 3x3 p1 | avgX, branch_pool c->pf   35; c 192->256->288->288
  Mixed_6a (B): branch3x3 288->384 3x3 s2 | branch3x3dbl_1 288->64, _2 64->96 p1, _3 96->96 3x3 s2 | maxpool 3 s2
                                                                                                       35->17, 768
  Mixed_6b..e (C, c7 = 128/160/160/192): branch1x1 768->192 | branch7x7_1 768->c7, _2 c7->c7 1x7 p(0,3),
             _3 c7->192 7x1 p(3,0) | branch7x7dbl_1 768->c7, _2 7x1, _3 1x7, _4 7x1, _5 c7->192 1x7 |
             avgX, branch_pool 768->192                                                                17, 768
  Mixed_7a (D): branch3x3_1 768->192, _2 192->320 3x3 s2 | branch7x7x3_1 768->192, _2 1x7, _3 7x1,
             _4 192->192 3x3 s2 | maxpool 3 s2                                                         17->8, 1280
  Mixed_7b (E_1) / Mixed_7c (E_2): branch1x1 c->320 | branch3x3_1 c->384, [_2a 1x3 p(0,1) || _2b 3x1 p(1,0)] |
             branch3x3dbl_1 c->448, _2 448->384 3x3 p1, [_3a 1x3 || _3b 3x1] | pool, branch_pool c->192;
             the pool is avgX in 7b and max 3x3 s1 p1 in 7c                                  8; 1280->2048->2048
  head       global mean over 8 x 8 -> 2048 features (fc unused)
Concat order = the listed branch order.  94 convs, 21.75 M conv weights, 11.42 GFLOP per image.

Frechet distance (torchmetrics): mu = s / n, Sigma = (G - n mu mu^T) / (n - 1) from the fp64 sums s = sum f and
G = F^T F accumulated on the device; FID = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1^1/2 S2 S1^1/2) on the host in
float64 (two ``eigh``, eigenvalues clamped at 0: the eigenvalues of torchmetrics' ``eigvals(S1 S2)``, stable for n < 2048).
"""
from __future__ import annotations

import os
from collections import OrderedDict

import torch

from . import _native

FEATURES = 2048
SIZE = 299
BN_EPS = 1e-3
C7 = {'Mixed_6b': 128, 'Mixed_6c': 160, 'Mixed_6d': 160, 'Mixed_6e': 192}
POOL_FEATURES = {'Mixed_5b': 32, 'Mixed_5c': 64, 'Mixed_5d': 64}
_MAX, _AVG = 0, 1


def conv_specs() -> 'OrderedDict[str, tuple]':
    """name -> (cin, cout, kh, kw, stride, ph, pw) of the 94 BasicConvs, in network order"""
    s = OrderedDict()

    def bc(name, cin, cout, k=(1, 1), stride=1, pad=(0, 0)):
        s[name] = (cin, cout, k[0], k[1], stride, pad[0], pad[1])

    bc('Conv2d_1a_3x3', 3, 32, (3, 3), 2)
    bc('Conv2d_2a_3x3', 32, 32, (3, 3))
    bc('Conv2d_2b_3x3', 32, 64, (3, 3), 1, (1, 1))
    bc('Conv2d_3b_1x1', 64, 80)
    bc('Conv2d_4a_3x3', 80, 192, (3, 3))
    c = 192
    for blk, pf in POOL_FEATURES.items():
        bc(f'{blk}.branch1x1', c, 64)
        bc(f'{blk}.branch5x5_1', c, 48)
        bc(f'{blk}.branch5x5_2', 48, 64, (5, 5), 1, (2, 2))
        bc(f'{blk}.branch3x3dbl_1', c, 64)
        bc(f'{blk}.branch3x3dbl_2', 64, 96, (3, 3), 1, (1, 1))
        bc(f'{blk}.branch3x3dbl_3', 96, 96, (3, 3), 1, (1, 1))
        bc(f'{blk}.branch_pool', c, pf)
        c = 64 + 64 + 96 + pf
    bc('Mixed_6a.branch3x3', 288, 384, (3, 3), 2)
    bc('Mixed_6a.branch3x3dbl_1', 288, 64)
    bc('Mixed_6a.branch3x3dbl_2', 64, 96, (3, 3), 1, (1, 1))
    bc('Mixed_6a.branch3x3dbl_3', 96, 96, (3, 3), 2)
    for blk, c7 in C7.items():
        bc(f'{blk}.branch1x1', 768, 192)
        bc(f'{blk}.branch7x7_1', 768, c7)
        bc(f'{blk}.branch7x7_2', c7, c7, (1, 7), 1, (0, 3))
        bc(f'{blk}.branch7x7_3', c7, 192, (7, 1), 1, (3, 0))
        bc(f'{blk}.branch7x7dbl_1', 768, c7)
        bc(f'{blk}.branch7x7dbl_2', c7, c7, (7, 1), 1, (3, 0))
        bc(f'{blk}.branch7x7dbl_3', c7, c7, (1, 7), 1, (0, 3))
        bc(f'{blk}.branch7x7dbl_4', c7, c7, (7, 1), 1, (3, 0))
        bc(f'{blk}.branch7x7dbl_5', c7, 192, (1, 7), 1, (0, 3))
        bc(f'{blk}.branch_pool', 768, 192)
    bc('Mixed_7a.branch3x3_1', 768, 192)
    bc('Mixed_7a.branch3x3_2', 192, 320, (3, 3), 2)
    bc('Mixed_7a.branch7x7x3_1', 768, 192)
    bc('Mixed_7a.branch7x7x3_2', 192, 192, (1, 7), 1, (0, 3))
    bc('Mixed_7a.branch7x7x3_3', 192, 192, (7, 1), 1, (3, 0))
    bc('Mixed_7a.branch7x7x3_4', 192, 192, (3, 3), 2)
    for blk, c in (('Mixed_7b', 1280), ('Mixed_7c', 2048)):
        bc(f'{blk}.branch1x1', c, 320)
        bc(f'{blk}.branch3x3_1', c, 384)
        bc(f'{blk}.branch3x3_2a', 384, 384, (1, 3), 1, (0, 1))
        bc(f'{blk}.branch3x3_2b', 384, 384, (3, 1), 1, (1, 0))
        bc(f'{blk}.branch3x3dbl_1', c, 448)
        bc(f'{blk}.branch3x3dbl_2', 448, 384, (3, 3), 1, (1, 1))
        bc(f'{blk}.branch3x3dbl_3a', 384, 384, (1, 3), 1, (0, 1))
        bc(f'{blk}.branch3x3dbl_3b', 384, 384, (3, 1), 1, (1, 0))
        bc(f'{blk}.branch_pool', c, 192)
    return s


def expected_keys() -> 'OrderedDict[str, tuple]':
    """state-dict key -> shape, in the torchvision ``Inception3`` naming of the published file"""
    out = OrderedDict()
    for name, (cin, cout, kh, kw, *_rest) in conv_specs().items():
        out[f'{name}.conv.weight'] = (cout, cin, kh, kw)
        for p in ('weight', 'bias', 'running_mean', 'running_var'):
            out[f'{name}.bn.{p}'] = (cout,)
    return out


def _ignored(key: str) -> bool:
    return key.startswith(('fc.', 'AuxLogits.')) or key.endswith('.num_batches_tracked')


def load_weights(weights) -> dict:
    """Validate a state dict (or the path of a ``torch.save``d one) and fold the BatchNorms: name -> (weight [cout][cin][kh][kw],
    bias [cout]) as fp32 CPU tensors, folded in float64.  ``fc.*``, ``AuxLogits.*`` and ``*.num_batches_tracked`` are ignored;
    a missing, mis-shaped or unknown key raises an error that names it."""
    sd = torch.load(weights, map_location='cpu', weights_only=True) if isinstance(weights, (str, os.PathLike)) else weights
    want = expected_keys()
    for key in sd:
        if key not in want and not _ignored(key):
            raise KeyError(f'fid: unexpected key {key!r} in the Inception weights')
    for key, shape in want.items():
        if key not in sd:
            raise KeyError(f'fid: the Inception weights lack {key!r}')
        if tuple(sd[key].shape) != shape:
            raise ValueError(f'fid: {key!r} has shape {tuple(sd[key].shape)}, expected {shape}')
    folded = {}
    for name in conv_specs():
        w = sd[f'{name}.conv.weight'].detach().to('cpu', torch.float64)
        gamma, beta, mean, var = (sd[f'{name}.bn.{p}'].detach().to('cpu', torch.float64)
                                  for p in ('weight', 'bias', 'running_mean', 'running_var'))
        scale = gamma / torch.sqrt(var + BN_EPS)
        folded[name] = ((w * scale[:, None, None, None]).float(), (beta - mean * scale).float())
    return folded


def _out(n: int, k: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - k) // stride + 1


class InceptionFeatures:
    """The table above on the HIP kernels.  Not an ``nn.Module``: nothing here is a parameter of the model that uses it.
    ``events``: when a list, every launch appends (kind, start, end) HIP events, kind in conv / pool / preprocess / stats
    (tools/fid_bench.py)."""

    def __init__(self, weights, device='cuda'):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('vqk: the FID network runs on the GPU only (HIP kernels, no CPU fallback)')
        self.specs = conv_specs()
        self.packed = {}
        for name, (w, b) in load_weights(weights).items():
            if w.shape[1] % 4:                                      # Conv2d_1a: 3 input channels -> the 4-channel input image
                w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 4 - w.shape[1] % 4))
            krsc = w.permute(0, 2, 3, 1).contiguous().to(self.device)
            self.packed[name] = (krsc, b.contiguous().to(self.device))
        self.events = None

    def _launch(self, kind, fn):
        if self.events is None:
            fn()
            return
        st = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        self.events.append((kind, e0, e1))

    def preprocess(self, images: torch.Tensor) -> torch.Tensor:
        """[B, 3, H, W] float view -> [B, 299, 299, 4] fp32 (pad channel zero), no copy of the input"""
        x = images.detach()
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or x.device.type != 'cuda':
            raise RuntimeError(f'vqk: FID images must be a CUDA float32 [B, 3, H, W] tensor, got {tuple(x.shape)} {x.dtype}')
        b, _, h, w = x.shape
        y = torch.empty(b, SIZE, SIZE, 4, device=x.device, dtype=torch.float32)
        sn, sc, sh, sw = x.stride()
        lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream
        self._launch('preprocess', lambda: _native.check(
            lib.vqk_fid_preprocess(x.data_ptr(), b, h, w, sn, sc, sh, sw, y.data_ptr(), st), 'fid_preprocess'))
        return y

    def conv(self, name: str, x: torch.Tensor, out: torch.Tensor | None = None, c_off: int = 0) -> torch.Tensor:
        cin, cout, kh, kw, stride, ph, pw = self.specs[name]
        w, bias = self.packed[name]
        b, h, wd, c = x.shape
        oh, ow = _out(h, kh, stride, ph), _out(wd, kw, stride, pw)
        if out is None:
            out = torch.empty(b, oh, ow, cout, device=x.device, dtype=torch.float32)
        lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream
        self._launch('conv', lambda: _native.check(
            lib.vqk_fid_conv(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), b, h, wd, c, cout, kh, kw, stride, ph,
                             pw, oh, ow, out.shape[3], c_off, st), f'fid_conv({name})'))
        return out

    def pool(self, x: torch.Tensor, mode: int, stride: int, pad: int, out: torch.Tensor | None = None, c_off: int = 0):
        b, h, w, c = x.shape
        oh, ow = _out(h, 3, stride, pad), _out(w, 3, stride, pad)
        if out is None:
            out = torch.empty(b, oh, ow, c, device=x.device, dtype=torch.float32)
        lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream
        self._launch('pool', lambda: _native.check(
            lib.vqk_fid_pool(x.data_ptr(), out.data_ptr(), b, h, w, c, mode, stride, pad, oh, ow, out.shape[3], c_off, st),
            'fid_pool'))
        return out

    def _empty(self, x, c):
        return torch.empty(x.shape[0], x.shape[1], x.shape[2], c, device=x.device, dtype=torch.float32)

    def _block_a(self, x, blk, pf):
        out = self._empty(x, 64 + 64 + 96 + pf)
        self.conv(f'{blk}.branch1x1', x, out, 0)
        self.conv(f'{blk}.branch5x5_2', self.conv(f'{blk}.branch5x5_1', x), out, 64)
        t = self.conv(f'{blk}.branch3x3dbl_2', self.conv(f'{blk}.branch3x3dbl_1', x))
        self.conv(f'{blk}.branch3x3dbl_3', t, out, 128)
        self.conv(f'{blk}.branch_pool', self.pool(x, _AVG, 1, 1), out, 224)
        return out

    def _block_b(self, x):
        b, h, w, c = x.shape
        out = torch.empty(b, _out(h, 3, 2, 0), _out(w, 3, 2, 0), 384 + 96 + c, device=x.device, dtype=torch.float32)
        self.conv('Mixed_6a.branch3x3', x, out, 0)
        t = self.conv('Mixed_6a.branch3x3dbl_2', self.conv('Mixed_6a.branch3x3dbl_1', x))
        self.conv('Mixed_6a.branch3x3dbl_3', t, out, 384)
        self.pool(x, _MAX, 2, 0, out, 480)
        return out

    def _block_c(self, x, blk):
        out = self._empty(x, 768)
        self.conv(f'{blk}.branch1x1', x, out, 0)
        t = self.conv(f'{blk}.branch7x7_2', self.conv(f'{blk}.branch7x7_1', x))
        self.conv(f'{blk}.branch7x7_3', t, out, 192)
        t = self.conv(f'{blk}.branch7x7dbl_1', x)
        for i in (2, 3, 4):
            t = self.conv(f'{blk}.branch7x7dbl_{i}', t)
        self.conv(f'{blk}.branch7x7dbl_5', t, out, 384)
        self.conv(f'{blk}.branch_pool', self.pool(x, _AVG, 1, 1), out, 576)
        return out

    def _block_d(self, x):
        b, h, w, c = x.shape
        out = torch.empty(b, _out(h, 3, 2, 0), _out(w, 3, 2, 0), 320 + 192 + c, device=x.device, dtype=torch.float32)
        self.conv('Mixed_7a.branch3x3_2', self.conv('Mixed_7a.branch3x3_1', x), out, 0)
        t = self.conv('Mixed_7a.branch7x7x3_1', x)
        for i in (2, 3):
            t = self.conv(f'Mixed_7a.branch7x7x3_{i}', t)
        self.conv('Mixed_7a.branch7x7x3_4', t, out, 320)
        self.pool(x, _MAX, 2, 0, out, 512)
        return out

    def _block_e(self, x, blk, pool_mode):
        out = self._empty(x, 2048)
        self.conv(f'{blk}.branch1x1', x, out, 0)
        t = self.conv(f'{blk}.branch3x3_1', x)
        self.conv(f'{blk}.branch3x3_2a', t, out, 320)
        self.conv(f'{blk}.branch3x3_2b', t, out, 704)
        t = self.conv(f'{blk}.branch3x3dbl_2', self.conv(f'{blk}.branch3x3dbl_1', x))
        self.conv(f'{blk}.branch3x3dbl_3a', t, out, 1088)
        self.conv(f'{blk}.branch3x3dbl_3b', t, out, 1472)
        self.conv(f'{blk}.branch_pool', self.pool(x, pool_mode, 1, 1), out, 1856)
        return out

    @torch.no_grad()
    def trunk(self, x: torch.Tensor) -> torch.Tensor:
        """the preprocessed [B, 299, 299, 4] input -> the last [B, 8, 8, 2048] map (any input size the table admits)"""
        for name in ('Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3'):
            x = self.conv(name, x)
        x = self.pool(x, _MAX, 2, 0)
        x = self.conv('Conv2d_4a_3x3', self.conv('Conv2d_3b_1x1', x))
        x = self.pool(x, _MAX, 2, 0)
        for blk, pf in POOL_FEATURES.items():
            x = self._block_a(x, blk, pf)
        x = self._block_b(x)
        for blk in C7:
            x = self._block_c(x, blk)
        x = self._block_d(x)
        x = self._block_e(x, 'Mixed_7b', _AVG)
        return self._block_e(x, 'Mixed_7c', _MAX)

    @torch.no_grad()
    def features(self, images: torch.Tensor) -> torch.Tensor:
        """[B, 3, H, W] float images in [0, 1] (any H x W, any strides) -> [B, 2048] fp32 features"""
        x = self.trunk(self.preprocess(images))
        b, h, w, c = x.shape
        f = torch.empty(b, c, device=x.device, dtype=torch.float32)
        lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream
        self._launch('pool', lambda: _native.check(lib.vqk_fid_mean(x.data_ptr(), f.data_ptr(), b, h * w, c, st), 'fid_mean'))
        return f


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1^1/2 S2 S1^1/2), float64 on the host"""
    mu1, mu2, s1, s2 = (torch.as_tensor(t).detach().to('cpu', torch.float64) for t in (mu1, mu2, sigma1, sigma2))
    e1, v1 = torch.linalg.eigh(s1)
    root1 = (v1 * e1.clamp(min=0).sqrt()) @ v1.T
    m = root1 @ s2 @ root1
    tr_covmean = torch.linalg.eigvalsh((m + m.T) / 2).clamp(min=0).sqrt().sum()
    diff = mu1 - mu2
    return float(diff.dot(diff) + torch.trace(s1) + torch.trace(s2) - 2.0 * tr_covmean)


class FrechetInceptionDistance:
    """torchmetrics ``FrechetInceptionDistance(feature=2048)`` on the HIP network: per side, the fp64 feature sum and Gram
    matrix live on the device (``vqk_fid_stats``, no host synchronisation in ``update``); ``compute`` reads them once."""

    def __init__(self, network, device='cuda'):
        self.net = network if isinstance(network, InceptionFeatures) else InceptionFeatures(network, device)
        self.device = self.net.device
        self.reset()

    def reset(self) -> None:
        d = FEATURES
        self.sums = {s: torch.zeros(d, dtype=torch.float64, device=self.device) for s in (True, False)}
        self.grams = {s: torch.zeros(d, d, dtype=torch.float64, device=self.device) for s in (True, False)}
        self.counts = {True: 0, False: 0}

    @torch.no_grad()
    def update(self, images: torch.Tensor, real: bool) -> None:
        f = self.net.features(images)
        self.update_features(f, real)

    def update_features(self, f: torch.Tensor, real: bool) -> None:
        """add [B, 2048] fp32 CUDA features to one side's statistics"""
        real = bool(real)
        if f.dim() != 2 or f.shape[1] != FEATURES or f.dtype != torch.float32 or not f.is_cuda:
            raise RuntimeError('vqk: FID features must be a CUDA float32 [B, 2048] tensor')
        f = f.contiguous()
        lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream
        self.net._launch('stats', lambda: _native.check(
            lib.vqk_fid_stats(f.data_ptr(), f.shape[0], FEATURES, self.sums[real].data_ptr(), self.grams[real].data_ptr(), st),
            'fid_stats'))
        self.counts[real] += f.shape[0]

    def statistics(self, real: bool):
        """(mu, Sigma) of one side as float64 CPU tensors"""
        n = self.counts[bool(real)]
        if n < 2:
            raise RuntimeError('vqk: FID needs at least two images on each side (real and fake)')
        s, g = self.sums[bool(real)].cpu(), self.grams[bool(real)].cpu()
        mu = s / n
        return mu, (g - n * torch.outer(mu, mu)) / (n - 1)

    def compute(self) -> float:
        mu1, s1 = self.statistics(True)
        mu2, s2 = self.statistics(False)
        return frechet_distance(mu1, s1, mu2, s2)
