"""n-layer PatchGAN discriminator (Isola et al. 2017, "Image-to-Image Translation with Conditional Adversarial Networks") on the vqk
kernels: the discriminator of the usual VQ-GAN recipes.  A stack of 4x4 convs (strides 2 ... 2, 1, 1; padding 1) with BatchNorm and
LeakyReLU(0.2) that ends in a map of patch logits.

State-dict keys and shapes are those of the familiar ``nn.Sequential`` named ``main``: ``main.0`` conv + bias, ``main.1`` LeakyReLU,
then ``n_layers`` groups of (conv without bias, BatchNorm2d, LeakyReLU) and a last conv + bias to one channel -- a torch module built
from ``nn.Conv2d(.., 4, s, 1)`` / ``nn.BatchNorm2d`` / ``nn.LeakyReLU(0.2)`` in that order exchanges state dicts with this one under
``strict=True``.  Here a conv launch carries its bias and LeakyReLU, and a BatchNorm launch sequence carries its LeakyReLU
(csrc/patchgan.hip), so the LeakyReLU entries of ``main`` are placeholders.

BatchNorm couples the samples of a pass: real and fake batches are never concatenated (``loss.py``), and statistics and buffers are
per process -- no SyncBN, as with plain DDP.  Not built: R1 / double backward, SyncBN, ActNorm, spectral norm."""
import math

import torch
from torch import nn

from ... import ops
from ..autoencoder import _to_internal


class PatchConv(nn.Module):
    """4x4 conv, padding 1; weight is the logical [O, I, 4, 4] stored channels_last (the kernels' [O][4][4][I] layout)"""

    def __init__(self, in_channels: int, out_channels: int, stride: int, bias: bool):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        w = torch.empty(out_channels, in_channels, 4, 4)
        nn.init.normal_(w, 0.0, 0.02)
        self.weight = nn.Parameter(w.contiguous(memory_format=torch.channels_last))
        if bias:                                               # as torch.nn.Conv2d draws it
            bound = 1 / math.sqrt(in_channels * 16)
            self.bias = nn.Parameter(torch.empty(out_channels).uniform_(-bound, bound))
        else:
            self.register_parameter('bias', None)

    def forward(self, x, lrelu: bool = False):
        return ops.conv4x4(x, self.weight, self.bias, stride=self.stride, lrelu=lrelu)


class PatchBatchNorm(nn.Module):
    """``torch.nn.BatchNorm2d`` (affine, track_running_stats, momentum 0.1, eps 1e-5) with the following LeakyReLU fused"""

    def __init__(self, num_features: int, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.weight = nn.Parameter(torch.empty(num_features).normal_(1.0, 0.02))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer('running_mean', torch.zeros(num_features))
        self.register_buffer('running_var', torch.ones(num_features))
        self.register_buffer('num_batches_tracked', torch.tensor(0, dtype=torch.long))

    def forward(self, x, lrelu: bool = True):
        return ops.batch_norm_lrelu(x, self.weight, self.bias, self.running_mean, self.running_var, self.num_batches_tracked,
                                    training=self.training, lrelu=lrelu, eps=self.eps, momentum=self.momentum)


class PatchLeakyReLU(nn.Module):
    """placeholder that keeps the index layout of the sequential: the activation runs in the launch of the layer in front of it"""
    negative_slope = 0.2

    def forward(self, x):
        raise RuntimeError('fused into the preceding layer: NLayerDiscriminator.forward walks `main` itself')


class NLayerDiscriminator(nn.Module):
    def __init__(self, input_nc: int = 3, ndf: int = 64, n_layers: int = 3):
        super().__init__()
        if input_nc < 1 or ndf < 1 or n_layers < 1:
            raise ValueError(f'NLayerDiscriminator: input_nc, ndf and n_layers must be positive, got {input_nc}, {ndf}, {n_layers}')
        self.compute_dtype = torch.float32
        self.conv_products = 'fp32'          # (4x4 convs have one product form per storage type: fp32 exact, bf16)
        self.input_nc, self.ndf, self.n_layers = input_nc, ndf, n_layers
        seq = [PatchConv(input_nc, ndf, 2, True), PatchLeakyReLU()]
        mult = 1
        for n in range(1, n_layers + 1):
            prev, mult = mult, min(2 ** n, 8)
            seq += [PatchConv(ndf * prev, ndf * mult, 2 if n < n_layers else 1, False), PatchBatchNorm(ndf * mult), PatchLeakyReLU()]
        seq.append(PatchConv(ndf * mult, 1, 1, True))
        self.main = nn.Sequential(*seq)

    @staticmethod
    def logit_size(size: int, n_layers: int = 3) -> int:
        """side of the logit map for an input side (0 or less: the image is too small)"""
        for _ in range(n_layers):
            size = ops.conv4x4_out(size, 2)
        return ops.conv4x4_out(ops.conv4x4_out(size, 1), 1) if size >= 1 else 0

    def forward(self, img, **_):
        """img [B, input_nc, H, W] (or already padded NHWC of the compute dtype) -> fp32 patch logits [B, 1, h', w']"""
        x = _to_internal(img, self.compute_dtype)
        layers = list(self.main)
        i = 0
        while i < len(layers):
            m = layers[i]
            act = i + 1 < len(layers) and isinstance(layers[i + 1], PatchLeakyReLU)
            x = m(x, lrelu=act)
            i += 2 if act else 1
        return x[:, :1].to(torch.float32)
