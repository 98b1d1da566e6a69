"""ConvNeXt (Liu et al. 2022, "A ConvNet for the 2020s") on NHWC activations end to end.

The input is a channels_last ``[B, 3, H, W]`` tensor; from the stem on every activation is a
contiguous ``[B, H, W, C]`` tensor (``permute(0, 2, 3, 1)`` of a channels_last tensor is a view), so
LayerNorm and the linear layers work on the last dimension with no layout copy. A block is the 7x7
depthwise convolution on xddp's HIP kernels (``ops/dwconv.py``), ``FusedLayerNorm``, two linear
layers around a GELU, a per-channel scale and the residual. The patchify convolutions (4x4/s4
stem, 2x2/s2 downsamples) are a reshape into patches and one GEMM; their weights keep the
``nn.Conv2d`` shape, so parameter names and counts are the usual ones (ConvNeXt-T: 28,589,128).
Random init. No stochastic depth and no EMA.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.dwconv import DepthwiseConv2d
from ..ops.layer_norm import FusedLayerNorm
from ..ops.pool import global_avg_pool

__all__ = ["ConvNeXt", "convnext_tiny"]


class _Patchify(nn.Conv2d):
    """A p x p / stride p convolution of an NHWC tensor [B, H, W, C] -> [B, H / p, W / p, O] as one GEMM."""

    def __init__(self, cin, cout, p):
        super().__init__(cin, cout, kernel_size=p, stride=p)

    def forward(self, x):
        B, H, W, C = x.shape
        p = self.kernel_size[0]
        x = x[:, :H - H % p, :W - W % p]  # a strided convolution drops the remainder
        patches = x.reshape(B, H // p, p, W // p, p, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // p, W // p, p * p * C)
        return F.linear(patches, self.weight.permute(0, 2, 3, 1).reshape(self.out_channels, -1), self.bias)


class Block(nn.Module):
    def __init__(self, dim, layer_scale):
        super().__init__()
        self.dwconv = DepthwiseConv2d(dim, 7)
        self.norm = FusedLayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale * torch.ones(dim))

    def forward(self, x):  # [B, H, W, C]
        y = self.dwconv(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        y = self.pwconv2(self.act(self.pwconv1(self.norm(y))))
        return x + self.gamma * y


class ConvNeXt(nn.Module):
    def __init__(self, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), num_classes=1000, layer_scale=1e-6):
        super().__init__()
        self.downsample_layers = nn.ModuleList([nn.Sequential(_Patchify(3, dims[0], 4), FusedLayerNorm(dims[0], eps=1e-6))])
        for a, b in zip(dims[:-1], dims[1:]):
            self.downsample_layers.append(nn.Sequential(FusedLayerNorm(a, eps=1e-6), _Patchify(a, b, 2)))
        self.stages = nn.ModuleList([nn.Sequential(*[Block(d, layer_scale) for _ in range(n)])
                                     for n, d in zip(depths, dims)])
        self.norm = FusedLayerNorm(dims[-1], eps=1e-6)
        self.head = nn.Linear(dims[-1], num_classes)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = x.permute(0, 2, 3, 1)  # channels_last [B, 3, H, W]: a contiguous [B, H, W, 3] view
        for down, stage in zip(self.downsample_layers, self.stages):
            x = stage(down(x))
        return self.head(self.norm(global_avg_pool(x.permute(0, 3, 1, 2))))


def convnext_tiny(**kw):
    return ConvNeXt((3, 3, 9, 3), (96, 192, 384, 768), **kw)
