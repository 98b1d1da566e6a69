"""Swin Transformer (Liu et al. 2021, "Hierarchical Vision Transformer using Shifted Windows") on NHWC
activations.

The input is a channels_last ``[B, 3, S, S]`` tensor; from the patch embedding on every activation is
a contiguous ``[B, H, W, C]`` tensor. A block is ``FusedLayerNorm``, attention inside ``window x window``
windows on xddp's HIP kernels (``ops/window_attention.py``: QKV projection, relative-position bias,
output projection), the residual, and a GELU MLP with its residual. Every second block shifts the map
by ``window // 2`` (a cyclic roll) and masks the attention so that tokens brought together by the wrap
do not see each other: the mask is kept as one int32 label per token (the region of the standard
nine-region partition it lies in), built once for the model's resolution and kept as a buffer. When a
stage's map is no larger than the window (7 x 7 at 224 input) there is no shift and no mask. Patch
embedding and patch merging are a reshape and one GEMM; the window partition, its reverse and the
roll stay in torch. Parameter names and counts are the usual ones (Swin-T: 28,288,354). Random init.
No stochastic depth.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops.layer_norm import FusedLayerNorm
from ..ops.window_attention import WindowAttention
from .convnext import _Patchify

__all__ = ["SwinTransformer", "shift_labels", "swin_t", "swin_tiny"]


def _windows(x, ws):
    """[B, H, W, C] -> [B * (H / ws) * (W / ws), ws * ws, C], windows row-major inside each image."""
    B, H, W, C = x.shape
    return x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def _unwindows(w, ws, B, H, W):
    return w.view(B, H // ws, W // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)


def shift_labels(H: int, W: int, window: int, shift: int) -> torch.Tensor:
    """int32 [windows, window^2]: for every token of the rolled map the region (0..8) of the standard
    nine-region partition it lies in. Two tokens of a window may attend to each other iff equal."""
    img = torch.zeros(1, H, W, 1, dtype=torch.int32)
    cuts = (slice(0, -window), slice(-window, -shift), slice(-shift, None))
    for i, hs in enumerate(cuts):
        for j, wsl in enumerate(cuts):
            img[:, hs, wsl] = 3 * i + j
    return _windows(img, window)[:, :, 0].contiguous()


class Block(nn.Module):
    def __init__(self, dim, heads, window, shift, mlp_ratio, resolution):
        super().__init__()
        self.window, self.shift = window, shift
        self.norm1 = FusedLayerNorm(dim, eps=1e-5)
        self.attn = WindowAttention(dim, heads, window)
        self.norm2 = FusedLayerNorm(dim, eps=1e-5)
        self.mlp = nn.Sequential(nn.Linear(dim, mlp_ratio * dim), nn.GELU(), nn.Linear(mlp_ratio * dim, dim))
        self.resolution = resolution
        self.register_buffer("labels", shift_labels(*resolution, window, shift) if shift else None, persistent=False)

    def forward(self, x):  # [B, H, W, C]
        B, H, W, _ = x.shape
        assert (H, W) == self.resolution, f"built for a {self.resolution} map, got {(H, W)}"
        y = self.norm1(x)
        if self.shift:
            y = torch.roll(y, (-self.shift, -self.shift), (1, 2))
        y = _unwindows(self.attn(_windows(y, self.window), self.labels), self.window, B, H, W)
        if self.shift:
            y = torch.roll(y, (self.shift, self.shift), (1, 2))
        x = x + y
        return x + self.mlp(self.norm2(x))


class PatchMerging(nn.Module):
    """2 x 2 neighbours concatenated (the usual order: (0,0), (1,0), (0,1), (1,1)), LayerNorm, 4C -> 2C."""

    def __init__(self, dim):
        super().__init__()
        self.norm = FusedLayerNorm(4 * dim, eps=1e-5)
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)

    def forward(self, x):
        B, H, W, C = x.shape
        x = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).reshape(B, H // 2, W // 2, 4 * C)
        return self.reduction(self.norm(x))


class SwinTransformer(nn.Module):
    def __init__(self, depths=(2, 2, 6, 2), embed_dim=96, heads=(3, 6, 12, 24), window=7, image_size=224, patch=4,
                 mlp_ratio=4, num_classes=1000):
        super().__init__()
        side = image_size // patch
        self.patch_embed = nn.Sequential(_Patchify(3, embed_dim, patch), FusedLayerNorm(embed_dim, eps=1e-5))
        stages = []
        for s, (depth, nh) in enumerate(zip(depths, heads)):
            dim, res = embed_dim << s, side >> s
            assert res % min(window, res) == 0, f"stage {s}: a {res} x {res} map does not split into {window}-windows"
            ws = min(window, res)  # a map no larger than the window is one window: no shift, no mask
            blocks = [Block(dim, nh, ws, ws // 2 if (i % 2 and res > window) else 0, mlp_ratio, (res, res))
                      for i in range(depth)]
            stages.append(nn.Sequential(*([PatchMerging(dim // 2)] if s else []), *blocks))
        self.stages = nn.Sequential(*stages)
        dim = embed_dim << (len(depths) - 1)
        self.norm = FusedLayerNorm(dim, eps=1e-5)
        self.head = nn.Linear(dim, num_classes)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.stages(self.patch_embed(x.permute(0, 2, 3, 1)))  # channels_last input: a contiguous NHWC view
        return self.head(self.norm(x).mean((1, 2)))


def swin_t(**kw):
    return SwinTransformer((2, 2, 6, 2), 96, (3, 6, 12, 24), **kw)


def swin_tiny(**kw):
    """Test-sized: 32 x 32 input, an 8 x 8 map of 4 x 4 windows (shifted in the second block), then one window."""
    return SwinTransformer((2, 2), 32, (1, 2), window=4, image_size=32, **kw)
