"""Depthwise convolution (``groups == C``) on xddp's NHWC HIP kernels (csrc/kernels/dwconv.hip): the
spatial mixing layer of ConvNeXt and of the MobileNet / EfficientNet family.

The HIP path covers dense channels_last ``x`` [B, C, H, W] with a 16-byte aligned base in bf16, fp16
or fp32, ``C % 8 == 0``, a ``[C, 1, k, k]`` weight with ``k`` in {3, 5, 7} of ``x``'s dtype (and an
optional bias of that dtype), stride 1, padding ``k // 2``, dilation 1. Everything else (CPU tensors
included), and every call under ``XDDP_DWCONV=0``, takes ``F.conv2d`` with identical arguments.

Forward and input gradient are one kernel (the gradient runs it on ``dy`` with the taps flipped);
the weight and bias gradient is a two-stage fixed-order reduction, bitwise repeatable. The weight
is repacked tap-major ``[k * k, C]`` once per forward (at most 37 k elements) and the copy is kept
for the backward.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .._native import load

__all__ = ["DepthwiseConv2d", "depthwise_conv2d", "dwconv_supported"]


def dwconv_supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """Whether ``depthwise_conv2d(x, weight)`` runs on the HIP kernels."""
    if os.environ.get("XDDP_DWCONV", "1") == "0":
        return False
    if not (x.is_cuda and x.dim() == 4 and weight.dim() == 4 and x.dtype in (torch.bfloat16, torch.float16, torch.float32)):
        return False
    C, k = x.size(1), weight.size(2)
    return (C % 8 == 0 and tuple(weight.shape) == (C, 1, k, k) and k in (3, 5, 7) and weight.dtype == x.dtype
            and weight.device == x.device and x.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0)


class _DWConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        C, k = weight.size(0), weight.size(2)
        w_taps = weight.detach().reshape(C, k * k).t().contiguous()
        ctx.save_for_backward(x, w_taps)
        ctx.k = k
        return load().dwconv_forward(x, w_taps, None if bias is None else bias.detach(), False)

    @staticmethod
    def backward(ctx, dy):
        x, w_taps = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad
        dx = dw = db = None
        if not dy.is_contiguous(memory_format=torch.channels_last):
            dy = dy.contiguous(memory_format=torch.channels_last)
        elif dy.data_ptr() % 16 != 0:
            dy = dy.clone()
        if need_x:
            dx = load().dwconv_forward(dy, w_taps, None, True)
        if need_w or need_b:
            dw, db = load().dwconv_wgrad(dy, x, ctx.k, need_b)
        return dx, (dw if need_w else None), db


def depthwise_conv2d(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """``F.conv2d(x, weight, bias, padding=k // 2, groups=C)`` for a ``[C, 1, k, k]`` weight."""
    if dwconv_supported(x, weight) and (bias is None or (bias.dtype == x.dtype and bias.device == x.device)):
        return _DWConv.apply(x, weight, bias)
    return F.conv2d(x, weight, bias, stride=1, padding=weight.size(2) // 2, groups=weight.size(0))


class DepthwiseConv2d(nn.Conv2d):
    """``nn.Conv2d(channels, channels, kernel_size, padding=kernel_size // 2, groups=channels)`` (the
    same parameters and state dict) whose forward is :func:`depthwise_conv2d`."""

    def __init__(self, channels: int, kernel_size: int, bias: bool = True, device=None, dtype=None):
        super().__init__(channels, channels, kernel_size, padding=kernel_size // 2, groups=channels, bias=bias,
                         device=device, dtype=dtype)

    def forward(self, x):
        return depthwise_conv2d(x, self.weight, self.bias)
