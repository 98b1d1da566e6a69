"""Attention inside small windows with a learned relative-position bias and a shifted-window mask
(Swin and its kin) on xddp's HIP kernels (csrc/kernels/window_attn.hip).

``qkv`` is the QKV projection's output viewed ``[Bw, N, 3, H, D]`` (windows, tokens per window,
q / k / v, heads, head width); the result is ``[Bw, N, H, D]``, ready for the output projection:

    softmax(scale * q k^T + bias[h], over the keys whose label equals the query's) v

``bias`` is ``[H, N, N]``. ``labels`` is an int32 ``[nW, N]`` tensor with ``Bw % nW == 0``: window
``w`` uses row ``w % nW``, and query ``i`` sees key ``j`` only where the two labels are equal. That is
Swin's shifted-window mask (its 0 / -100 table has exactly this structure) at 4 N bytes per window
instead of 4 N^2. Masked keys are truly excluded (weight 0), where the usual additive -100 leaves
them a weight below 4e-44: the two differ by less than any tolerance, but not bit for bit. Every
query must see at least one key (it always sees itself).

The HIP path covers bf16, ``D == 32``, ``1 <= N <= 64``, a dense 16-byte aligned ``qkv``, a contiguous
bf16 or fp32 ``bias`` and contiguous int32 ``labels``, all on one GPU. The backward recomputes the
softmax, so the autograd node saves ``qkv``, ``bias`` and ``labels`` only, and is bitwise repeatable
(the bias gradient is a fixed-order sum). Everything else (CPU tensors included), and every call
under ``XDDP_WINDOW_ATTN=0``, takes one eager torch implementation of the same mathematics.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .._native import load

__all__ = ["WindowAttention", "window_attention", "window_attention_supported"]


def window_attention_supported(qkv: torch.Tensor, bias: torch.Tensor | None = None,
                               labels: torch.Tensor | None = None) -> bool:
    """Whether ``window_attention(qkv, bias, labels)`` runs on the HIP kernels."""
    if os.environ.get("XDDP_WINDOW_ATTN", "1") == "0":
        return False
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 5 and qkv.size(2) == 3 and qkv.size(4) == 32
            and 1 <= qkv.size(1) <= 64 and qkv.size(3) < 65536 and qkv.is_contiguous() and qkv.data_ptr() % 16 == 0):
        return False
    Bw, N, _, H, _ = qkv.shape
    if bias is not None and not (bias.device == qkv.device and bias.dtype in (torch.bfloat16, torch.float32)
                                 and tuple(bias.shape) == (H, N, N) and bias.is_contiguous()):
        return False
    if labels is not None and not (labels.device == qkv.device and labels.dtype == torch.int32 and labels.dim() == 2
                                   and labels.size(1) == N and labels.size(0) >= 1 and Bw % labels.size(0) == 0
                                   and labels.is_contiguous()):
        return False
    return True


def _eager(qkv, bias, labels, scale):
    """The same mathematics in torch (fp32 for the 16-bit types), masked keys at -inf."""
    Bw, N, _, H, D = qkv.shape
    ct = torch.float32 if qkv.dtype in (torch.bfloat16, torch.float16) else qkv.dtype
    q, k, v = qkv.to(ct).permute(2, 0, 3, 1, 4)  # each [Bw, H, N, D]
    s = (q @ k.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.to(ct)
    if labels is not None:
        nW = labels.size(0)
        same = labels[:, :, None] == labels[:, None, :]  # [nW, N, N]; window w = b * nW + r uses row r
        s = s.view(Bw // nW, nW, H, N, N).masked_fill(~same[None, :, None], float("-inf")).view(Bw, H, N, N)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).to(qkv.dtype)


class _WindowAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bias, labels, scale):
        ctx.save_for_backward(qkv, bias, labels)
        ctx.scale = scale
        return load().window_attn_forward(qkv, None if bias is None else bias.detach(), labels, scale)

    @staticmethod
    def backward(ctx, d_out):
        qkv, bias, labels = ctx.saved_tensors
        need_qkv, need_bias = ctx.needs_input_grad[:2]
        if not (need_qkv or need_bias):
            return None, None, None, None
        if not d_out.is_contiguous():
            d_out = d_out.contiguous()
        elif d_out.data_ptr() % 16 != 0:
            d_out = d_out.clone()
        dqkv, dbias = load().window_attn_backward(qkv, bias, labels, d_out, ctx.scale, need_bias)
        return (dqkv if need_qkv else None), dbias, None, None


def window_attention(qkv: torch.Tensor, bias: torch.Tensor | None = None, labels: torch.Tensor | None = None,
                     scale: float | None = None) -> torch.Tensor:
    """``[Bw, N, 3, H, D]`` -> ``[Bw, N, H, D]`` (module docstring); ``scale`` defaults to ``D ** -0.5``."""
    if qkv.dim() != 5 or qkv.size(2) != 3:
        raise ValueError(f"qkv must be [Bw, N, 3, H, D], got {tuple(qkv.shape)}")
    scale = float(qkv.size(-1) ** -0.5 if scale is None else scale)
    if window_attention_supported(qkv, bias, labels):
        return _WindowAttention.apply(qkv, bias, labels, scale)
    return _eager(qkv, bias, labels, scale)


class WindowAttention(nn.Module):
    """Swin's W-MSA / SW-MSA on ``[Bw, window^2, dim]`` windows: QKV projection, attention with the
    relative-position bias (a learned ``[(2 window - 1)^2, heads]`` table gathered through a fixed
    index; the gather and, through autograd, its scatter-add stay in torch) and output projection."""

    def __init__(self, dim: int, heads: int, window: int):
        super().__init__()
        assert dim % heads == 0
        self.dim, self.heads, self.window = dim, heads, window
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        c = torch.stack(torch.meshgrid(torch.arange(window), torch.arange(window), indexing="ij")).flatten(1)  # [2, N]
        rel = c[:, :, None] - c[:, None, :] + (window - 1)  # [2, N, N], each in 0 .. 2 window - 2
        self.register_buffer("relative_position_index", rel[0] * (2 * window - 1) + rel[1], persistent=False)

    def bias(self) -> torch.Tensor:
        N = self.window ** 2
        t = self.relative_position_bias_table[self.relative_position_index.reshape(-1)]
        return t.view(N, N, self.heads).permute(2, 0, 1).contiguous()

    def forward(self, x: torch.Tensor, labels: torch.Tensor | None = None) -> torch.Tensor:
        Bw, N, C = x.shape
        qkv = self.qkv(x).view(Bw, N, 3, self.heads, C // self.heads)
        return self.proj(window_attention(qkv, self.bias(), labels).reshape(Bw, N, C))
