"""Flash attention on gfx950 MFMA kernels (``csrc/kernels/flash_attn.hip``) for the ViT-L/16 and
Llama-3-8B configs of BASELINE.json.

Inputs and output are ``[B, S, H, D]`` (the projection's own layout: q/k/v are views of the
projection outputs and the output reshapes to ``[B, S, H·D]`` for the output projection without a
copy). Grouped-query attention: ``k``/``v`` may have fewer heads than ``q``. bf16, D in {64, 128}.

``XDDP_FLASH_ATTN=0`` sends every call to ``F.scaled_dot_product_attention`` (A/B and parity).
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

from .._native import load

__all__ = ["flash_attention", "flash_supported"]


def flash_supported(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    if os.environ.get("XDDP_FLASH_ATTN", "1") == "0":
        return False
    D = q.shape[-1]
    ok = (q.is_cuda and q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16
          and q.dim() == 4 and D in (64, 128) and k.shape[-1] == D and v.shape == k.shape
          and q.shape[2] % k.shape[2] == 0)
    if not ok:
        return False
    for t in (q, k, v):
        if t.stride(-1) != 1 or any(s % 8 for s in t.stride()[:3]) or t.data_ptr() % 16:
            return False
    return True


class _FlashAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal: bool, scale: float, doc_start=None, doc_end=None):
        if doc_start is None:
            o, lse = load().flash_attn_forward(q, k, v, causal, scale)
        else:
            o, lse = load().flash_attn_forward(q, k, v, causal, scale, doc_start)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal, ctx.scale = causal, scale
        ctx.docs = None if doc_start is None else (doc_start, doc_end)  # int32, not differentiable
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        if do.stride(-1) != 1 or any(s % 8 for s in do.stride()[:3]):
            do = do.contiguous()
        if ctx.docs is None:
            dq, dk, dv = load().flash_attn_backward(do, q, k, v, o, lse, ctx.causal, ctx.scale)
        else:
            dq, dk, dv = load().flash_attn_backward(do, q, k, v, o, lse, ctx.causal, ctx.scale,
                                                    doc_start=ctx.docs[0], doc_end=ctx.docs[1])
        return dq, dk, dv, None, None, None, None


def _bounds(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.int32).contiguous()


def doc_mask(doc_start: torch.Tensor, causal: bool) -> torch.Tensor:
    """Boolean ``[B, 1, S, S]`` attention mask (true = visible) of a packed batch: same document,
    and under ``causal`` also key <= query."""
    S = doc_start.shape[1]
    k = torch.arange(S, device=doc_start.device)
    if causal:  # doc_start[q] <= k <= q
        m = (k[None, None, :] >= doc_start[:, :, None]) & (k[None, None, :] <= k[None, :, None])
    else:
        m = doc_start[:, :, None] == doc_start[:, None, :]
    return m[:, None]


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False,
                    scale: float | None = None, docs=None) -> torch.Tensor:
    """softmax(q kᵀ · scale [+ causal mask]) v over [B, S, H, D] tensors; returns [B, S, H, D].

    ``docs`` (packed sequences; any object with int32 ``[B, S]`` ``.doc_start`` / ``.doc_end``, see
    ``data/packing.py``) restricts every query to the keys of its own document. Causal calls the
    kernels cover run their document-masked variants, which also skip the K/V tiles before a query
    block's first document; every other call takes SDPA with the equivalent boolean mask."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    if docs is None:
        if flash_supported(q, k, v):
            return _FlashAttn.apply(q, k, v, causal, scale)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=causal,
                                           scale=scale, enable_gqa=k.shape[2] != q.shape[2])
        return o.transpose(1, 2)
    if q.shape[1] != k.shape[1] or tuple(docs.doc_start.shape) != (q.shape[0], q.shape[1]):
        raise ValueError("flash_attention: docs needs Sq == Sk and [B, S] bounds")
    if causal and flash_supported(q, k, v):
        return _FlashAttn.apply(q, k, v, True, scale, _bounds(docs.doc_start, q.device),
                                _bounds(docs.doc_end, q.device))
    mask = doc_mask(docs.doc_start.to(q.device), causal)
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    if k.shape[2] != q.shape[2]:
        try:
            return F.scaled_dot_product_attention(qt, kt, vt, attn_mask=mask, scale=scale,
                                                  enable_gqa=True).transpose(1, 2)
        except RuntimeError:  # a backend that refuses a mask together with enable_gqa
            rep = q.shape[2] // k.shape[2]
            kt, vt = kt.repeat_interleave(rep, dim=1), vt.repeat_interleave(rep, dim=1)
    return F.scaled_dot_product_attention(qt, kt, vt, attn_mask=mask, scale=scale).transpose(1, 2)
