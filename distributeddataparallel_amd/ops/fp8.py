"""Opt-in FP8 training for the bias-free linear layers (``XDDP_FP8``; Llama projections).

Recipe: per-tensor *current* scaling — the scale of a tensor is ``FMAX / amax`` of this step's
values, with no history and no state carried across steps — e4m3 for activations and weights,
e5m2 for output gradients, fp32 accumulation, bf16 results. All three GEMMs of a linear run on
FP8 operands, each written as the one NT form ``gemm_fp8_nt`` (``csrc/kernels/gemm_fp8.hip``)
supports, so the cast kernel (``csrc/kernels/fp8_cast.hip``) also emits the transposed copy::

    Y [M,N] = X  [M,K] e4m3 · W  [N,K] e4m3 ᵀ
    dX[M,K] = dY [M,N] e5m2 · Wᵀ [K,N] e4m3 ᵀ
    dW[N,K] = dYᵀ[N,M] e5m2 · Xᵀ [K,M] e4m3 ᵀ

Saved for the backward: Xᵀ and Wᵀ as FP8 bytes and the two scales — not the bf16 X.

``XDDP_FP8=1`` runs the HIP kernels; ``XDDP_FP8=emulate`` runs the same autograd Functions with
every cast and GEMM in plain torch (same quantization formula, fp32 ``mm`` of the dequantized
bytes, result rounded to bf16): it works on CPU tensors too, shows FP8 numerics without a GPU
and is the oracle of the GPU tests. Scales and amax stay on the device; nothing syncs the host.
"""
from __future__ import annotations

import torch

from .._native import load
from .linear import _claim_grad_target

__all__ = ["E4M3", "E5M2", "FMAX", "quantize", "quantize_reference", "gemm_nt", "gemm_nt_reference"]

E4M3, E5M2 = 0, 1
FMAX = (448.0, 57344.0)
_DTYPES = (torch.float8_e4m3fn, torch.float8_e5m2)
_TINY = 1e-30  # keeps FMAX / amax finite for denormal-sized maxima


def quantize_reference(x2: torch.Tensor, fmt: int, transpose: bool = True):
    """Torch-only per-tensor quantization: ``(q, qT or None, scale)`` with ``q`` the FP8 bytes as
    uint8. The values are clamped to ±FMAX before the cast (torch's own cast of an out-of-range
    value to ``float8_e4m3fn`` gives NaN)."""
    amax = x2.abs().max().float().reshape(1)
    fmax = FMAX[fmt]
    # a tensor / tensor division: `float / tensor` is reciprocal-then-multiply in torch, one ulp off the
    # kernel's IEEE quotient, which flips every value that sits on a rounding tie
    scale = torch.where(amax > 0, torch.full_like(amax, fmax) / amax.clamp_min(_TINY), torch.ones_like(amax))
    q = (x2.float() * scale).clamp(-fmax, fmax).to(_DTYPES[fmt]).view(torch.uint8)
    return q, (q.t().contiguous() if transpose else None), scale


def quantize(x2: torch.Tensor, fmt: int, transpose: bool = True, emulate: bool = False):
    """``x2 [R, C]`` bf16 -> ``(q [R, C] uint8, qT [C, R] uint8 or None, scale float32[1])``."""
    if emulate:
        return quantize_reference(x2, fmt, transpose)
    C = load()
    return C.fp8_quantize(x2, C.fp8_amax(x2), fmt, transpose)


def gemm_nt_reference(a, b, sa, sb, a_fmt, b_fmt, res=None, out=None):
    """Torch-only ``gemm_fp8_nt``: fp32 ``mm`` of the dequantized bytes, rounded to bf16 (then
    ``+ res`` in fp32 and rounded again, as the kernel's epilogue does)."""
    y = (a.view(_DTYPES[a_fmt]).float() @ b.view(_DTYPES[b_fmt]).float().t()) / (sa * sb)
    y = y.to(torch.bfloat16)
    if res is not None:
        y = (res.float() + y.float()).to(torch.bfloat16)
    if out is not None:
        out.copy_(y)
        return out
    return y


def gemm_nt(a, b, sa, sb, a_fmt, b_fmt, res=None, out=None, emulate: bool = False):
    """bf16 ``(a · bᵀ) / (sa · sb)`` (+ ``res``, which may be ``out``) on FP8 bytes."""
    if emulate:
        return gemm_nt_reference(a, b, sa, sb, a_fmt, b_fmt, res, out)
    return load().gemm_fp8_nt(a, b, sa, sb, a_fmt, b_fmt, 0 if res is None else 1, res, out)


def _rows(t: torch.Tensor, cols: int) -> torch.Tensor:
    t2 = t.reshape(-1, cols)
    return t2 if t2.is_contiguous() and t2.data_ptr() % 16 == 0 else t2.clone(memory_format=torch.contiguous_format)


def _dw(dqT, sd, xqT, sx, param, emulate):
    """``dW = dYᵀ·X`` on FP8 operands — into the weight's registered gradient target when this is
    its first contribution (the claim rules of ``ops/linear.py``), returned as a fresh alias."""
    t = _claim_grad_target(param)
    if t is not None:
        gemm_nt(dqT, xqT, sd, sx, E5M2, E4M3, out=t, emulate=emulate)
        return t.view(t.shape)
    return gemm_nt(dqT, xqT, sd, sx, E5M2, E4M3, emulate=emulate)


class _Fp8Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emulate, x, weight, residual):
        N, K = weight.shape
        need_dx, need_dw = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        xq, xqT, sx = quantize(_rows(x, K), E4M3, need_dw, emulate)
        wq, wqT, sw = quantize(weight, E4M3, need_dx, emulate)
        res = None if residual is None else _rows(residual, N)
        y = gemm_nt(xq, wq, sx, sw, E4M3, E4M3, res=res, emulate=emulate)
        ctx.save_for_backward(xqT, wqT, sx, sw)
        ctx.emulate, ctx.param, ctx.shape, ctx.has_res = emulate, weight, x.shape, residual is not None
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xqT, wqT, sx, sw = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx = dw = None
        if need_dx or need_dw:
            dq, dqT, sd = quantize(_rows(dy, ctx.param.shape[0]), E5M2, need_dw, ctx.emulate)
            if need_dx:
                dx = gemm_nt(dq, wqT, sd, sw, E5M2, E4M3, emulate=ctx.emulate).view(ctx.shape)
            if need_dw:
                dw = _dw(dqT, sd, xqT, sx, ctx.param, ctx.emulate)
        dres = dy if ctx.has_res and ctx.needs_input_grad[3] else None
        return None, dx, dw, dres


class _Fp8MultiLinear(torch.autograd.Function):
    """``[x·W_iᵀ]`` over one input quantized once; the backward's ``dX = Σ dY_i·W_i`` accumulates in
    the GEMM epilogue (``res = out = dx`` from the second weight on)."""

    @staticmethod
    def forward(ctx, emulate, x, *weights):
        K = x.shape[-1]
        need_dx, need_dw = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
        xq, xqT, sx = quantize(_rows(x, K), E4M3, need_dw, emulate)
        ys, saved = [], []
        for w in weights:
            wq, wqT, sw = quantize(w, E4M3, need_dx, emulate)
            ys.append(gemm_nt(xq, wq, sx, sw, E4M3, E4M3, emulate=emulate).view(*x.shape[:-1], w.shape[0]))
            saved += [wqT, sw]
        ctx.save_for_backward(xqT, sx, *saved)
        ctx.emulate, ctx.params, ctx.shape = emulate, weights, x.shape
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        xqT, sx, *saved = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[1]
        dx, dws = None, []
        for i, (dy, w) in enumerate(zip(dys, ctx.params)):
            need_dw = dy is not None and ctx.needs_input_grad[2 + i]
            if dy is None or not (need_dx or need_dw):
                dws.append(None)
                continue
            wqT, sw = saved[2 * i], saved[2 * i + 1]
            dq, dqT, sd = quantize(_rows(dy, w.shape[0]), E5M2, need_dw, ctx.emulate)
            if need_dx:
                dx = gemm_nt(dq, wqT, sd, sw, E5M2, E4M3, res=dx, out=dx, emulate=ctx.emulate)
            dws.append(_dw(dqT, sd, xqT, sx, w, ctx.emulate) if need_dw else None)
        if dx is not None:
            dx = dx.view(ctx.shape)
        return (None, dx, *dws)


def eligible(mode: str, x: torch.Tensor, weight: torch.Tensor) -> bool:
    """Whether ``x·Wᵀ`` can take the FP8 path: bf16 operands (on the GPU for the kernels), both
    weight dimensions and the token count multiples of 128 (each is the N or K of one GEMM)."""
    if weight.dim() != 2 or x.dim() < 1 or x.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16:
        return False
    if x.device != weight.device or (mode == "1" and not x.is_cuda):
        return False
    N, K = weight.shape
    if x.shape[-1] != K or N % 128 or K % 128 or not weight.is_contiguous() or weight.data_ptr() % 16:
        return False
    tokens = x.numel() // K
    return tokens > 0 and tokens % 128 == 0


def fp8_linear(mode: str, x, weight, residual=None):
    return _Fp8Linear.apply(mode == "emulate", x, weight, residual)


def fp8_multi_linear(mode: str, x, *weights):
    return _Fp8MultiLinear.apply(mode == "emulate", x, *weights)
