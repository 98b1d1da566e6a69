"""8-bit block-quantized gradient wire (``csrc/kernels/q8_comm.hip``).

A flat bucket of ``n`` elements is cut into blocks of ``block`` (128 | 256 | 512 | 1024) consecutive
elements. A block of finite values stores ``lo = min``, ``scale = (max - lo) / 255`` and one byte per
element, ``code = clamp(rint((x - lo) / scale), 0, 255)`` (0 for a constant block), and decodes as
``fmaf(code, scale, lo)``: within ``scale / 2`` of ``x``, whatever the block's sign or offset. A block
with a NaN or an inf (or whose ``max - min`` overflows fp32) stores ``scale = NaN`` and decodes to
NaN everywhere, so an overflow check after the reduction still fires.

A payload is one uint8 buffer of ``segments`` segments; a segment covers ``cb`` blocks and holds
``cb * block`` code bytes, then ``cb`` fp32 pairs ``(lo, scale)``: ``payload_bytes`` in all. Blocks
past the bucket's end (the padding to a multiple of ``segments``) hold zeros.

CUDA tensors (fp32 / bf16 / fp16) run the HIP kernels; CPU tensors run the same rules in torch, so
a hook built on these ops works on the CPU backend too (there ``fmaf`` is evaluated in fp64 and
rounded, which can differ from the kernel in the last bit).
"""
from __future__ import annotations

from typing import Optional

import torch

__all__ = ["BLOCKS", "payload_bytes", "quantize", "dequantize_mean", "reduce_requantize"]

BLOCKS = (128, 256, 512, 1024)


def _check(block: int, segments: int):
    if block not in BLOCKS:
        raise ValueError(f"q8: block must be one of {BLOCKS}, got {block}")
    if segments < 1:
        raise ValueError(f"q8: segments must be >= 1, got {segments}")


def _flat(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"q8: {name} must be a flat contiguous tensor, got shape {tuple(t.shape)}")
    return t


def payload_bytes(numel: int, block: int = 512, segments: int = 1) -> int:
    """Bytes of a payload of ``segments`` segments for a bucket of ``numel`` elements."""
    _check(block, segments)
    nb = -(-numel // block)
    return segments * -(-nb // segments) * (block + 8)


def _split(payload: torch.Tensor, block: int, segments: int):
    """(codes [S, cb, block] uint8 view, params bytes [S, cb * 8] uint8 view) of a payload."""
    seg = payload.view(segments, -1)
    cb = seg.size(1) // (block + 8)
    return seg[:, :cb * block].view(segments, cb, block), seg[:, cb * block:]


def _params(pbytes: torch.Tensor):
    p = pbytes.contiguous().view(torch.float32).view(pbytes.size(0), -1, 2)
    return p[..., 0:1], p[..., 1:2]  # lo, scale: [S, cb, 1]


def _quantize_rows(v: torch.Tensor, real: torch.Tensor):
    """Rows of fp32 values (``real`` marks the bucket's own elements) -> codes uint8, lo, scale."""
    inf = torch.tensor(float("inf"), dtype=torch.float32)
    lo = torch.where(real, v, inf).amin(1, keepdim=True)
    hi = torch.where(real, v, -inf).amax(1, keepdim=True)
    empty = ~real.any(1, keepdim=True)
    lo = torch.where(empty, torch.zeros_like(lo), lo)
    hi = torch.where(empty, torch.zeros_like(hi), hi)
    bad = ~(torch.isfinite(torch.where(real, v, torch.zeros_like(v))).all(1, keepdim=True)
            & torch.isfinite(hi - lo))
    scale = torch.where(bad, torch.full_like(lo, float("nan")), (hi - lo) / 255.0)
    ok = real & (scale > 0)
    q = torch.where(ok, ((v - lo) / scale).round().clamp(0, 255), torch.zeros_like(v))
    return torch.nan_to_num(q).to(torch.uint8), lo, scale


def _store(payload, block, segments, codes, lo, scale):
    pc, pp = _split(payload, block, segments)
    pc.copy_(codes.view(pc.shape))
    pp.copy_(torch.cat([lo, scale], 1).contiguous().view(torch.uint8).view(pp.shape))


def _decode_mean(payload, block, segments):
    """fp32 [cb * block]: the decoded segments accumulated in order, divided by their number."""
    codes, pbytes = _split(payload, block, segments)
    lo, scale = _params(pbytes)
    acc = torch.zeros(codes.shape[1:], dtype=torch.float32)
    for r in range(segments):
        acc += (codes[r].double() * scale[r].double() + lo[r].double()).float()
    if segments > 1:
        acc = acc / float(segments)
    return acc.view(-1)


def quantize(x: torch.Tensor, block: int = 512, segments: int = 1,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Quantize flat ``x`` into a payload of ``segments`` segments (``out`` or a new buffer)."""
    _check(block, segments)
    x = _flat(x, "x")
    nbytes = payload_bytes(x.numel(), block, segments)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if x.is_cuda:
        from .._native import load

        load().q8_quantize(x, out, block, segments)
        return out
    if out.dtype != torch.uint8 or out.numel() != nbytes:
        raise ValueError(f"q8.quantize: out must be uint8 with {nbytes} elements")
    if nbytes == 0:
        return out
    total, n = nbytes // (block + 8), x.numel()
    v = torch.zeros(total * block, dtype=torch.float32)
    v[:n] = x.float()
    real = (torch.arange(total * block) < n).view(total, block)
    _store(out, block, segments, *_quantize_rows(v.view(total, block), real))
    return out


def dequantize_mean(payload: torch.Tensor, out: torch.Tensor, block: int = 512, segments: int = 1,
                    mode: str = "mean") -> torch.Tensor:
    """Decode ``payload`` into flat ``out``. ``mode="mean"``: the segments are ``segments`` ranks'
    payloads of the same bucket and ``out`` is their mean, accumulated in fp32 in segment order
    and divided once; ``mode="concat"``: the segments cover consecutive block ranges."""
    _check(block, segments)
    if mode not in ("mean", "concat"):
        raise ValueError(f"q8.dequantize_mean: mode must be 'mean' or 'concat', got {mode!r}")
    out = _flat(out, "out")
    if out.is_cuda:
        from .._native import load

        load().q8_dequantize_mean(payload, out, block, segments, mode)
        return out
    if mode == "mean":
        want = segments * payload_bytes(out.numel(), block, 1)
    else:
        want = payload_bytes(out.numel(), block, segments)
    if payload.dtype != torch.uint8 or payload.numel() != want:
        raise ValueError(f"q8.dequantize_mean: payload must be uint8 with {want} elements")
    if want == 0:
        return out
    if mode == "mean":
        dec = _decode_mean(payload, block, segments)
    else:
        dec = torch.cat([_decode_mean(s, block, 1) for s in payload.view(segments, -1)])
    out.copy_(dec[:out.numel()])
    return out


def reduce_requantize(payload_in: torch.Tensor, block: int = 512, segments: int = 1,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One segment holding the quantized mean of ``payload_in``'s ``segments`` segments (the chunk a
    rank owns in the two-shot all-reduce); the mean never exists in fp32 in memory."""
    _check(block, segments)
    if payload_in.numel() % (segments * (block + 8)):
        raise ValueError(f"q8.reduce_requantize: payload_in must hold {segments} segments of whole blocks")
    if out is None:
        out = torch.empty(payload_in.numel() // segments, dtype=torch.uint8, device=payload_in.device)
    if payload_in.is_cuda:
        from .._native import load

        load().q8_reduce_requant(payload_in, out, block, segments)
        return out
    if out.dtype != torch.uint8 or out.numel() * segments != payload_in.numel():
        raise ValueError("q8.reduce_requantize: out must be uint8, one segment long")
    if out.numel() == 0:
        return out
    v = _decode_mean(payload_in, block, segments).view(-1, block)
    _store(out, block, 1, *_quantize_rows(v, torch.ones_like(v, dtype=torch.bool)))
    return out
