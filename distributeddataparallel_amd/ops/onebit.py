"""1-bit gradient wire with error feedback (``csrc/kernels/onebit_comm.hip``).

A flat bucket of ``n`` elements is cut into blocks of ``block`` (512 | 1024 | 2048) consecutive
elements. With the fp32 residual ``e`` a block of ``c`` real elements stores, for ``v = float(x) + e``,
``scale = sum |v| / c`` (fp32) and one bit per element, ``v < 0``; it decodes to ``d = -scale`` or
``+scale``, and the residual becomes ``v - d``. Element ``i`` of a block is bit ``i % 8`` of byte
``i // 8``. A block with a NaN or an inf (or whose ``|v|`` sum overflows fp32) stores
``scale = NaN`` and zero bits, decodes to NaN everywhere and keeps its residual as it was.

A payload is one uint8 buffer of ``segments`` segments; a segment covers ``cb`` blocks and holds
``cb * block / 8`` sign bytes, then ``cb`` fp32 scales: ``payload_bytes`` in all. Blocks past the
bucket's end (the padding to a multiple of ``segments``) hold zeros.

CUDA tensors (fp32 / bf16 / fp16) run the HIP kernels; CPU tensors run the same rules in torch with
the same fp32 operations in the same order, so sign bits and residuals agree bit for bit with the
kernels given the same scale; only the order of the ``|v|`` sum, and so the scale's last bits, may
differ.
"""
from __future__ import annotations

from typing import Optional

import torch

__all__ = ["BLOCKS", "payload_bytes", "compress", "decode_mean", "reduce_recompress"]

BLOCKS = (512, 1024, 2048)


def _check(block: int, segments: int):
    if block not in BLOCKS:
        raise ValueError(f"onebit: block must be one of {BLOCKS}, got {block}")
    if segments < 1:
        raise ValueError(f"onebit: segments must be >= 1, got {segments}")


def _flat(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"onebit: {name} must be a flat contiguous tensor, got shape {tuple(t.shape)}")
    return t


def _err(err: torch.Tensor, numel: int, like: torch.Tensor) -> torch.Tensor:
    if err.dtype != torch.float32 or err.numel() != numel or err.device != like.device:
        raise ValueError(f"onebit: err must be fp32 with {numel} elements on {like.device}")
    return _flat(err, "err")


def payload_bytes(numel: int, block: int = 1024, segments: int = 1) -> int:
    """Bytes of a payload of ``segments`` segments for a bucket of ``numel`` elements."""
    _check(block, segments)
    nb = -(-numel // block)
    return segments * -(-nb // segments) * (block // 8 + 4)


def _split(payload: torch.Tensor, block: int, segments: int):
    """(sign bytes [S, cb * block / 8], scale bytes [S, cb * 4]) uint8 views of a payload."""
    seg = payload.view(segments, -1)
    cb = seg.size(1) // (block // 8 + 4)
    return seg[:, :cb * (block // 8)], seg[:, cb * (block // 8):]


_WEIGHTS = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32)


def _compress_rows(v: torch.Tensor, count: torch.Tensor):
    """Rows of fp32 ``v`` (zeros past the real elements, ``count`` of them per row) -> sign bytes
    [rows, block / 8], scale [rows], the new residual rows and the rows that were skipped."""
    total = v.abs().sum(1)
    bad = ~torch.isfinite(total)
    scale = torch.where(bad, torch.full_like(total, float("nan")), total / count.clamp_min(1).float())
    neg = (v < 0) & ~bad[:, None]
    packed = (neg.view(v.size(0), -1, 8).to(torch.int32) * _WEIGHTS).sum(2).to(torch.uint8)
    d = torch.where(neg, -scale[:, None], scale[:, None])
    return packed, scale, v - d, bad


def _store(payload, block, segments, packed, scale):
    pb, ps = _split(payload, block, segments)
    pb.copy_(packed.view(segments, -1))
    ps.copy_(scale.contiguous().view(torch.uint8).view(segments, -1))


def _decode_mean(payload, block, segments):
    """fp32 [cb * block]: the decoded segments added up in order, divided by their number."""
    pb, ps = _split(payload, block, segments)
    scale = ps.contiguous().view(torch.float32)  # [S, cb]
    neg = ((pb.to(torch.int32)[..., None] >> torch.arange(8, dtype=torch.int32)) & 1).bool()
    neg = neg.view(segments, scale.size(1), block)
    d = torch.where(neg, -scale[..., None], scale[..., None])
    acc = d[0]
    for r in range(1, segments):
        acc = acc + d[r]
    if segments > 1:
        acc = acc / float(segments)
    return acc.reshape(-1)


def compress(x: torch.Tensor, err: torch.Tensor, block: int = 1024, segments: int = 1,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Compress flat ``x + err`` into a payload of ``segments`` segments (``out`` or a new buffer)
    and leave what the payload does not carry in ``err`` (fp32, as long as ``x``)."""
    _check(block, segments)
    x = _flat(x, "x")
    err = _err(err, x.numel(), x)
    nbytes = payload_bytes(x.numel(), block, segments)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if x.is_cuda:
        from .._native import load

        load().onebit_compress(x, err, out, block, segments)
        return out
    if out.dtype != torch.uint8 or out.numel() != nbytes:
        raise ValueError(f"onebit.compress: out must be uint8 with {nbytes} elements")
    if nbytes == 0:
        return out
    total, n = nbytes // (block // 8 + 4), x.numel()
    v = torch.zeros(total * block, dtype=torch.float32)
    v[:n] = x.float() + err
    count = (n - torch.arange(total) * block).clamp(0, block)
    packed, scale, new, bad = _compress_rows(v.view(total, block), count)
    _store(out, block, segments, packed, scale)
    keep = bad[:, None].expand(-1, block).reshape(-1)[:n]
    err.copy_(torch.where(keep, err, new.view(-1)[:n]))
    return out


def decode_mean(payload: torch.Tensor, out: torch.Tensor, block: int = 1024, segments: int = 1,
                mode: str = "mean") -> torch.Tensor:
    """Decode ``payload`` into flat ``out``. ``mode="mean"``: the segments are ``segments`` ranks'
    payloads of the same bucket and ``out`` is their mean, added up in fp32 in segment order and
    divided once; ``mode="concat"``: the segments cover consecutive block ranges."""
    _check(block, segments)
    if mode not in ("mean", "concat"):
        raise ValueError(f"onebit.decode_mean: mode must be 'mean' or 'concat', got {mode!r}")
    out = _flat(out, "out")
    if out.is_cuda:
        from .._native import load

        load().onebit_decode_mean(payload, out, block, segments, mode)
        return out
    if mode == "mean":
        want = segments * payload_bytes(out.numel(), block, 1)
    else:
        want = payload_bytes(out.numel(), block, segments)
    if payload.dtype != torch.uint8 or payload.numel() != want:
        raise ValueError(f"onebit.decode_mean: payload must be uint8 with {want} elements")
    if want == 0:
        return out
    if mode == "mean":
        dec = _decode_mean(payload, block, segments)
    else:
        dec = torch.cat([_decode_mean(s, block, 1) for s in payload.view(segments, -1)])
    out.copy_(dec[:out.numel()])
    return out


def reduce_recompress(payload_in: torch.Tensor, err: torch.Tensor, block: int = 1024, segments: int = 1,
                      numel: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One segment holding ``compress(mean of payload_in's segments + err)`` for the chunk a rank
    owns in the two-shot all-reduce; ``err`` (fp32, ``cb * block`` long) is this rank's residual of
    the chunk and is updated in place, ``numel`` (default: all) says how many elements of the chunk
    are real. The mean never exists in memory."""
    _check(block, segments)
    bpb = block // 8 + 4
    if payload_in.numel() % (segments * bpb):
        raise ValueError(f"onebit.reduce_recompress: payload_in must hold {segments} segments of whole blocks")
    cb = payload_in.numel() // (segments * bpb)
    err = _err(err, cb * block, payload_in)
    numel = cb * block if numel is None else numel
    if not 0 <= numel <= cb * block:
        raise ValueError(f"onebit.reduce_recompress: numel must be in [0, {cb * block}], got {numel}")
    if out is None:
        out = torch.empty(cb * bpb, dtype=torch.uint8, device=payload_in.device)
    if payload_in.is_cuda:
        from .._native import load

        load().onebit_reduce_recompress(payload_in, err, out, block, segments, numel)
        return out
    if out.dtype != torch.uint8 or out.numel() != cb * bpb:
        raise ValueError("onebit.reduce_recompress: out must be uint8, one segment long")
    if cb == 0:
        return out
    real = torch.arange(cb * block) < numel
    v = torch.where(real, _decode_mean(payload_in, block, segments) + err, torch.zeros(()))
    packed, scale, new, bad = _compress_rows(v.view(cb, block), real.view(cb, block).sum(1))
    _store(out, block, 1, packed, scale)
    keep = bad[:, None].expand(-1, block).reshape(-1) | ~real
    err.copy_(torch.where(keep, err, new.view(-1)))
    return out
