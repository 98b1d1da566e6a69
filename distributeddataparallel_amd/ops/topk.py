"""Top-k sparsified gradient wire with error feedback (``csrc/kernels/topk_comm.hip``).

A flat bucket of ``n`` elements is cut into blocks of ``block`` (1024 | 2048 | 4096) consecutive
elements, and every block keeps exactly ``k`` (8 | 16 | 32 | 64) entries. With the fp32 residual
``e`` an element's value is ``v = float(x) + e`` and its key the bit pattern of ``|v|``; the block
keeps the ``k`` real elements of largest key, ties going to the lower index, as slots in ascending
index order: a uint16 offset within the block and the fp32 ``v`` itself. The residual becomes 0 on
the selected elements and ``v`` on the others, so nothing is rounded. A block with fewer than ``k``
real elements ends in empty slots (offset ``0xFFFF``, value 0). A block with a NaN or an inf stores
offset ``0xFFFF`` and value NaN in all its slots, decodes to NaN everywhere and keeps its residual
as it was.

A payload is one uint8 buffer of ``segments`` segments; a segment covers ``cb`` blocks and holds
``cb * k`` fp32 values, then ``cb * k`` uint16 offsets: ``6 k / block`` bytes per element,
``payload_bytes`` in all. Blocks past the bucket's end (the padding to a multiple of ``segments``)
hold empty slots.

CUDA tensors (fp32 / bf16 / fp16) run the HIP kernels; CPU tensors run the same rules in torch. The
selection is a pure function of the block and no value is rounded, so the two agree bit for bit.
"""
from __future__ import annotations

from typing import Optional

import torch

__all__ = ["BLOCKS", "KS", "payload_bytes", "compress", "decode_mean", "reduce_reselect"]

BLOCKS = (1024, 2048, 4096)
KS = (8, 16, 32, 64)


def _check(block: int, k: int, segments: int):
    if block not in BLOCKS:
        raise ValueError(f"topk: block must be one of {BLOCKS}, got {block}")
    if k not in KS:
        raise ValueError(f"topk: k must be one of {KS}, got {k}")
    if segments < 1:
        raise ValueError(f"topk: segments must be >= 1, got {segments}")


def _flat(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"topk: {name} must be a flat contiguous tensor, got shape {tuple(t.shape)}")
    return t


def _err(err: torch.Tensor, numel: int, like: torch.Tensor) -> torch.Tensor:
    if err.dtype != torch.float32 or err.numel() != numel or err.device != like.device:
        raise ValueError(f"topk: err must be fp32 with {numel} elements on {like.device}")
    return _flat(err, "err")


def payload_bytes(numel: int, block: int = 2048, k: int = 32, segments: int = 1) -> int:
    """Bytes of a payload of ``segments`` segments for a bucket of ``numel`` elements."""
    _check(block, k, segments)
    nb = -(-numel // block)
    return segments * -(-nb // segments) * 6 * k


def _split(payload: torch.Tensor, k: int, segments: int):
    """(values [S, cb, k] fp32, offsets [S, cb, k] int32 in 0 .. 0xFFFF) of a payload."""
    seg = payload.view(segments, -1)
    cb = seg.size(1) // (6 * k)
    val = seg[:, :cb * k * 4].contiguous().view(torch.float32).view(segments, cb, k)
    off = seg[:, cb * k * 4:].contiguous().view(torch.int16).view(segments, cb, k).to(torch.int32) & 0xFFFF
    return val, off


def _select_rows(v: torch.Tensor, count: torch.Tensor, k: int):
    """Rows of fp32 ``v`` (zeros past the ``count`` real elements of a row) -> slot values [rows, k],
    slot offsets [rows, k] (int32), the new residual rows and the rows that were skipped."""
    rows, block = v.shape
    real = torch.arange(block) < count[:, None]
    key = torch.where(real, v.abs().view(torch.int32), -1)
    top = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :k]  # ties: the lower index
    off = torch.sort(top, dim=1).values
    val = v.gather(1, off)
    empty = off >= count[:, None]
    bad = (~torch.isfinite(v) & real).any(1)
    new = v.scatter(1, off, 0.0)  # padding stays 0 as well
    val = torch.where(bad[:, None], float("nan"), torch.where(empty, 0.0, val))
    off = torch.where(bad[:, None] | empty, 0xFFFF, off).to(torch.int32)
    return val, off, new, bad


def _store(payload, segments, val, off):
    seg = payload.view(segments, -1)
    values = seg.size(1) // 6 * 4  # bytes of a segment's values; its offsets follow
    seg[:, :values] = val.contiguous().view(torch.uint8).view(segments, -1)
    seg[:, values:] = off.to(torch.int16).view(torch.uint8).view(segments, -1)


def _decode_mean(payload, block, k, segments):
    """fp32 [cb * block]: the decoded segments added up in order, divided by their number."""
    val, off = _split(payload, k, segments)
    cb = val.size(1)
    skipped = (off[..., 0] == 0xFFFF) & torch.isnan(val[..., 0])  # [S, cb]
    dense = torch.zeros(segments, cb, block + 1)  # column `block` takes the empty slots
    dense.scatter_(2, off.clamp_max(block).long(), val)
    d = torch.where(skipped[..., None], float("nan"), dense[..., :block])
    acc = d[0]
    for r in range(1, segments):
        acc = acc + d[r]
    if segments > 1:
        acc = acc / float(segments)
    return acc.reshape(-1)


def compress(x: torch.Tensor, err: torch.Tensor, block: int = 2048, k: int = 32, segments: int = 1,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Compress flat ``x + err`` into a payload of ``segments`` segments (``out`` or a new buffer)
    and leave what the payload does not carry in ``err`` (fp32, as long as ``x``)."""
    _check(block, k, segments)
    x = _flat(x, "x")
    err = _err(err, x.numel(), x)
    nbytes = payload_bytes(x.numel(), block, k, segments)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if x.is_cuda:
        from .._native import load

        load().topk_compress(x, err, out, block, k, segments)
        return out
    if out.dtype != torch.uint8 or out.numel() != nbytes:
        raise ValueError(f"topk.compress: out must be uint8 with {nbytes} elements")
    if nbytes == 0:
        return out
    total, n = nbytes // (6 * k), x.numel()
    v = torch.zeros(total * block, dtype=torch.float32)
    v[:n] = x.float() + err
    count = (n - torch.arange(total) * block).clamp(0, block)
    val, off, new, bad = _select_rows(v.view(total, block), count, k)
    _store(out, segments, val, off)
    keep = bad[:, None].expand(-1, block).reshape(-1)[:n]
    err.copy_(torch.where(keep, err, new.view(-1)[:n]))
    return out


def decode_mean(payload: torch.Tensor, out: torch.Tensor, block: int = 2048, k: int = 32, segments: int = 1,
                mode: str = "mean") -> torch.Tensor:
    """Decode ``payload`` into flat ``out``. ``mode="mean"``: the segments are ``segments`` ranks'
    payloads of the same bucket and ``out`` is their mean, added up in fp32 in segment order (an
    element a rank did not select counts as +0) and divided once; ``mode="concat"``: the segments
    cover consecutive block ranges."""
    _check(block, k, segments)
    if mode not in ("mean", "concat"):
        raise ValueError(f"topk.decode_mean: mode must be 'mean' or 'concat', got {mode!r}")
    out = _flat(out, "out")
    if out.is_cuda:
        from .._native import load

        load().topk_decode_mean(payload, out, block, k, segments, mode)
        return out
    if mode == "mean":
        want = segments * payload_bytes(out.numel(), block, k, 1)
    else:
        want = payload_bytes(out.numel(), block, k, segments)
    if payload.dtype != torch.uint8 or payload.numel() != want:
        raise ValueError(f"topk.decode_mean: payload must be uint8 with {want} elements")
    if want == 0:
        return out
    if mode == "mean":
        dec = _decode_mean(payload, block, k, segments)
    else:
        dec = torch.cat([_decode_mean(s, block, k, 1) for s in payload.view(segments, -1)])
    out.copy_(dec[:out.numel()])
    return out


def reduce_reselect(payload_in: torch.Tensor, err: torch.Tensor, block: int = 2048, k: int = 32, segments: int = 1,
                    numel: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One segment holding ``compress(mean of payload_in's segments + err)`` for the chunk a rank
    owns in the two-shot all-reduce; ``err`` (fp32, ``cb * block`` long) is this rank's residual of
    the chunk and is updated in place, ``numel`` (default: all) says how many elements of the chunk
    are real. The mean never exists in memory."""
    _check(block, k, segments)
    bpb = 6 * k
    if payload_in.numel() % (segments * bpb):
        raise ValueError(f"topk.reduce_reselect: payload_in must hold {segments} segments of whole blocks")
    cb = payload_in.numel() // (segments * bpb)
    err = _err(err, cb * block, payload_in)
    numel = cb * block if numel is None else numel
    if not 0 <= numel <= cb * block:
        raise ValueError(f"topk.reduce_reselect: numel must be in [0, {cb * block}], got {numel}")
    if out is None:
        out = torch.empty(cb * bpb, dtype=torch.uint8, device=payload_in.device)
    if payload_in.is_cuda:
        from .._native import load

        load().topk_reduce_reselect(payload_in, err, out, block, k, segments, numel)
        return out
    if out.dtype != torch.uint8 or out.numel() != cb * bpb:
        raise ValueError("topk.reduce_reselect: out must be uint8, one segment long")
    if cb == 0:
        return out
    real = torch.arange(cb * block) < numel
    v = torch.where(real, _decode_mean(payload_in, block, k, segments) + err, torch.zeros(()))
    val, off, new, bad = _select_rows(v.view(cb, block), real.view(cb, block).sum(1), k)
    _store(out, 1, val, off)
    keep = bad[:, None].expand(-1, block).reshape(-1) | ~real
    err.copy_(torch.where(keep, err, new.view(-1)))
    return out
