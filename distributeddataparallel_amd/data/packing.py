"""Packed-sequence bookkeeping: several short documents back to back in one fixed-length row.

A packed row is described per token, not by ``cu_seqlens``: ``doc_start[b, s]`` is the index of the
first token of the document token ``s`` belongs to, ``doc_end[b, s]`` one past its last token, and
``positions[b, s] = s - doc_start[b, s]`` the token's position inside its document (what rotary
embeddings index). Key ``k`` is visible to query ``q`` iff ``doc_start[b, q] <= k <= q`` — so each
kernel lane needs one scalar and no search (``ops/attention.py``, ``csrc/kernels/flash_attn.hip``).

Everything here is vectorised torch (cummax / cummin, no loop over tokens), runs on CPU or GPU and
never synchronises with the device.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

__all__ = ["PackedDocs", "packed_docs", "packed_docs_from_ids", "packed_labels"]


class PackedDocs(NamedTuple):
    """Per-token document bounds of a packed batch, each int32 ``[B, S]``."""
    doc_start: torch.Tensor
    doc_end: torch.Tensor
    positions: torch.Tensor

    def to(self, device) -> "PackedDocs":
        return PackedDocs(*(t.to(device) for t in self))


def _from_first(first: torch.Tensor) -> PackedDocs:
    """``first[b, s]``: token ``s`` opens a document (``first[:, 0]`` is taken as true)."""
    B, S = first.shape
    idx = torch.arange(S, device=first.device).expand(B, S)
    first = first.clone()
    first[:, 0] = True
    # the latest opening at or before s / the earliest opening after s (S when there is none)
    start = torch.where(first, idx, torch.zeros_like(idx)).cummax(dim=1).values
    nxt = torch.where(first, idx, torch.full_like(idx, S))
    nxt = torch.cat([nxt[:, 1:], torch.full_like(idx[:, :1], S)], dim=1)
    end = nxt.flip(1).cummin(dim=1).values.flip(1)
    return PackedDocs(start.to(torch.int32).contiguous(), end.to(torch.int32).contiguous(),
                      (idx - start).to(torch.int32).contiguous())


def packed_docs(tokens: torch.Tensor, eos_id: int) -> PackedDocs:
    """Bounds of ``tokens: [B, S]`` where an EOS token closes the document it belongs to and the
    token after it opens the next one; a row's last document runs to ``S``."""
    first = torch.zeros_like(tokens, dtype=torch.bool)
    first[:, 1:] = tokens[:, :-1] == eos_id
    return _from_first(first)


def packed_docs_from_ids(doc_ids: torch.Tensor) -> PackedDocs:
    """Bounds from per-token document ids ``[B, S]``: a document starts wherever the id changes."""
    first = torch.zeros_like(doc_ids, dtype=torch.bool)
    first[:, 1:] = doc_ids[:, 1:] != doc_ids[:, :-1]
    return _from_first(first)


def packed_labels(tokens: torch.Tensor, docs: PackedDocs, ignore_index: int = -100) -> torch.Tensor:
    """Next-token targets ``[B, S]`` of a packed batch: the last token of every document (its "next
    token" opens another document) and of the row gets ``ignore_index``."""
    B, S = tokens.shape
    nxt = torch.cat([tokens[:, 1:], tokens[:, :1]], dim=1)
    idx = torch.arange(S, device=tokens.device).expand(B, S)
    last = idx + 1 >= docs.doc_end.to(tokens.device)
    return torch.where(last, torch.full_like(nxt, ignore_index), nxt)
