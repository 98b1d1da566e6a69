"""Softmax cross-entropy on xddp's HIP kernels: fp32 math on fp32 / bf16 / fp16 logits
[rows, classes] without an fp32 copy of the logits, its zero-filled fp32 gradient and the casts
(one read of the logits forward, one read + one write in the logits' dtype backward).

Two sets of kernels serve it. ``csrc/kernels/cross_entropy.hip`` is the Llama-3-8B LM head of
BASELINE.json config 5: bf16 logits, a class count divisible by 8, mean over the non-ignored rows;
a call with default arguments on such logits runs it exactly as before. Every other native call
runs ``csrc/kernels/cross_entropy_rows.hip``: any class count >= 1 and any row alignment (one wave
per row up to 1024 classes, the classification heads; one block per row above), label smoothing,
z-loss and the reductions none / sum / mean, reduced on the device. CPU tensors, other ranks and
other dtypes fall back to a torch composition with the same semantics.

With ``lse`` the row's log-sum-exp, ``keep = target != ignore_index``, ``eps = label_smoothing`` and
``z = z_loss``::

    row loss      keep * ((1 - eps) * (lse - x[t]) + eps * (lse - mean(x)) + z * lse**2)
    row gradient  g_r * keep * (softmax * (1 + 2 * z * lse) - (1 - eps) * onehot(t) - eps / classes)

At ``z = 0`` this is torch's ``label_smoothing``. ``"mean"`` divides by the number of kept rows,
at least 1: a finite 0 (not torch's NaN) when every row is ignored. A ``-inf`` (masked) logit gets a
gradient of exactly 0 and leaves the loss finite at ``eps = 0``; at ``eps > 0`` that row's loss is
``+inf``, as in torch (the smoothing term averages ``-log p`` over every class).

A :class:`MixedTarget` ``(a, b, lam)`` in place of the int64 target scores each row against two
classes (Mixup / CutMix, ``data/mixup.py``) in one pass of ``csrc/kernels/cross_entropy_mixed.hip``
instead of ``lam * CE(x, a) + (1 - lam) * CE(x, b)``. With ``w_a = lam``, ``w_b = 1 - lam`` and
``keep = (a != ignore_index) and (b != ignore_index)``::

    row loss      keep * ((1 - eps) * (lse - w_a x[a] - w_b x[b]) + eps * (lse - mean(x)) + z * lse**2)
    row gradient  g_r * keep * (softmax * (1 + 2 z lse) - (1 - eps) * (w_a onehot(a) + w_b onehot(b)) - eps / classes)

A weight of exactly 0 contributes nothing, also on a ``-inf`` logit: ``lam == 1`` gives the bits of
the hard-target call on ``a``, ``lam == 0`` those of the call on ``b``. ``lam`` is not checked to lie
in ``[0, 1]``. Dense probability targets (a ``[rows, classes]`` float target), class weights and
int32 targets are not supported.

Targets outside ``[0, classes)`` other than ``ignore_index`` are an error, as in torch. The
kernel makes that row's loss NaN (so the step's loss shows it at once), gives it no gradient and
sets a per-device flag; the flag is copied to pinned host memory behind the kernel and read at
the next call (or by :func:`check_targets`), which raises ``IndexError`` — no host sync per step.
``XDDP_XENT_CHECK=sync`` checks right after the forward instead (a sync per call).

Under HIP-graph capture (``bench.py --graphs``, ``utils/graphs.py``) the host-side check, the flag
copy and the event are skipped: an event query or record inside a capture is not allowed, and a
replay could not run the host check anyway. The device flag is still set and the row's loss is
still NaN, so a bad target shows in the replayed loss; the next eager call raises as usual.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import torch
import torch.nn.functional as F

from .._native import load

__all__ = ["cross_entropy", "CrossEntropyLoss", "MixedTarget", "check_targets"]

_FLAGS: dict = {}  # device index -> (device flag int32[1], pinned host copy, event of the copy)
_REDUCTIONS = {"none": 0, "sum": 1, "mean": 2}
_NATIVE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


class MixedTarget(NamedTuple):
    """The target of a Mixup / CutMix batch (``data.Mixup``): int64 classes ``a`` and ``b`` [rows]
    weighted ``lam`` and ``1 - lam``; ``lam`` is an fp32 tensor with 1 or ``rows`` elements (a
    Python number is accepted and copied to the device). It is read on the device, so a captured
    step sees the value written before each replay, and it gets no gradient."""
    a: torch.Tensor
    b: torch.Tensor
    lam: torch.Tensor


def _flag(dev: torch.device):
    f = _FLAGS.get(dev.index)
    if f is None:
        f = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32).pin_memory(),
             torch.cuda.Event())
        _FLAGS[dev.index] = f
    return f


def check_targets(block: bool = False) -> None:
    """Raise ``IndexError`` if a fused cross-entropy call so far saw a target outside
    ``[0, classes)`` (other than ``ignore_index``). Without ``block`` only copies that already
    landed are looked at (no sync)."""
    for dev, (flag, host, ev) in _FLAGS.items():
        if block:
            ev.synchronize()
        elif not ev.query():
            continue
        if int(host[0]) != 0:
            flag.zero_()
            host.zero_()
            raise IndexError(f"cross_entropy: a target is out of bounds (not in [0, classes) and not "
                             f"ignore_index) on cuda:{dev}")


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        C = load()
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            check_targets()  # an earlier call's invalid target surfaces here, without a sync
        flag, host, ev = _flag(logits.device)
        loss_rows, lse = C.cross_entropy_forward(logits, target, ignore_index, flag)
        if not capturing:
            host.copy_(flag, non_blocking=True)
            ev.record(torch.cuda.current_stream(logits.device))
            if os.environ.get("XDDP_XENT_CHECK") == "sync":
                check_targets(block=True)
        count = (target != ignore_index).sum().clamp_min(1).to(torch.float32)
        ctx.save_for_backward(logits, target, lse, count)
        ctx.ignore_index = ignore_index
        return loss_rows.sum() / count

    @staticmethod
    def backward(ctx, g):
        logits, target, lse, count = ctx.saved_tensors
        gscale = (g.to(torch.float32) / count).reshape(1).contiguous()
        d = load().cross_entropy_backward(logits, target, lse, gscale, ctx.ignore_index)
        return d, None, None


class _CrossEntropyRows(torch.autograd.Function):
    """cross_entropy_rows.hip: the row kernel and, for sum / mean, the finalize kernel forward (no
    torch reduction in between), one kernel backward; the kept-row count stays on the device."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, label_smoothing, z_loss, reduction):
        C = load()
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            check_targets()
        flag, host, ev = _flag(logits.device)
        out = C.cross_entropy_rows_forward(logits, target, ignore_index, label_smoothing, z_loss,
                                           _REDUCTIONS[reduction], flag)
        if not capturing:
            host.copy_(flag, non_blocking=True)
            ev.record(torch.cuda.current_stream(logits.device))
            if os.environ.get("XDDP_XENT_CHECK") == "sync":
                check_targets(block=True)
        if reduction == "mean":
            ctx.save_for_backward(logits, target, out[1], out[3])
        else:
            ctx.save_for_backward(logits, target, out[1])
        ctx.args = (ignore_index, label_smoothing, z_loss)
        return out[0] if reduction == "none" else out[2]

    @staticmethod
    def backward(ctx, g):
        logits, target, lse, *count = ctx.saved_tensors
        g = g.to(torch.float32).contiguous().reshape(-1)
        d = load().cross_entropy_rows_backward(logits, target, lse, g, count[0] if count else None, *ctx.args)
        return d, None, None, None, None, None


def _fallback(logits, target, ignore_index, label_smoothing, z_loss, reduction):
    """The same semantics in plain torch, on the fp32 upcast."""
    x = logits.float()
    if label_smoothing == 0.0 and z_loss == 0.0 and reduction == "mean":
        return F.cross_entropy(x, target, ignore_index=ignore_index)
    rows = F.cross_entropy(x, target, ignore_index=ignore_index, label_smoothing=label_smoothing, reduction="none")
    keep = target != ignore_index
    if z_loss != 0.0:
        rows = rows + z_loss * torch.logsumexp(x, 1 if x.dim() > 1 else 0) ** 2 * keep
    if reduction == "none":
        return rows
    return rows.sum() if reduction == "sum" else rows.sum() / keep.sum().clamp_min(1)


class _CrossEntropyMixed(torch.autograd.Function):
    """cross_entropy_mixed.hip: :class:`_CrossEntropyRows` against a :class:`MixedTarget`; ``lam``
    is saved for the backward and gets no gradient."""

    @staticmethod
    def forward(ctx, logits, a, b, lam, ignore_index, label_smoothing, z_loss, reduction):
        C = load()
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            check_targets()
        flag, host, ev = _flag(logits.device)
        out = C.cross_entropy_mixed_forward(logits, a, b, lam, ignore_index, label_smoothing, z_loss,
                                            _REDUCTIONS[reduction], flag)
        if not capturing:
            host.copy_(flag, non_blocking=True)
            ev.record(torch.cuda.current_stream(logits.device))
            if os.environ.get("XDDP_XENT_CHECK") == "sync":
                check_targets(block=True)
        if reduction == "mean":
            ctx.save_for_backward(logits, a, b, lam, out[1], out[3])
        else:
            ctx.save_for_backward(logits, a, b, lam, out[1])
        ctx.args = (ignore_index, label_smoothing, z_loss)
        return out[0] if reduction == "none" else out[2]

    @staticmethod
    def backward(ctx, g):
        logits, a, b, lam, lse, *count = ctx.saved_tensors
        g = g.to(torch.float32).contiguous().reshape(-1)
        d = load().cross_entropy_mixed_backward(logits, a, b, lam, lse, g, count[0] if count else None, *ctx.args)
        return d, None, None, None, None, None, None, None


def _fallback_mixed(logits, target, ignore_index, label_smoothing, z_loss, reduction):
    """The two-label semantics in plain torch, on the fp32 upcast: the two hard-target row losses
    weighted lam and 1 - lam, a weight of exactly 0 leaving its term out (no 0 * inf)."""
    x = logits.float()
    a, b = target.a, target.b
    wa = torch.as_tensor(target.lam, dtype=torch.float32, device=x.device).reshape(-1)
    wb = 1.0 - wa
    la = F.cross_entropy(x, a, ignore_index=ignore_index, label_smoothing=label_smoothing, reduction="none")
    lb = F.cross_entropy(x, b, ignore_index=ignore_index, label_smoothing=label_smoothing, reduction="none")
    rows = torch.where(wb == 0, la, torch.where(wa == 0, lb, wa * la + wb * lb))
    keep = (a != ignore_index) & (b != ignore_index)
    rows = torch.where(keep, rows, torch.zeros_like(rows))
    if z_loss != 0.0:
        rows = rows + z_loss * torch.logsumexp(x, 1) ** 2 * keep
    if reduction == "none":
        return rows
    return rows.sum() if reduction == "sum" else rows.sum() / keep.sum().clamp_min(1)


def _cross_entropy_mixed(logits, target, ignore_index, label_smoothing, z_loss, reduction):
    a, b, lam = target
    if logits.dim() != 2 or a.dim() != 1 or b.dim() != 1 or a.size(0) != logits.size(0) or b.size(0) != logits.size(0):
        raise ValueError(f"cross_entropy: a MixedTarget needs logits [rows, classes] and a, b [rows], got "
                         f"{tuple(logits.shape)}, {tuple(a.shape)}, {tuple(b.shape)}")
    n = lam.numel() if torch.is_tensor(lam) else 1
    if n != 1 and n != logits.size(0):
        raise ValueError(f"cross_entropy: MixedTarget.lam must have 1 or rows = {logits.size(0)} elements, got {n}")
    if (logits.is_cuda and logits.dtype in _NATIVE_DTYPES and logits.size(1) >= 1 and a.dtype == torch.long
            and b.dtype == torch.long and a.device == logits.device and b.device == logits.device):
        lam = torch.as_tensor(lam, dtype=torch.float32, device=logits.device).reshape(-1).contiguous()
        logits = logits.contiguous()
        if logits.data_ptr() % 16:
            logits = logits.clone()
        return _CrossEntropyMixed.apply(logits, a.contiguous(), b.contiguous(), lam, ignore_index,
                                        float(label_smoothing), float(z_loss), reduction)
    return _fallback_mixed(logits, target, ignore_index, label_smoothing, z_loss, reduction)


def cross_entropy(logits: torch.Tensor, target, ignore_index: int = -100, *,
                  label_smoothing: float = 0.0, z_loss: float = 0.0, reduction: str = "mean") -> torch.Tensor:
    """Softmax cross-entropy of ``logits`` [rows, classes] against ``target`` [rows] with label
    smoothing, z-loss (``z_loss * lse**2`` per row) and ``reduction`` in none / sum / mean (module
    docstring). ``target`` is an int64 class per row or a :class:`MixedTarget` (two classes per row
    and their weight, Mixup / CutMix); dense probability targets and class weights are not
    supported. 2-D fp32 / bf16 / fp16 CUDA logits with int64 targets run the HIP kernels, anything
    else the torch composition on the fp32 upcast."""
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"cross_entropy: label_smoothing must be in [0, 1), got {label_smoothing}")
    if not z_loss >= 0.0:
        raise ValueError(f"cross_entropy: z_loss must be >= 0, got {z_loss}")
    if reduction not in _REDUCTIONS:
        raise ValueError(f"cross_entropy: reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
    if isinstance(target, MixedTarget):
        return _cross_entropy_mixed(logits, target, ignore_index, label_smoothing, z_loss, reduction)
    default = label_smoothing == 0.0 and z_loss == 0.0 and reduction == "mean"
    if (default and logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2
            and logits.size(1) % 8 == 0 and target.dtype == torch.long and target.dim() == 1):
        return _CrossEntropy.apply(logits.contiguous(), target.contiguous(), ignore_index)
    if (logits.is_cuda and logits.dtype in _NATIVE_DTYPES and logits.dim() == 2 and logits.size(1) >= 1
            and target.dtype == torch.long and target.dim() == 1 and target.size(0) == logits.size(0)
            and target.device == logits.device):
        logits = logits.contiguous()
        if logits.data_ptr() % 16:  # a view into the middle of a buffer: the kernels want a 16-B aligned base
            logits = logits.clone()
        return _CrossEntropyRows.apply(logits, target.contiguous(), ignore_index, float(label_smoothing),
                                       float(z_loss), reduction)
    return _fallback(logits, target, ignore_index, label_smoothing, z_loss, reduction)


class CrossEntropyLoss(torch.nn.Module):
    """:func:`cross_entropy` as a module (``nn.CrossEntropyLoss`` without class weights and dense
    probability targets, plus ``z_loss``); ``target`` may be a :class:`MixedTarget`."""

    def __init__(self, ignore_index: int = -100, label_smoothing: float = 0.0, z_loss: float = 0.0,
                 reduction: str = "mean"):
        super().__init__()
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"CrossEntropyLoss: label_smoothing must be in [0, 1), got {label_smoothing}")
        if not z_loss >= 0.0:
            raise ValueError(f"CrossEntropyLoss: z_loss must be >= 0, got {z_loss}")
        if reduction not in _REDUCTIONS:
            raise ValueError(f"CrossEntropyLoss: reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
        self.ignore_index = ignore_index
        self.label_smoothing = label_smoothing
        self.z_loss = z_loss
        self.reduction = reduction

    def extra_repr(self) -> str:
        return (f"ignore_index={self.ignore_index}, label_smoothing={self.label_smoothing}, "
                f"z_loss={self.z_loss}, reduction={self.reduction!r}")

    def forward(self, logits: torch.Tensor, target) -> torch.Tensor:
        return cross_entropy(logits, target, self.ignore_index, label_smoothing=self.label_smoothing,
                             z_loss=self.z_loss, reduction=self.reduction)
