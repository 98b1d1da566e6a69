"""Mixup and CutMix on the device (``csrc/kernels/mixup.hip``), with the two-label target that
``ops.cross_entropy`` scores in one pass (:class:`~distributeddataparallel_amd.ops.MixedTarget`).

Every sample ``i`` is paired with ``j = B - 1 - i`` (the flip, timm's pairing). A plan holds, per
batch (``mode="batch"``) or per sample (``mode="elem"``), a weight ``lam`` and a box
``(y0, y1, x0, x1)``, half-open:

* Mixup (empty box): ``out[i] = lam * x[i] + (1 - lam) * x[j]``, ``lam ~ Beta(mixup_alpha, mixup_alpha)``;
* CutMix (a box): ``out[i]`` is ``x[j]`` inside the box and ``x[i]`` outside. The box is drawn as in
  timm's ``rand_bbox``: sides ``int(H * r)``, ``int(W * r)`` with ``r = sqrt(1 - lam)`` and
  ``lam ~ Beta(cutmix_alpha, cutmix_alpha)``, a uniform centre, clipped to the image; ``lam`` is then
  corrected to ``1 - area / (H * W)``, the share of the image that ``x[i]`` keeps.

The labels become ``MixedTarget(labels, labels[j], lam)``: ``lam`` weighs ``labels`` in the loss.
With both alphas positive each draw picks CutMix with probability ``switch_prob``; with probability
``1 - prob`` a draw is the identity (``lam = 1``, empty box).

:meth:`Mixup.draw` makes the plan on the host from a ``numpy.random.Generator`` seeded with
``seed`` and sends it to the object's persistent device tensors with one asynchronous copy from a
fresh pinned buffer (torch's caching host allocator keeps the buffer until the copy has run, so the
host never rewrites memory a copy still reads): no host sync. Under DDP pass ``seed = base + rank``,
or every rank mixes with the same plan. ``draw`` cannot be captured in a HIP graph;
:meth:`Mixup.apply` can: the kernel and the loss read ``lam`` and the box from the persistent
tensors, so a ``draw`` before each replay changes the mix. Because those tensors are rewritten by
the next ``draw``, run the backward of a step before drawing for the next one.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from ..ops.cross_entropy import MixedTarget

__all__ = ["Mixup", "MixPlan", "mix_images"]

_NATIVE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


class MixPlan(NamedTuple):
    """``lam`` fp32 [n] and ``box`` int32 [n, 4] on the device (n = 1 or B), and the host's values
    of both for logging (numpy, float32 / int32, same shapes)."""
    lam: torch.Tensor
    box: torch.Tensor
    host_lam: np.ndarray
    host_box: np.ndarray


def _mix_torch(x, partner, lam, box):
    """The rule of mixup.hip in torch (CPU tensors, other dtypes)."""
    B, _, H, W = x.shape
    xp = x.flip(0) if partner is None else x[partner.long()]
    lam = lam.to(device=x.device, dtype=torch.float32).reshape(-1, 1, 1, 1)
    box = box.to(x.device).reshape(-1, 4)
    y0, y1, x0, x1 = (box[:, k].reshape(-1, 1, 1, 1) for k in range(4))
    hh = torch.arange(H, device=x.device).reshape(1, 1, H, 1)
    ww = torch.arange(W, device=x.device).reshape(1, 1, 1, W)
    inside = (hh >= y0) & (hh < y1) & (ww >= x0) & (ww < x1)
    cut = (y1 > y0) & (x1 > x0)
    blend = (lam * x.float() + (1.0 - lam) * xp.float()).to(x.dtype)
    blend = torch.where(lam == 1, x, torch.where(lam == 0, xp, blend))  # a weight of 0 contributes nothing
    out = torch.empty_like(x)
    out.copy_(torch.where(cut, torch.where(inside, xp, x), blend))
    return out


def mix_images(x: torch.Tensor, partner: Optional[torch.Tensor], lam: torch.Tensor, box: torch.Tensor) -> torch.Tensor:
    """``out[i]`` = ``x[partner[i]]`` inside ``box`` and ``x[i]`` outside or, with an empty box,
    ``lam * x[i] + (1 - lam) * x[partner[i]]`` (module docstring); ``partner=None`` is the flip.
    fp32 / bf16 / fp16 CUDA images run the HIP kernel (a non-dense ``x`` is made contiguous first),
    anything else the same rule in torch."""
    if x.dim() != 4:
        raise ValueError(f"mix_images: x must be [B, C, H, W], got {tuple(x.shape)}")
    B = x.size(0)
    if lam.numel() not in (1, B) or box.numel() not in (4, 4 * B):
        raise ValueError(f"mix_images: lam must have 1 or B = {B} elements and box 1 or B rows of 4, got "
                         f"{lam.numel()} and {tuple(box.shape)}")
    if x.is_cuda and x.dtype in _NATIVE_DTYPES:
        from .._native import load

        if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
            x = x.contiguous()
        lam = lam.to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
        box = box.to(device=x.device, dtype=torch.int32).reshape(-1, 4).contiguous()
        if partner is not None:
            partner = partner.to(device=x.device, dtype=torch.int32).contiguous()
        return load().mix_images(x, partner, lam, box)
    return _mix_torch(x, partner, lam, box)


class Mixup:
    """Mixup / CutMix for image batches ``[B, C, H, W]`` with int64 labels ``[B]`` (module docstring).

    ``mixer(x, labels)`` draws a plan and applies it: ``(x_mixed, MixedTarget)``. In a captured
    step call :meth:`draw` outside the capture (before each replay) and :meth:`apply` inside."""

    def __init__(self, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0, prob: float = 1.0,
                 switch_prob: float = 0.5, mode: str = "batch", seed: int = 0):
        if mixup_alpha < 0 or cutmix_alpha < 0 or (mixup_alpha == 0 and cutmix_alpha == 0):
            raise ValueError("Mixup: mixup_alpha and cutmix_alpha must be >= 0 and not both 0")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError("Mixup: prob and switch_prob must be in [0, 1]")
        if mode not in ("batch", "elem"):
            raise ValueError(f"Mixup: mode must be 'batch' or 'elem', got {mode!r}")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode
        self.rng = np.random.default_rng(seed)
        self._buf = None  # int32 [5 n] on the device: lam's bits, then the boxes
        self.plan: Optional[MixPlan] = None

    def _draw_one(self, H: int, W: int):
        """(lam, box) of one draw, on the host."""
        if self.rng.random() >= self.prob:
            return 1.0, (0, 0, 0, 0)
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = self.rng.random() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0
        if not cut:
            return float(self.rng.beta(self.mixup_alpha, self.mixup_alpha)), (0, 0, 0, 0)
        lam = float(self.rng.beta(self.cutmix_alpha, self.cutmix_alpha))
        ratio = math.sqrt(max(0.0, 1.0 - lam))
        cut_h, cut_w = int(H * ratio), int(W * ratio)
        cy, cx = int(self.rng.integers(0, H)), int(self.rng.integers(0, W))
        y0, y1 = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
        x0, x1 = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
        if y1 <= y0 or x1 <= x0:  # nothing pasted: the identity
            return 1.0, (0, 0, 0, 0)
        return 1.0 - (y1 - y0) * (x1 - x0) / (H * W), (y0, y1, x0, x1)

    def draw(self, B: int, H: int, W: int, device) -> MixPlan:
        """Draw the plan for a batch of ``B`` images ``H x W`` and send it to ``device`` (no sync;
        not capturable). Returns the plan, which :meth:`apply` also finds in ``self.plan``."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:  # "cuda": name the device, or _buf never compares equal
            device = torch.device("cuda", torch.cuda.current_device())
        n = B if self.mode == "elem" else 1
        stage = torch.empty(5 * n, dtype=torch.int32, pin_memory=device.type == "cuda")
        lam = stage[:n].view(torch.float32).numpy()
        box = stage[n:].view(n, 4).numpy()
        for i in range(n):
            lam[i], box[i] = self._draw_one(H, W)
        if self._buf is None or self._buf.device != device or self._buf.numel() != 5 * n:
            self._buf = torch.empty(5 * n, dtype=torch.int32, device=device)
        self._buf.copy_(stage, non_blocking=True)
        self.plan = MixPlan(self._buf[:n].view(torch.float32), self._buf[n:].view(n, 4), lam.copy(), box.copy())
        return self.plan

    def apply(self, x: torch.Tensor, labels: torch.Tensor, plan: Optional[MixPlan] = None):
        """Mix ``x`` by ``plan`` (default: the last :meth:`draw`) -> ``(x_mixed, MixedTarget)``.
        Capturable: one kernel and a flip of the labels, both reading device memory."""
        plan = self.plan if plan is None else plan
        if plan is None:
            raise RuntimeError("Mixup.apply: no plan; call draw() first")
        out = mix_images(x, None, plan.lam, plan.box)
        return out, MixedTarget(labels, labels.flip(0), plan.lam)

    def __call__(self, x: torch.Tensor, labels: torch.Tensor):
        return self.apply(x, labels, self.draw(x.size(0), x.size(2), x.size(3), x.device))
