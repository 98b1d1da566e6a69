"""``FusedAdafactor``: ``torch.optim.Adafactor`` semantics on the tiled 2-D HIP kernels of
``csrc/kernels/adafactor.hip``, plus fp32 master weights and ``grad_scale``.

Adafactor keeps one row vector and one column vector of second moments per weight matrix instead of
a full-size moment: for an ``[R, C]`` matrix ``4 (R + C)`` bytes of state where Adam keeps ``8 R C``.
A step is a fixed number of stream-ordered launches per (dtype group x 40 tensors) and nothing
synchronises with the host. The update of any element needs sums over its whole tensor, so, as for
the layer-wise optimizers, there is no ``advance`` / ``step_slices``:
``DDP.register_overlapped_optimizer(schedule="backward")`` works, ``schedule="tail"`` is refused.

CPU tensors, and parameters that are not contiguous (row-major), take an equivalent torch path.
"""
from __future__ import annotations

from collections import defaultdict

import torch

from .._native import load
from .fused import _group_key
from .layerwise import _WholeParams

__all__ = ["FusedAdafactor"]

_STATES = ("row_var", "col_var", "variance")


class FusedAdafactor(_WholeParams):
    """Adafactor without a first moment (Shazeer & Stern 2018), exactly ``torch.optim.Adafactor``.
    Per parameter tensor, with ``w`` the fp32 master (``master_weights=True``, bf16 / fp16
    parameters) or the parameter in fp32, ``g' = g * grad_scale * (-1 if maximize)`` and ``t`` the
    step count from 1::

        omb = t ** beta2_decay                  rho = min(lr, 1 / sqrt(t))
        alpha = max(eps2, RMS(w)) * rho         w <- w * (1 - lr * weight_decay)
        dim >= 2, as [B, R, C] over the last two dims:
          row_var <- lerp(row_var, mean_j g'^2, omb)      col_var <- lerp(col_var, mean_i g'^2, omb)
          var = row_var * col_var / max(mean_i row_var, eps1)
        dim <= 1:
          variance <- lerp(variance, g'^2, omb);  var = variance
        u = g' * rsqrt(max(var, eps1^2))
        w <- w - alpha / max(1, RMS(u) / d) * u

    ``eps = (eps1, eps2)``; ``eps1=None`` is ``finfo(dtype of w).eps``. State names and shapes are
    torch's (``step``, ``row_var [..., R, 1]``, ``col_var [..., 1, C]``, ``variance``; all fp32, plus
    ``master``), and a ``torch.optim.Adafactor`` state dict loads. One non-finite gradient element
    makes its whole tensor NaN and no other. A step cannot be captured into a HIP graph
    (``RuntimeError``): ``t`` is a host value baked into the launch.
    """

    def __init__(self, params, lr: float = 1e-2, beta2_decay: float = -0.8, eps=(None, 1e-3), d: float = 1.0,
                 weight_decay: float = 0.0, *, maximize: bool = False, master_weights: bool = False):
        defaults = dict(lr=lr, beta2_decay=beta2_decay, eps=eps, d=d, weight_decay=weight_decay, maximize=maximize,
                        master_weights=master_weights)
        self._check_group(defaults)
        super().__init__(params, defaults)

    def _check_group(self, group):
        eps1, eps2 = group["eps"]
        if not 0.0 <= group["lr"]:
            raise ValueError(f"Learning rate should be >= 0 but is: {group['lr']}")
        if not 0.0 >= group["beta2_decay"]:
            raise ValueError(f"beta2_decay should be <= 0 but is: {group['beta2_decay']}")
        if eps1 is not None and not 0.0 <= eps1:
            raise ValueError(f"epsilon1 should be >= 0 but is: {eps1}")
        if not 0.0 <= eps2:
            raise ValueError(f"epsilon2 should be >= 0 but is: {eps2}")
        if not 1.0 <= group["d"]:
            raise ValueError(f"Clipping threshold d should be >= 1 but is: {group['d']}")
        if not 0.0 <= group["weight_decay"]:
            raise ValueError(f"weight_decay should be >= 0 but is: {group['weight_decay']}")

    def _check(self, work):
        if torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdafactor cannot be captured into a HIP graph: the step count is a host value "
                               "baked into the launch (omb = t ** beta2_decay, rho = min(lr, 1 / sqrt(t))); step "
                               "outside the capture")
        super()._check(work)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():  # torch's: a 0-dim CPU tensor `step`, states in the parameter's dtype
            if "step" in st:
                st["step"] = int(st["step"])
            for key in _STATES:
                if key in st:
                    st[key] = st[key].float().contiguous()

    def _step_group(self, group, items, grad_scale):
        eps1, eps2 = group["eps"]
        buckets = defaultdict(lambda: ([], [], [], [], [], []))
        for p, g in items:
            st = self.state[p]
            if "step" not in st:
                st["step"] = 0
                if p.dim() > 1:
                    st["row_var"] = torch.zeros(p.shape[:-1] + (1,), dtype=torch.float32, device=p.device)
                    st["col_var"] = torch.zeros(p.shape[:-2] + (1,) + p.shape[-1:], dtype=torch.float32,
                                                device=p.device)
                else:
                    st["variance"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            st["step"] += 1
            use_master = self._master(p, group)
            fused = p.device.type == "cuda" and p.is_contiguous() and g.is_contiguous() and (
                not use_master or st["master"].is_contiguous())
            b = buckets[_group_key(p, g) + (st["step"], use_master, p.dim() > 1, fused)]
            b[0].append(p), b[1].append(g)
            for slot, key in zip(b[2:5], _STATES):
                if key in st:
                    slot.append(st[key])
            if use_master:
                b[5].append(st["master"])
        for (dev, pdt, gdt, step, use_master, matrix, fused), (ps, gs, rvs, cvs, vs, masters) in buckets.items():
            e1 = torch.finfo(torch.float32 if use_master else pdt).eps if eps1 is None else eps1
            args = (group["lr"], group["beta2_decay"], e1, eps2, group["d"], group["weight_decay"], step,
                    group["maximize"], grad_scale)
            (load().fused_adafactor if fused else self._torch_step)(ps, gs, rvs, cvs, vs, masters, *args)

    @staticmethod
    def _torch_step(ps, gs, rvs, cvs, vs, masters, lr, beta2_decay, eps1, eps2, d, weight_decay, step, maximize,
                    grad_scale):
        """The same formulas as torch ops on device scalars (no ``.item()``)."""
        omb, rho = float(step) ** beta2_decay, min(lr, 1.0 / float(step) ** 0.5)
        for i, (p, g) in enumerate(zip(ps, gs)):
            if p.numel() == 0:
                continue
            w = masters[i] if masters else p.float()
            gg = g.float()
            if grad_scale is not None:
                gg = gg * grad_scale.float().reshape(())
            if maximize:
                gg = -gg
            root_n = p.numel() ** 0.5
            alpha = (torch.linalg.vector_norm(w) / root_n).clamp_min(eps2) * rho
            if weight_decay != 0:
                w = w * (1 - lr * weight_decay)
            if p.dim() > 1:
                rvs[i].lerp_(gg.square().mean(dim=-1, keepdim=True), omb)
                cvs[i].lerp_(gg.square().mean(dim=-2, keepdim=True), omb)
                var = rvs[i] * cvs[i] / rvs[i].mean(dim=-2, keepdim=True).clamp_min(eps1)
            else:
                vs[i].lerp_(gg * gg, omb)
                var = vs[i]
            u = gg * var.clamp_min(eps1 * eps1).rsqrt()
            w = w - alpha / (torch.linalg.vector_norm(u) / (root_n * d)).clamp_min(1.0) * u
            if masters:
                masters[i].copy_(w)
            p.copy_(w)
