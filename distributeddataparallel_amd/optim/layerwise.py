"""Layer-wise trust-ratio optimizers on the multi-tensor HIP kernels: ``FusedLAMB`` (Apex
``FusedLAMB`` semantics) and ``FusedLARS`` (Apex ``LARC(clip=False)`` over SGD).

Both scale each parameter tensor's update by a ratio of L2 norms taken over that whole tensor, so a
step is three stream-ordered launches per (dtype group x 40 tensors): per-chunk sums of squares, one
fold per tensor, the update. Nothing synchronises with the host. A chunked update cannot know a
tensor's norm before its last chunk is there, so neither class has ``advance`` / ``step_slices``:
``DDP.register_overlapped_optimizer(schedule="backward")`` works (buckets hold whole parameters),
``schedule="tail"`` is refused.

CPU tensors take an equivalent torch path (the GPU-free test backend).
"""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, Optional

import torch
from torch.optim import Optimizer

from .._native import load
from .fused import FusedSGD, _dense_like, _group_key, _KeepStateDtypes

__all__ = ["FusedLAMB", "FusedLARS"]

_LOW = (torch.bfloat16, torch.float16)


def _trust(ok_num, ok_den, value):
    """``value`` where both norms are non-zero, else 1 (a NaN norm compares non-zero: not masked)."""
    return torch.where((ok_num != 0) & (ok_den != 0), value, torch.ones_like(value))


class _LayerWise(_KeepStateDtypes, Optimizer):
    """What the two classes share: whole-parameter stepping and the record of the last ratios."""

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self.__dict__.pop("_group_of", None)

    def _check(self, work):
        """Every refusal, over all of ``work`` = ``[(group, [(param, grad)])]``, before any state is
        created or any step count advances."""
        for group, items in work:
            self._check_group(group)
            for p, g in items:
                if p.dtype == torch.float64 or g.dtype == torch.float64:
                    raise TypeError(f"{type(self).__name__}: fp64 parameters / gradients are not supported "
                                    f"(fp32, bf16 or fp16)")

    def _check_group(self, group):
        pass

    def _group_index(self, p):
        if not hasattr(self, "_group_of"):
            self._group_of = {id(q): gi for gi, grp in enumerate(self.param_groups) for q in grp["params"]}
        return self._group_of.get(id(p))

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[torch.Tensor] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = [(group, [(p, p.grad) for p in group["params"] if p.grad is not None]) for group in self.param_groups]
        self._check(work)
        self._ratios = {}
        for group, items in work:
            self._step_group(group, items, grad_scale)
        return loss

    @torch.no_grad()
    def step_params(self, params, grads):
        """Step only ``params`` (whole parameters) with the given gradients, e.g. one DDP bucket's
        reduced views from the overlapped optimizer's ``schedule="backward"``: the same update as
        ``step`` for those parameters."""
        per_group = defaultdict(list)
        for p, g in zip(params, grads):
            gi = self._group_index(p)
            if g is not None and gi is not None:
                per_group[gi].append((p, g if g.shape == p.shape else g.view_as(p)))
        work = [(self.param_groups[gi], items) for gi, items in per_group.items()]
        self._check(work)
        if not hasattr(self, "_ratios"):
            self._ratios = {}
        for group, items in work:
            self._step_group(group, items, None)

    def trust_ratios(self) -> Dict[torch.Tensor, torch.Tensor]:
        """``{param: 0-dim fp32 tensor on the parameter's device}``: the ratio each parameter's last
        update was scaled by (1 where layer adaptation is off). Reading it does not synchronise."""
        return dict(getattr(self, "_ratios", {}))

    def _record(self, params, ratios):
        for p, r in zip(params, ratios.unbind(0) if torch.is_tensor(ratios) else ratios):
            self._ratios[p] = r

    def _master(self, p, group):
        st = self.state[p]
        use = group["master_weights"] and p.dtype in _LOW
        if use and "master" not in st:
            st["master"] = p.detach().float().clone(memory_format=torch.preserve_format)
        return use


class FusedLAMB(_LayerWise):
    """LAMB (You et al. 2020; Apex ``FusedLAMB`` semantics). Per parameter tensor, with ``w`` the fp32
    master (``master_weights=True``, bf16 / fp16 parameters) or the parameter in fp32 and
    ``g' = g * grad_scale * (-1 if maximize)``::

        m = b1 m + (1 - b1) g'            v = b2 v + (1 - b2) g'^2
        u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + weight_decay * w
        r = |w| / |u|   if weight_decay != 0 or always_adapt, else 1;  1 where |w| == 0 or |u| == 0
        w <- w - lr * r * u

    ``bc1 = 1 - b1^t``, ``bc2 = 1 - b2^t`` (both 1 with ``bias_correction=False``); the norms are L2
    over the whole tensor. A zero-initialised tensor therefore still trains (``r = 1``), and a
    non-finite norm is not masked: one NaN gradient element makes its whole tensor NaN at once.
    Moments and masters are fp32 with the parameter's strides.
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.01,
                 bias_correction: bool = True, always_adapt: bool = False, maximize: bool = False,
                 master_weights: bool = False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, bias_correction=bias_correction,
                        always_adapt=always_adapt, maximize=maximize, master_weights=master_weights)
        super().__init__(params, defaults)

    def _step_group(self, group, items, grad_scale):
        b1, b2 = group["betas"]
        adapt = group["weight_decay"] != 0 or group["always_adapt"]
        buckets = defaultdict(lambda: ([], [], [], [], []))
        for p, g in items:
            st = self.state[p]
            if "step" not in st:
                st["step"] = 0
                st["exp_avg"] = _dense_like(p).zero_()
                st["exp_avg_sq"] = _dense_like(p).zero_()
            st["step"] += 1
            use_master = self._master(p, group)
            b = buckets[_group_key(p, g) + (st["step"], use_master)]
            b[0].append(p), b[1].append(g), b[2].append(st["exp_avg"]), b[3].append(st["exp_avg_sq"])
            if use_master:
                b[4].append(st["master"])
        for (dev, pdt, gdt, step, use_master), (ps, gs, m1, m2, masters) in buckets.items():
            if dev.type == "cuda":
                ratios = load().fused_lamb(ps, gs, m1, m2, masters, group["lr"], b1, b2, group["eps"],
                                           group["weight_decay"], step, group["bias_correction"], adapt,
                                           group["maximize"], grad_scale)
            else:
                ratios = self._cpu_step(ps, gs, m1, m2, masters, group, step, adapt, grad_scale)
            self._record(ps, ratios)

    @staticmethod
    def _cpu_step(ps, gs, m1, m2, masters, group, step, adapt, grad_scale):
        b1, b2 = group["betas"]
        lr, eps, wd = group["lr"], group["eps"], group["weight_decay"]
        bc1, bc2 = (1 - b1 ** step, 1 - b2 ** step) if group["bias_correction"] else (1.0, 1.0)
        ratios = []
        for i, (p, g) in enumerate(zip(ps, gs)):
            w = masters[i] if masters else p.float()
            gg = g.float() * (grad_scale.float() if grad_scale is not None else 1.0)
            if group["maximize"]:
                gg = -gg
            m1[i].mul_(b1).add_(gg, alpha=1 - b1)
            m2[i].mul_(b2).addcmul_(gg, gg, value=1 - b2)
            u = (m1[i] / bc1) / (m2[i].sqrt() / (bc2 ** 0.5)).add_(eps)
            if wd != 0:
                u = u + wd * w
            r = torch.ones((), dtype=torch.float32)
            if adapt:
                wn, un = torch.linalg.vector_norm(w), torch.linalg.vector_norm(u)
                r = _trust(wn, un, wn / un)
            w = w - lr * r * u
            if masters:
                masters[i].copy_(w)
            p.copy_(w)
            ratios.append(r)
        return ratios


class FusedLARS(_LayerWise):
    """LARS (You et al. 2017; Apex ``LARC(clip=False)`` over SGD). Per parameter tensor, with ``w``
    the fp32 master or the parameter in fp32 and ``g' = g * grad_scale * (-1 if maximize)``::

        lam = trust_coefficient * |w| / (|g'| + weight_decay * |w| + eps);  1 where |w| == 0 or |g'| == 0
        d   = lam * (g' + weight_decay * w)

    and then ``torch.optim.SGD`` on ``d``: the first step sets ``buf = d``, later ones
    ``buf = momentum * buf + (1 - dampening) * d``; Nesterov steps along ``d + momentum * buf``;
    ``w <- w - lr * direction``. A param group with ``layer_adaptation=False`` (the usual home of
    biases and BatchNorm parameters) is updated by ``FusedSGD``'s kernels, bit for bit.
    """

    def __init__(self, params, lr: float, momentum: float = 0.9, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, trust_coefficient: float = 1e-3, eps: float = 1e-8,
                 layer_adaptation: bool = True, maximize: bool = False, master_weights: bool = False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        trust_coefficient=trust_coefficient, eps=eps, layer_adaptation=layer_adaptation,
                        maximize=maximize, master_weights=master_weights)
        super().__init__(params, defaults)

    def _check_group(self, group):
        if group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def _step_group(self, group, items, grad_scale):
        C = load()
        mom = group["momentum"]
        buckets = defaultdict(lambda: ([], [], [], []))
        for p, g in items:
            st = self.state[p]
            first = "momentum_buffer" not in st
            if mom != 0 and first:
                st["momentum_buffer"] = _dense_like(p)
            use_master = self._master(p, group)
            b = buckets[_group_key(p, g) + (first, use_master)]
            b[0].append(p), b[1].append(g), b[2].append(st.get("momentum_buffer"))
            if use_master:
                b[3].append(st["master"])
        sgd = (group["lr"], mom, group["dampening"], group["weight_decay"], group["nesterov"], group["maximize"])
        for (dev, pdt, gdt, first, use_master), (ps, gs, bufs, masters) in buckets.items():
            bufs = bufs if mom != 0 else []
            if dev.type != "cuda":
                ratios = self._cpu_step(ps, gs, bufs, masters, group, first, grad_scale)
            elif group["layer_adaptation"]:
                ratios = C.fused_lars(ps, gs, bufs, masters, *sgd, first, group["trust_coefficient"], group["eps"],
                                      grad_scale)
            else:  # exactly FusedSGD
                if use_master:
                    C.fused_sgd_master(masters, gs, bufs, ps, *sgd, first, grad_scale)
                else:
                    C.fused_sgd(ps, gs, bufs, *sgd, first, grad_scale)
                ratios = torch.ones(len(ps), dtype=torch.float32, device=dev)
            self._record(ps, ratios)

    @staticmethod
    def _cpu_step(ps, gs, bufs, masters, group, first, grad_scale):
        ws = masters if masters else ps
        if not group["layer_adaptation"]:
            FusedSGD._cpu_step(ws, gs, bufs, group, first, grad_scale)
            ratios = [torch.ones((), dtype=torch.float32) for _ in ps]
        else:
            lr, mom, damp, wd = group["lr"], group["momentum"], group["dampening"], group["weight_decay"]
            ratios = []
            for i, (w, g) in enumerate(zip(ws, gs)):
                wf, d = w.float(), g.float()
                scale = grad_scale.float().reshape(()) if grad_scale is not None else torch.ones(())
                wn, gn = torch.linalg.vector_norm(wf), torch.linalg.vector_norm(d) * scale.abs()
                lam = _trust(wn, gn, group["trust_coefficient"] * wn / (gn + wd * wn + group["eps"]))
                d = d * (-scale if group["maximize"] else scale)
                if wd != 0:
                    d = d + wd * wf
                d = lam * d
                if mom != 0:
                    buf = bufs[i]
                    if first:
                        buf.copy_(d)
                    else:
                        buf.mul_(mom).add_(d, alpha=1 - damp)
                    d = d + mom * buf if group["nesterov"] else buf
                w.copy_(wf - lr * d)
                ratios.append(lam)
        if masters:
            for m, p in zip(masters, ps):
                p.copy_(m)
        return ratios
