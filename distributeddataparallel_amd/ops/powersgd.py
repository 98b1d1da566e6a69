"""One PowerSGD power-iteration step on a list of matrices (``csrc/kernels/powersgd.hip``).

``mats`` are row-major ``[n, m]`` views ``G`` of a gradient bucket (fp32 / bf16 / fp16, any alignment),
``errors`` their fp32 error memories ``E`` (``None``: no error feedback), ``ps`` fp32 ``[n, r]`` and
``qs`` fp32 ``[m, r]`` with ``1 <= r <= min(n, m, 32)``. With ``M' = G + E``, formed in fp32 and
never stored:

* ``project``:        ``P = M' Q``;
* ``orthonormalize``: CholeskyQR2, ``X <- X L^-T`` twice with
  ``L L^T = X^T X + (max(epsilon, 0) + 1e-10 * max diag + 1e-30) I`` (the rules of
  ``comm_hooks.powerSGD_hook._orthogonalize``), in fp32;
* ``backproject``:    ``Q = M'^T P``;
* ``reconstruct``:    ``A = inv_world * P Q^T`` rounded to the dtype of ``G``, then
  ``E <- (G + E) - float(A)`` and ``G <- A``: what the optimizer sees plus what is remembered is
  what came in, to one fp32 rounding.

CUDA tensors run the HIP kernels; CPU tensors run the same rules in torch (fp32 accumulation, the
same regularisation, the same rounding of ``A``), so a hook built on these ops works on the CPU
backend too. :func:`plan` binds one list once (on the GPU: the launch tables and the partial-sum
workspace), for a caller that repeats the step on the same buffers.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

__all__ = ["MAX_RANK", "plan", "project", "orthonormalize", "backproject", "reconstruct"]

MAX_RANK = 32
_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _check_nr(x: torch.Tensor, name: str):
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"powersgd: {name} must be a contiguous fp32 [rows, r] tensor, got "
                         f"{x.dtype} {tuple(x.shape)}")
    if not 1 <= x.shape[1] <= MAX_RANK:
        raise ValueError(f"powersgd: rank must be in 1..{MAX_RANK}, got {x.shape[1]}")
    if x.shape[1] > x.shape[0]:
        raise ValueError(f"powersgd: {name} has more columns than rows: {tuple(x.shape)}")


def _check(mats, errors, ps, qs):
    if not (len(mats) == len(ps) == len(qs)) or (errors is not None and len(errors) != len(mats)):
        raise ValueError("powersgd: the lists must have one entry per matrix")
    for i, g in enumerate(mats):
        if g.dim() != 2 or not g.is_contiguous() or g.numel() == 0:
            raise ValueError(f"powersgd: matrix {i} must be a non-empty contiguous 2-D view, got {tuple(g.shape)} "
                             f"with strides {g.stride()}")
        if g.dtype not in _DTYPES or g.dtype != mats[0].dtype:
            raise ValueError(f"powersgd: matrices must share one dtype of fp32 / bf16 / fp16, got {g.dtype}")
        _check_nr(ps[i], "P")
        _check_nr(qs[i], "Q")
        n, m = g.shape
        if ps[i].shape[0] != n or qs[i].shape[0] != m or ps[i].shape[1] != qs[i].shape[1]:
            raise ValueError(f"powersgd: matrix {i} is {n} x {m} but P is {tuple(ps[i].shape)} and Q "
                             f"{tuple(qs[i].shape)}")
        if errors is not None:
            e = errors[i]
            if e.dtype != torch.float32 or not e.is_contiguous() or e.numel() != g.numel():
                raise ValueError(f"powersgd: error memory {i} must be contiguous fp32 with {g.numel()} elements")
        if any(t.device != g.device for t in (ps[i], qs[i]) + (() if errors is None else (errors[i],))):
            raise ValueError("powersgd: all tensors of a matrix must be on its device")


def _ortho_cpu(x: torch.Tensor, epsilon: float):
    for _ in range(2):
        gram = x.t() @ x
        gram.diagonal().add_(max(epsilon, 0.0) + 1e-10 * gram.diagonal().amax() + 1e-30)
        chol, _ = torch.linalg.cholesky_ex(gram)
        inv = torch.linalg.solve_triangular(chol, torch.eye(x.shape[1]), upper=False)  # L^-1
        x.copy_(x @ inv.t())


class _CpuPlan:
    def __init__(self, mats, errors, ps, qs):
        self.mats, self.errors, self.ps, self.qs = mats, errors, ps, qs

    def _m(self, i):
        g = self.mats[i].float()
        return g if self.errors is None else g + self.errors[i].view_as(g)

    def project(self):
        for i, (p, q) in enumerate(zip(self.ps, self.qs)):
            torch.matmul(self._m(i), q, out=p)

    def backproject(self):
        for i, (p, q) in enumerate(zip(self.ps, self.qs)):
            torch.matmul(self._m(i).t(), p, out=q)

    def reconstruct(self, inv_world: float):
        for i, (g, p, q) in enumerate(zip(self.mats, self.ps, self.qs)):
            a = ((p @ q.t()) * inv_world).to(g.dtype)
            if self.errors is not None:
                self.errors[i].view_as(g).copy_(self._m(i) - a.float())
            g.copy_(a)

    def orthonormalize_p(self, epsilon: float = 0.0):
        for p in self.ps:
            _ortho_cpu(p, epsilon)

    def orthonormalize_q(self, epsilon: float = 0.0):
        for q in self.qs:
            _ortho_cpu(q, epsilon)


def plan(mats: Sequence[torch.Tensor], errors: Optional[Sequence[torch.Tensor]], ps: Sequence[torch.Tensor],
         qs: Sequence[torch.Tensor]):
    """An object with ``project()``, ``orthonormalize_p(eps)``, ``orthonormalize_q(eps)``,
    ``backproject()`` and ``reconstruct(inv_world)`` bound to these tensors."""
    mats, ps, qs = list(mats), list(ps), list(qs)
    errors = None if errors is None else list(errors)
    _check(mats, errors, ps, qs)
    if not mats:
        raise ValueError("powersgd: empty matrix list")
    if mats[0].is_cuda:
        from .._native import load

        return load().PsgdPlan(mats, errors or [], ps, qs)
    return _CpuPlan(mats, errors, ps, qs)


def project(mats, errors, qs, ps) -> List[torch.Tensor]:
    """``ps[i] = (mats[i] + errors[i]) @ qs[i]``."""
    plan(mats, errors, ps, qs).project()
    return ps


def backproject(mats, errors, ps, qs) -> List[torch.Tensor]:
    """``qs[i] = (mats[i] + errors[i])^T @ ps[i]``."""
    plan(mats, errors, ps, qs).backproject()
    return qs


def reconstruct(mats, errors, ps, qs, inv_world: float = 1.0):
    """``mats[i] <- round(inv_world * ps[i] @ qs[i]^T)``, ``errors[i] <- (mats[i] + errors[i]) - mats[i]_new``."""
    plan(mats, errors, ps, qs).reconstruct(float(inv_world))
    return mats


def orthonormalize(mats_nr: Sequence[torch.Tensor], epsilon: float = 0.0):
    """CholeskyQR2 of every ``[n, r]`` fp32 matrix of the list, in place."""
    mats_nr = list(mats_nr)
    for x in mats_nr:
        _check_nr(x, "a matrix to orthonormalize")
    if not mats_nr:
        return mats_nr
    if mats_nr[0].is_cuda:
        from .._native import load

        load().psgd_orthonormalize(mats_nr, float(epsilon))
    else:
        for x in mats_nr:
            _ortho_cpu(x, epsilon)
    return mats_nr
