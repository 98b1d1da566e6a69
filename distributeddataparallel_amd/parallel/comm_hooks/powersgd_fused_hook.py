"""PowerSGD gradient compression on the fused kernels (``ops/powersgd.py``,
``csrc/kernels/powersgd.hip``).

Per bucket the semantics are those of :func:`powerSGD_hook.powerSGD_hook`: a plain all-reduce
before ``start_powerSGD_iter``; after it every gradient that ``_should_compress`` accepts is viewed
as an ``n x m`` matrix, ``M' = G + E`` is approximated by ``P Q^T`` with one power-iteration step
(``P = M' Q``, all-reduce, orthonormalize, ``Q = M'^T P``, all-reduce, ``G = P Q^T / W``), and the
other tensors are all-reduced uncompressed in one flat buffer. ``Q`` is drawn on the CPU in fp32
from ``state.rng`` on first use (every step with ``warm_start=False``).

What differs: ``P``, ``Q`` and the error memory ``E`` are fp32 whatever the bucket dtype; ``E`` is
updated by the reconstruct kernel as ``(G + E) - G_new`` (no clone of the bucket, no subtraction
pass); ``1 / W`` is folded into the reconstruct; and the launch tables, ``P`` / ``Q`` / ``E`` and the
partial-sum workspace are cached per ``(bucket index, numel, dtype, device)``, so a steady-state
step allocates nothing. A step is 4 passes over ``G`` and ``E`` (two reads for the products, one
read and one write for the reconstruct) and, per table of 40 matrices and rank, 9 to 11 launches.

Every collective is waited on where the existing hook waits (on the GPU backends that is stream
ordering). With ``state.error(bucket_index)`` and ``state.q_memory(bucket_index)`` the fp32 buffers
can be read: ``E`` has the bucket's layout, ``Q`` is the ``[m_i, r_i]`` blocks of
``state.layout(bucket_index)`` back to back.

Not covered: HIP-graph capture of the hook, the batched variant (the whole bucket as one square
matrix), ranks above 32 and fp64 buckets.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple

import torch

from ... import distributed as xdist
from ...ops import powersgd as psgd
from .default_hooks import _allreduce_fut
from .powerSGD_hook import _should_compress

__all__ = ["FusedPowerSGDState", "fused_powerSGD_hook"]


class Compressed(NamedTuple):
    """One compressed gradient: its element offset in the bucket, its matrix shape, its rank and
    the element offsets of its ``P`` and ``Q`` in their flat buffers."""
    offset: int
    n: int
    m: int
    r: int
    p_offset: int
    q_offset: int


class _BucketCache:
    __slots__ = ["signature", "layout", "error", "p", "q", "plan", "rank1", "rank1_buffer", "rank1_views",
                 "fresh", "stats"]


class FusedPowerSGDState:
    """State of :func:`fused_powerSGD_hook`; the arguments are those of ``PowerSGDState``."""

    def __init__(self, process_group=None, matrix_approximation_rank: int = 1, start_powerSGD_iter: int = 1_000,
                 min_compression_rate: float = 2, use_error_feedback: bool = True, warm_start: bool = True,
                 orthogonalization_epsilon: float = 0, random_seed: int = 0):
        if not 1 <= matrix_approximation_rank <= psgd.MAX_RANK:
            raise ValueError(f"matrix_approximation_rank must be in 1..{psgd.MAX_RANK}, got "
                             f"{matrix_approximation_rank}")
        if (use_error_feedback or warm_start) and start_powerSGD_iter <= 1:
            raise ValueError("start_powerSGD_iter must be > 1 when error feedback or warm start is enabled")
        import numpy as np

        self.process_group = process_group
        self.matrix_approximation_rank = matrix_approximation_rank
        self.start_powerSGD_iter = start_powerSGD_iter
        self.min_compression_rate = min_compression_rate
        self.use_error_feedback = use_error_feedback
        self.warm_start = warm_start
        self.orthogonalization_epsilon = orthogonalization_epsilon
        self.rng = np.random.RandomState(random_seed)
        self.iter = 0
        self.total_numel_before_compression = 0
        self.total_numel_after_compression = 0
        self._cache: Dict[tuple, _BucketCache] = {}

    def maybe_increase_iter(self, bucket):
        if bucket.is_last():
            self.iter += 1

    def compression_stats(self):
        ratio = (self.total_numel_before_compression / self.total_numel_after_compression
                 if self.total_numel_after_compression > 0 else 0)
        return ratio, self.total_numel_before_compression, self.total_numel_after_compression

    def _of(self, bucket_index: int) -> _BucketCache:
        for key, c in self._cache.items():
            if key[0] == bucket_index:
                return c
        raise KeyError(f"bucket {bucket_index} has not been compressed yet")

    def error(self, bucket_index: int) -> torch.Tensor:
        """The fp32 error memory of a bucket, in the bucket's layout (``None`` without error feedback)."""
        return self._of(bucket_index).error

    def q_memory(self, bucket_index: int) -> torch.Tensor:
        return self._of(bucket_index).q

    def layout(self, bucket_index: int) -> List[Compressed]:
        return self._of(bucket_index).layout


def _bind(state: FusedPowerSGDState, bucket, flat: torch.Tensor) -> _BucketCache:
    """The cached buffers and plan of this bucket, rebuilt when the bucket's memory or layout changed."""
    tensors = bucket.gradients()
    esize, base = flat.element_size(), flat.data_ptr()
    signature = (base, tuple((t.data_ptr(), tuple(t.shape)) for t in tensors))
    key = (bucket.index(), flat.numel(), flat.dtype, flat.device)
    c = state._cache.get(key)
    if c is not None and c.signature == signature:
        return c
    layout, mats, rank1 = [], [], []
    before = after = p_off = q_off = 0
    for t in tensors:
        if not t.is_contiguous():
            raise ValueError("fused_powerSGD_hook: the bucket's gradients must be contiguous")
        m2 = t.view(t.shape[0], -1) if t.dim() >= 1 and t.numel() else t.reshape(1, -1)
        n, m = m2.shape
        r = min(n, m, state.matrix_approximation_rank)
        compress, u, cm = _should_compress(n, m, r, state.min_compression_rate)
        before += u
        off = (t.data_ptr() - base) // esize
        if compress and r >= 1:
            if off < 0 or off + u > flat.numel():
                raise ValueError("fused_powerSGD_hook: the bucket's gradients must be views of its buffer")
            layout.append(Compressed(off, n, m, r, p_off, q_off))
            mats.append(m2)
            p_off += n * r
            q_off += m * r
            after += cm
        else:
            rank1.append(t)
            after += u
    old, c = c, _BucketCache()
    c.signature, c.layout, c.rank1, c.stats = signature, layout, rank1, (before, after)
    dev = flat.device
    if old is not None and old.layout == layout:  # the same bucket at a new address: keep E, P, Q
        c.error, c.p, c.q, c.fresh = old.error, old.p, old.q, old.fresh
    else:
        c.error = torch.zeros(flat.numel(), dtype=torch.float32, device=dev) if state.use_error_feedback else None
        c.p = torch.empty(p_off, dtype=torch.float32, device=dev)
        c.q = torch.empty(q_off, dtype=torch.float32, device=dev)
        c.fresh = True
    c.plan = None
    if mats:
        errors = None if c.error is None else [c.error[x.offset:x.offset + x.n * x.m] for x in layout]
        ps = [c.p[x.p_offset:x.p_offset + x.n * x.r].view(x.n, x.r) for x in layout]
        qs = [c.q[x.q_offset:x.q_offset + x.m * x.r].view(x.m, x.r) for x in layout]
        c.plan = psgd.plan(mats, errors, ps, qs)
    total1 = sum(t.numel() for t in rank1)
    c.rank1_buffer = torch.empty(total1, dtype=flat.dtype, device=dev)
    c.rank1_views, o = [], 0
    for t in rank1:
        c.rank1_views.append(c.rank1_buffer[o:o + t.numel()].view_as(t))
        o += t.numel()
    state._cache[key] = c
    return c


def _randomize(state: FusedPowerSGDState, c: _BucketCache):
    gen = torch.Generator().manual_seed(int(state.rng.randint(1_000_000_000)))
    for x in c.layout:
        c.q[x.q_offset:x.q_offset + x.m * x.r].view(x.m, x.r).copy_(
            torch.randn(x.m, x.r, dtype=torch.float32, generator=gen))
    c.plan.orthonormalize_q(state.orthogonalization_epsilon)
    c.fresh = False


def fused_powerSGD_hook(state: FusedPowerSGDState, bucket) -> torch.futures.Future:
    pg = state.process_group if state.process_group is not None else xdist.get_default_group()
    world = pg.size()
    input_tensor = bucket.buffer()
    if state.iter < state.start_powerSGD_iter:
        state.maybe_increase_iter(bucket)
        return _allreduce_fut(pg, input_tensor)

    c = _bind(state, bucket, input_tensor.view(-1))
    state.total_numel_before_compression += c.stats[0]
    state.total_numel_after_compression += c.stats[1]
    eps = state.orthogonalization_epsilon
    if c.plan is not None:
        if c.fresh or not state.warm_start:
            _randomize(state, c)
        c.plan.project()  # P = (G + E) Q
    if c.rank1:
        torch._foreach_copy_(c.rank1_views, c.rank1)
        pg.allreduce(c.rank1_buffer).wait()
        c.rank1_buffer.div_(world)
        torch._foreach_copy_(c.rank1, c.rank1_views)
    if c.plan is not None:
        pg.allreduce(c.p).wait()
        c.plan.orthonormalize_p(eps)
        c.plan.backproject()  # Q = (G + E)^T P
        pg.allreduce(c.q).wait()
        c.plan.reconstruct(1.0 / world)  # G = P Q^T / W, E = (G + E) - G
    state.maybe_increase_iter(bucket)
    fut = torch.futures.Future()
    fut.set_result(input_tensor)
    return fut
