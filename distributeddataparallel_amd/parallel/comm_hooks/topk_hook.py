"""Top-k sparsified gradient all-reduce with error feedback (``ops/topk.py``,
``csrc/kernels/topk_comm.hip``): block-wise top-k selection with memory (Stich et al. 2018,
"Sparsified SGD with memory"; the sparsification of Deep Gradient Compression, Lin et al. 2018),
applied to the gradient buckets.

Before iteration ``start_iter`` the hook is the plain averaging all-reduce (``state.iter`` advances
on the last bucket of a backward, as in the PowerSGD hooks). After it,
``TopKState(algorithm="twoshot")`` (default) runs, per bucket of ``n`` elements on ``W`` ranks:

1. compress ``bucket + worker residual`` into ``W`` segments, segment ``r`` being the chunk rank
   ``r`` owns: every block of ``block`` elements keeps its ``k`` largest; the worker residual
   (fp32, ``n`` long) keeps the rest;
2. all-to-all: every rank receives the ``W`` versions of its own chunk;
3. ``reduce_reselect``: their mean plus the server residual (fp32, ``n / W`` long), selected
   again, without a copy of the mean in memory; the server residual keeps the rest;
4. all-gather of the ``W`` reduced chunks;
5. ``decode_mean(mode="concat")`` into the bucket.

A rank sends and receives ``2 (W - 1) / W * n * 6 k / block`` bytes. ``algorithm="allgather"``
(compress one segment, all-gather, ``decode_mean(mode="mean")``) moves ``(W - 1) * n * 6 k / block``
bytes, compresses once, needs the worker residual only, and is the only one on the ``"peer"``
backend, which has no all-to-all. Either way every rank decodes the same bytes with the same
arithmetic, so the replicas stay bitwise identical.

The steps are chained on the collectives' futures and ordered across buckets as in
:mod:`q8_hook`. Payloads and residuals are cached per bucket, so a steady-state step allocates
nothing; ``state.worker_error(i)`` and ``state.server_error(i)`` return bucket ``i``'s residuals.
When the bucket layout changes (the rebuild after the first iteration) the residuals of the old
layout are dropped and the new ones start at zero.

Not covered: global (whole-bucket) top-k and thresholds estimated by sampling, the momentum
correction and factor masking of DGC, bf16 values on the wire, variable-length payloads,
checkpointing the residuals, HIP-graph capture of the hook, ``comm_dtype`` integration, and the
convergence of any model. The rounding of the decoded mean to a bf16 / fp16 bucket is not fed back
into a residual.
"""
from __future__ import annotations

import torch

from ... import distributed as xdist
from ...ops import topk
from .default_hooks import _allreduce_fut
from .q8_hook import ALGORITHMS, _issue_in_order, _then

__all__ = ["TopKState", "topk_allreduce_hook"]


class _Buffers:
    __slots__ = ["key", "send", "recv", "reduced", "gathered", "worker_error", "server_error"]


class TopKState:
    """State of :func:`topk_allreduce_hook`: the process group (``None``: the default group), the
    block size, the entries kept per block, the algorithm, the first compressed iteration, and the
    payload and residual buffers, cached per bucket."""

    def __init__(self, process_group=None, block: int = 2048, k: int = 32, algorithm: str = "twoshot",
                 start_iter: int = 1_000):
        if algorithm not in ALGORITHMS:
            raise ValueError(f"TopKState: algorithm must be one of {ALGORITHMS}, got {algorithm!r}")
        if block not in topk.BLOCKS:
            raise ValueError(f"TopKState: block must be one of {topk.BLOCKS}, got {block}")
        if k not in topk.KS:
            raise ValueError(f"TopKState: k must be one of {topk.KS}, got {k}")
        if start_iter < 0:
            raise ValueError(f"TopKState: start_iter must be >= 0, got {start_iter}")
        self.process_group = process_group
        self.block = block
        self.k = k
        self.algorithm = algorithm
        self.start_iter = start_iter
        self.iter = 0
        self._buffers = {}  # bucket index -> _Buffers
        self._issued = None  # future: the bucket before this one has issued its last collective

    def maybe_increase_iter(self, bucket):
        if bucket.is_last():
            self.iter += 1

    def buffers(self, bucket, world: int) -> _Buffers:
        """The payload buffers and residuals of this bucket; new, zero residuals on first use."""
        buf = bucket.buffer()
        key = (bucket.index(), buf.numel(), buf.dtype, buf.device, world)
        b = self._buffers.get(bucket.index())
        if b is not None and b.key == key:
            return b
        if b is not None:  # another layout: none of its buckets' residuals describes this one
            self._buffers.clear()

        def new(count, dtype=torch.uint8):
            return torch.zeros(count, dtype=dtype, device=buf.device)

        b = _Buffers()
        b.key = key
        b.worker_error = new(buf.numel(), torch.float32)
        if self.algorithm == "twoshot":
            full = topk.payload_bytes(buf.numel(), self.block, self.k, world)
            chunk = full // world // (6 * self.k) * self.block
            b.send, b.recv, b.reduced, b.gathered = new(full), new(full), new(full // world), new(full)
            b.server_error = new(chunk, torch.float32)
        else:
            one = topk.payload_bytes(buf.numel(), self.block, self.k, 1)
            b.send, b.recv, b.reduced, b.gathered, b.server_error = new(one), new(world * one), None, None, None
        self._buffers[bucket.index()] = b
        return b

    def worker_error(self, bucket_index: int) -> torch.Tensor:
        """The fp32 residual of bucket ``bucket_index`` on this rank, in the bucket's layout."""
        return self._buffers[bucket_index].worker_error

    def server_error(self, bucket_index: int) -> torch.Tensor:
        """The fp32 residual of the chunk of bucket ``bucket_index`` that this rank reduces
        (``None`` for ``algorithm="allgather"``)."""
        return self._buffers[bucket_index].server_error


def topk_allreduce_hook(state: TopKState, bucket) -> torch.futures.Future:
    pg = state.process_group if state.process_group is not None else xdist.get_default_group()
    w, block, k = pg.size(), state.block, state.k
    if state.algorithm == "twoshot" and pg.backend == "peer":
        raise RuntimeError('topk_allreduce_hook: the "peer" backend has no all-to-all; use '
                           'TopKState(algorithm="allgather")')
    buf = bucket.buffer()
    if state.iter < state.start_iter:
        state.maybe_increase_iter(bucket)
        return _allreduce_fut(pg, buf)
    state.maybe_increase_iter(bucket)
    flat = buf.view(-1)
    b = state.buffers(bucket, w)
    done = torch.futures.Future()

    if state.algorithm == "allgather":
        topk.compress(flat, b.worker_error, block, k, 1, out=b.send)

        def finish():
            topk.decode_mean(b.recv, flat, block, k, w, "mean")
            done.set_result(buf)

        _then(pg.allgather_into_tensor(b.recv, b.send).get_future(), done, finish)
        return done

    topk.compress(flat, b.worker_error, block, k, w, out=b.send)
    chunk = b.server_error.numel()
    real = min(max(flat.numel() - pg.rank() * chunk, 0), chunk)  # elements of this rank's chunk
    issued = torch.futures.Future()

    def finish():
        topk.decode_mean(b.gathered, flat, block, k, w, "concat")
        done.set_result(buf)

    def gather():
        topk.reduce_reselect(b.recv, b.server_error, block, k, w, real, out=b.reduced)
        fut = pg.allgather_into_tensor(b.gathered, b.reduced).get_future()
        issued.set_result(None)
        _then(fut, done, finish)

    def exchange():
        _then(pg.alltoall_base(b.recv, b.send).get_future(), done, gather)

    _issue_in_order(state, issued, done, exchange)
    return done
