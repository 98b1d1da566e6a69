"""8-bit block-quantized gradient all-reduce (``ops/q8.py``, ``csrc/kernels/q8_comm.hip``).

``Q8State(algorithm="twoshot")`` (default), per bucket of ``n`` elements on ``W`` ranks:

1. quantize the bucket into ``W`` segments, segment ``r`` being the chunk rank ``r`` owns;
2. all-to-all: every rank receives the ``W`` versions of its own chunk;
3. ``reduce_requantize``: their mean, quantized again, without an fp32 copy in memory;
4. all-gather of the ``W`` reduced chunks;
5. ``dequantize_mean(mode="concat")`` into the bucket.

A rank sends and receives ``2 (W - 1) / W * n * (1 + 8 / block)`` bytes, against ``(W - 1) * n``
for ``algorithm="allgather"`` (quantize one segment, all-gather, ``dequantize_mean(mode="mean")``),
which quantizes once instead of twice and is the better choice for W = 2 and the only one on the
``"peer"`` backend, which has no all-to-all. Either way every rank decodes the same bytes with
the same arithmetic, so the replicas stay bitwise identical.

The hook never blocks its caller: each step runs in a ``then`` callback of the collective before
it and the returned future is completed by the last one. On the GPU backends those futures are
complete at once (the stream is ordered after the collective), so everything is issued inline. With
CPU tensors the second collective is issued from the completion thread; the hook then holds back a
bucket's first collective until the bucket before it has issued its second, so that all ranks
issue the same sequence. Collectives issued by others between a backward's first and last bucket
(``find_unused_parameters`` does one) are outside that ordering: use ``"allgather"`` with them on
CPU tensors.

Not covered: error feedback, stochastic rounding, 4-bit codes, ``comm_dtype`` integration and
HIP-graph capture of the hook.
"""
from __future__ import annotations

import torch

from ... import distributed as xdist
from ...ops import q8

__all__ = ["Q8State", "q8_allreduce_hook"]

ALGORITHMS = ("twoshot", "allgather")


class Q8State:
    """State of :func:`q8_allreduce_hook`: the process group (``None``: the default group), the
    block size and the algorithm, and the payload buffers, cached per bucket."""

    def __init__(self, process_group=None, block: int = 512, algorithm: str = "twoshot"):
        if algorithm not in ALGORITHMS:
            raise ValueError(f"Q8State: algorithm must be one of {ALGORITHMS}, got {algorithm!r}")
        if block not in q8.BLOCKS:
            raise ValueError(f"Q8State: block must be one of {q8.BLOCKS}, got {block}")
        self.process_group = process_group
        self.block = block
        self.algorithm = algorithm
        self._buffers = {}
        self._issued = None  # future: the bucket before this one has issued its last collective

    def buffers(self, bucket, world: int):
        """(send, recv[, reduced, gathered]) uint8 payload buffers for this bucket."""
        buf = bucket.buffer()
        key = (bucket.index(), buf.numel(), buf.dtype, buf.device, world)
        bufs = self._buffers.get(key)
        if bufs is None:
            def new(nbytes):
                return torch.empty(nbytes, dtype=torch.uint8, device=buf.device)

            if self.algorithm == "twoshot":
                full = q8.payload_bytes(buf.numel(), self.block, world)
                bufs = (new(full), new(full), new(full // world), new(full))
            else:
                one = q8.payload_bytes(buf.numel(), self.block, 1)
                bufs = (new(one), new(world * one))
            self._buffers[key] = bufs
        return bufs


def _then(fut, done, step):
    """Run ``step`` when ``fut`` completes; a failure of either goes to the future ``done``."""
    def callback(f):
        try:
            f.wait()
            step()
        except Exception as e:  # noqa: BLE001 — surfaced through the hook's future
            done.set_exception(e)

    fut.then(callback)


def _issue_in_order(state, issued, done, exchange):
    """Run ``exchange`` (a bucket's first collective) once the bucket before it on ``state`` has
    issued its second; the caller completes ``issued`` when this bucket has issued its own."""
    # after a failure too: the next bucket must not wait for ever
    done.add_done_callback(lambda _: issued.done() or issued.set_result(None))
    before, state._issued = state._issued, issued
    if before is None or before.done():
        exchange()
    else:
        _then(before, done, exchange)


def q8_allreduce_hook(state: Q8State, bucket) -> torch.futures.Future:
    pg = state.process_group if state.process_group is not None else xdist.get_default_group()
    w, block = pg.size(), state.block
    if state.algorithm == "twoshot" and pg.backend == "peer":
        raise RuntimeError('q8_allreduce_hook: the "peer" backend has no all-to-all; use '
                           'Q8State(algorithm="allgather")')
    buf = bucket.buffer()
    flat = buf.view(-1)
    done = torch.futures.Future()

    if state.algorithm == "allgather":
        send, recv = state.buffers(bucket, w)
        q8.quantize(flat, block, 1, out=send)

        def finish():
            q8.dequantize_mean(recv, flat, block, w, "mean")
            done.set_result(buf)

        _then(pg.allgather_into_tensor(recv, send).get_future(), done, finish)
        return done

    send, recv, reduced, gathered = state.buffers(bucket, w)
    q8.quantize(flat, block, w, out=send)
    issued = torch.futures.Future()

    def finish():
        q8.dequantize_mean(gathered, flat, block, w, "concat")
        done.set_result(buf)

    def gather():
        q8.reduce_requantize(recv, block, w, out=reduced)
        fut = pg.allgather_into_tensor(gathered, reduced).get_future()
        issued.set_result(None)
        _then(fut, done, finish)

    def exchange():
        _then(pg.alltoall_base(recv, send).get_future(), done, gather)

    _issue_in_order(state, issued, done, exchange)
    return done
