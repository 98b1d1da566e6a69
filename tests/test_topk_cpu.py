"""The torch path of ops.topk under the checks of the HIP kernels (tests/_topk_ref.py), the topk hook
on CPU tensors, where its steps run in the callbacks of the collectives' futures, and the argument
errors."""
import types

import pytest
import torch

import _topk_ref as ref
from _dist_utils import run_ranks


@pytest.mark.parametrize("block,k", ref.CASES)
def test_cpu_compress(block, k):
    for n in (1, k - 1, block + 1, 3 * block + 17):
        ref.run_compress("cpu", torch.float32, block, k, n, 1, variant=0)
        ref.run_compress("cpu", torch.bfloat16, block, k, n, 3, offset=1, variant=1)


@pytest.mark.parametrize("world", [2, 3])
def test_cpu_decode_and_reduce(world):
    for mode in ("mean", "concat"):
        ref.run_decode_mean("cpu", world, mode, torch.float32, 1024, 8)
        ref.run_decode_mean("cpu", world, mode, torch.bfloat16, 2048, 32)
    ref.run_reduce_reselect("cpu", world, 1024, 8)


@pytest.mark.parametrize("algorithm", ["twoshot", "allgather"])
def test_topk_hook_two_ranks_cpu(algorithm):
    run_ranks(ref.hook_worker, world=2, backend="cpu", args=("cpu", algorithm, torch.float32))


def test_argument_errors():
    from distributeddataparallel_amd.ops import topk
    from distributeddataparallel_amd.parallel.comm_hooks import TopKState, topk_allreduce_hook

    assert topk.payload_bytes(70003, 2048, 32, 8) == 8 * 5 * 192
    for bad in (dict(block=512), dict(k=24), dict(algorithm="ring"), dict(start_iter=-1)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            TopKState(**bad)
    x, e = torch.zeros(100), torch.zeros(100)
    for call in (lambda: topk.compress(x, e, 512, 8), lambda: topk.compress(x, e, 1024, 7),
                 lambda: topk.compress(x, e[:50], 1024, 8), lambda: topk.payload_bytes(100, 1024, 8, 0),
                 lambda: topk.decode_mean(topk.compress(x, e, 1024, 8), x, 1024, 8, 1, "sum")):
        with pytest.raises(ValueError):
            call()
    peer = types.SimpleNamespace(size=lambda: 2, backend="peer")
    with pytest.raises(RuntimeError, match='algorithm="allgather"'):
        topk_allreduce_hook(TopKState(process_group=peer), None)
