"""The torch fallbacks of ops.q8 under the bounds of the HIP kernels (tests/_q8_ref.py), and the q8
hook on CPU tensors, where its steps run in the callbacks of the collectives' futures."""
import types

import pytest
import torch

import _q8_ref as ref
from _dist_utils import run_ranks


@pytest.mark.parametrize("n", [1, 513])
def test_fallbacks(n):
    for dtype, segments in [(torch.float32, 1), (torch.bfloat16, 3)]:
        ref.run_quantize("cpu", dtype, n, 128, segments)
    for mode in ("mean", "concat"):
        ref.run_dequantize_mean("cpu", 3, mode, torch.float32, n, block=128)
        ref.run_dequantize_mean("cpu", 2, mode, torch.bfloat16, n, block=128)
    ref.run_reduce_requantize("cpu", 3, n, block=128)


@pytest.mark.parametrize("algorithm", ["twoshot", "allgather"])
def test_q8_hook_two_ranks_cpu(algorithm):
    run_ranks(ref.hook_worker, world=2, backend="cpu", args=("cpu", algorithm, torch.float32))


def test_state_and_backend_errors():
    from distributeddataparallel_amd.parallel.comm_hooks import Q8State, q8_allreduce_hook

    with pytest.raises(ValueError, match="block"):
        Q8State(block=100)
    with pytest.raises(ValueError, match="algorithm"):
        Q8State(algorithm="ring")
    peer = types.SimpleNamespace(size=lambda: 2, backend="peer")
    with pytest.raises(RuntimeError, match='algorithm="allgather"'):
        q8_allreduce_hook(Q8State(process_group=peer), None)
