"""The torch path of ops.onebit under the checks of the HIP kernels (tests/_onebit_ref.py), and the
onebit hook on CPU tensors, where its steps run in the callbacks of the collectives' futures."""
import types

import pytest
import torch

import _onebit_ref as ref
from _dist_utils import run_ranks


@pytest.mark.parametrize("n", [1, 513, 7 * 512 + 9])
def test_cpu_path(n):
    for dtype, segments in [(torch.float32, 1), (torch.bfloat16, 3)]:
        ref.run_compress("cpu", dtype, n, 512, segments)
    ref.run_error_feedback("cpu")


@pytest.mark.parametrize("world", [2, 3])
def test_cpu_decode_and_reduce(world):
    for mode in ("mean", "concat"):
        ref.run_decode_mean("cpu", world, mode, torch.float32, 7 * 512 + 9)
        ref.run_decode_mean("cpu", world, mode, torch.bfloat16, 7 * 512 + 9)
    ref.run_reduce_recompress("cpu", world)


@pytest.mark.parametrize("algorithm", ["twoshot", "allgather"])
def test_onebit_hook_two_ranks_cpu(algorithm):
    run_ranks(ref.hook_worker, world=2, backend="cpu", args=("cpu", algorithm, torch.float32))


def test_state_and_backend_errors():
    from distributeddataparallel_amd.ops import onebit
    from distributeddataparallel_amd.parallel.comm_hooks import OneBitState, onebit_allreduce_hook

    assert onebit.payload_bytes(70003, 1024, 8) == 8 * 9 * 132
    with pytest.raises(ValueError, match="block"):
        OneBitState(block=256)
    with pytest.raises(ValueError, match="algorithm"):
        OneBitState(algorithm="ring")
    peer = types.SimpleNamespace(size=lambda: 2, backend="peer")
    with pytest.raises(RuntimeError, match='algorithm="allgather"'):
        onebit_allreduce_hook(OneBitState(process_group=peer), None)
