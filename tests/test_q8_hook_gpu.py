"""The q8 all-reduce hook on device tensors: two ranks share cuda:0 over the CPU backend (RCCL
refuses two ranks on one device), so the HIP kernels run on both sides of real collectives.
Bound per gradient element: (R / 255)(1 + 1e-3) plus one ulp of the parameter dtype, R the largest
max - min of any rank's flat gradient (no block's scale exceeds R / 255, neither at the first
quantization nor at the second)."""
import pytest
import torch

from _dist_utils import run_ranks
from _q8_ref import hook_worker

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("algorithm", ["twoshot", "allgather"])
def test_q8_hook_two_ranks_one_gpu(algorithm, dtype):
    run_ranks(hook_worker, world=2, backend="cpu", args=("cuda", algorithm, dtype))
