"""The topk all-reduce hook on device tensors: two ranks share cuda:0 over the CPU backend (RCCL
refuses two ranks on one device), so the HIP kernels run on both sides of real collectives. Every
rank takes the same shard every iteration and no optimizer steps, so the gradient g_r is constant.

Iteration 0 is the warm-up: within one ulp of the dtype of the exact fp64 mean over the shards.
Iterations 1..T, T = 4, at block 1024 and k = 64: bitwise equal gradients on both ranks, and since
the decoded values telescope (sum_t d_t = T v - e_T on every worker, and again on the chunk's
owner), per element

    |mean_t out_t - exact| <= (mean_r max|e_worker,r| + max|e_server|) / T
                              + ulp(dtype, max_t |out_t|) + T 2^-22 max|v|,

the residual maxima taken over all buckets (the server's also over the ranks; 0 for allgather), the
ulp for the output rounding that is not fed back, the last term for two fp32 roundings a round with
max|v| <= max|g| + max|e_worker| + max|out| + max|e_server|. That the running mean beats the first
compressed step is not implied for top-k at this density and is not asserted."""
import pytest
import torch

from _dist_utils import run_ranks
from _topk_ref import hook_worker

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("algorithm", ["twoshot", "allgather"])
def test_topk_hook_two_ranks_one_gpu(algorithm, dtype):
    run_ranks(hook_worker, world=2, backend="cpu", args=("cuda", algorithm, dtype))
