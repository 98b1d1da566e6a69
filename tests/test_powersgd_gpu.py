"""The fused PowerSGD kernels (csrc/kernels/powersgd.hip) against fp64, at the shapes where their tiles turn
over (``_psgd_refs.SHAPES``), with unaligned bases, over a launch-table turnover, and under the hook: two
ranks share cuda:0 over the CPU backend, as in test_q8_hook_gpu.py."""
import pytest
import torch

import _psgd_refs as R
from _dist_utils import run_ranks
from distributeddataparallel_amd.ops import powersgd as psgd

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rank", [1, 3, 8, 32])
@pytest.mark.parametrize("shapes,offset", [(R.SHAPES, 0), (R.SHAPES, 1), (R.SMALL, 0)], ids=["edges", "shifted", "41"])
def test_step_against_fp64(shapes, offset, rank, dtype):
    R.run_step("cuda", shapes, rank, dtype, offset=offset)


@pytest.mark.parametrize("rank", [3, 32])
def test_orthonormalize_zero_and_epsilon(rank):
    gen = torch.Generator().manual_seed(rank)
    zero = torch.zeros(300, rank, device="cuda")
    x = R.make_matrix(300, rank, rank, gen).float().contiguous().cuda()
    before = x.clone()
    psgd.orthonormalize([zero, x], epsilon=1e-3)
    assert torch.isfinite(zero).all()
    R.check_ortho(x, before, 1e-3, "epsilon 1e-3")
    psgd.orthonormalize([zero])
    assert torch.isfinite(zero).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_alone_in_a_list_and_twice(dtype):
    lone = R.run_step("cuda", [R.SMALL[40]], 3, dtype, seed=5)
    for _ in range(2):
        many = R.run_step("cuda", [R.SMALL[40]] + R.SMALL[:40], 3, dtype, seed=5)
        for a, b in zip(lone, many):
            assert torch.equal(a[0], b[0])
    wide = [R.run_step("cuda", [(65, 257)] + extra, 8, dtype, seed=6) for extra in ([], R.SMALL)]
    for a, b in zip(*wide):
        assert torch.equal(a[0], b[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_hook_two_ranks_one_gpu(dtype):
    run_ranks(R.hook_worker, world=2, backend="cpu", args=("cuda", dtype))
