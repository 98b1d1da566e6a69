"""The CPU fallbacks of ``ops.powersgd`` against fp64 (the bounds of ``_psgd_refs``), the fused PowerSGD hook
on the CPU backend, and the argument errors."""
import pytest
import torch

import _psgd_refs as R
from _dist_utils import run_ranks
from distributeddataparallel_amd.ops import powersgd as psgd


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rank", [3, 32])
def test_cpu_ops(rank, dtype):
    R.run_step("cpu", R.SHAPES, rank, dtype, offset=1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_hook(dtype):
    run_ranks(R.hook_worker, world=2, backend="cpu", args=("cpu", dtype))


def test_argument_errors():
    g, e = torch.zeros(8, 6), torch.zeros(48)
    p, q = torch.zeros(8, 2), torch.zeros(6, 2)
    psgd.project([g], [e], [q], [p])
    for bad in (dict(ps=[torch.zeros(8, 33)], qs=[torch.zeros(6, 33)]),  # rank outside 1..32
                dict(mats=[torch.zeros(6, 8).t()]),                        # not contiguous
                dict(ps=[p.double()]), dict(qs=[q.half()]), dict(errors=[e.double()]),  # P, Q, E not fp32
                dict(qs=[torch.zeros(5, 2)]), dict(errors=[torch.zeros(47)]), dict(ps=[p, p])):  # sizes
        args = {"mats": [g], "errors": [e], "ps": [p], "qs": [q], **bad}
        with pytest.raises(ValueError):
            psgd.project(args["mats"], args["errors"], args["qs"], args["ps"])
    with pytest.raises(ValueError):
        psgd.orthonormalize([torch.zeros(40, 33)])
