"""The topk HIP kernels (csrc/kernels/topk_comm.hip) against the wire's rules in plain torch.

Checks (tests/_topk_ref.py), all bitwise: the slots are the k real elements of largest |v| bits, ties
to the lower index, in ascending index order, with v itself as the value; empty slots are 0xFFFF / 0,
skipped (NaN / inf) blocks 0xFFFF / NaN in every slot; err is 0 on selected elements, v on the
others, and unchanged on skipped blocks and padding; the kernel's payload is the CPU path's; decoded
means are the fp32 accumulation in segment order, one division, one rounding to the output dtype.
decoded + e_new is compared with v + 0.0, not v: a sum of zeros of which one is +0 is +0, so an
element v = -0 comes back as +0 (selected: -0 + 0; not selected: 0 + -0)."""
import pytest
import torch

import _topk_ref as ref
from distributeddataparallel_amd.ops import topk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("segments", [1, 3])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", ["1", "k-1", "G-1", "G", "G+1", "3G+17"])
@pytest.mark.parametrize("block,k", ref.CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_compress(dtype, block, k, n, offset, segments):
    n = {"1": 1, "k-1": k - 1, "G-1": block - 1, "G": block, "G+1": block + 1, "3G+17": 3 * block + 17}[n]
    for variant in (0, 1):  # 0: ties at the k-th magnitude, a repeated value, a NaN; 1: zeros with a -0, +inf
        ref.run_compress("cuda", dtype, block, k, n, segments, offset, variant)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["mean", "concat"])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("block,k", ref.CASES)
def test_decode_mean(block, k, world, mode, out_dtype):
    ref.run_decode_mean("cuda", world, mode, out_dtype, block, k)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("block,k", ref.CASES)
def test_reduce_reselect(block, k, world):
    ref.run_reduce_reselect("cuda", world, block, k)


def test_payload_length_is_checked_before_launch():
    from distributeddataparallel_amd._native import load

    short = torch.empty(128, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="payload must hold 192 bytes"):
        load().topk_compress(torch.zeros(1000, device="cuda"), torch.zeros(1000, device="cuda"), short, 2048, 32, 1)
    with pytest.raises(RuntimeError, match="k must be"):
        load().topk_compress(torch.zeros(1000, device="cuda"), torch.zeros(1000, device="cuda"), short, 2048, 24, 1)
