"""The onebit HIP kernels (csrc/kernels/onebit_comm.hip) against the wire's rules in plain torch.

Checks (tests/_onebit_ref.py): sign bytes bitwise the packing of (x.float() + e) < 0, padding zero;
the stored scale within relative (c + 1) 2^-24 of the fp64 sum |v| / c (the worst case of any fp32
summation order plus the division); err bitwise fp32(v - d) with d from the stored scale; NaN / inf
blocks store scale = NaN, keep their err and leave their neighbours finite; decoded means bitwise the
fp32 accumulation in segment order, one division, one rounding to the output dtype."""
import pytest
import torch

import _onebit_ref as ref
from distributeddataparallel_amd.ops import onebit

pytestmark = pytest.mark.gpu

N_BIG = 70003  # 137 blocks of 512, 35 of 2048: several workgroups, a short tail, every special block


@pytest.mark.parametrize("segments", [1, 3])
@pytest.mark.parametrize("block", [512, 1024, 2048])
@pytest.mark.parametrize("n", [(0, 1), (1, -1), (1, 0), (1, 1), (4, 8), (0, N_BIG)], ids=lambda t: f"{t[0]}G{t[1]:+d}")
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_compress(dtype, n, block, segments):
    ref.run_compress("cuda", dtype, n[0] * block + n[1], block, segments)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_compress_misaligned_view(dtype):
    """Views one element into their storage: no 16-byte accesses, same checks."""
    ref.run_compress("cuda", dtype, N_BIG, 1024, 1, offset=1)


@pytest.mark.parametrize("block", [512, 1024, 2048])
def test_compress_does_not_depend_on_the_grid_position(block):
    """The same blocks compressed alone and behind 5 more blocks: bitwise the same payload rows."""
    n = 4 * block + 8
    x = ref.make_input(n, torch.float32, block, seed=1)
    e = ref.make_err(x, block, seed=1)
    lead = torch.randn(5 * block)
    alone = onebit.compress(x.cuda(), e.cuda(), block, 1)
    behind = onebit.compress(torch.cat([lead, x]).cuda(), torch.cat([lead, e]).cuda(), block, 1)
    (pa, sa), (pb, sb) = ref.unpack(alone, block, 1), ref.unpack(behind, block, 1)
    assert torch.equal(pa, pb[5:]) and torch.equal(sa.view(torch.int32), sb[5:].view(torch.int32))


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["mean", "concat"])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_decode_mean(world, mode, out_dtype):
    ref.run_decode_mean("cuda", world, mode, out_dtype, N_BIG)


@pytest.mark.parametrize("block", [512, 2048])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_reduce_recompress(world, block):
    ref.run_reduce_recompress("cuda", world, block)


def test_error_feedback_telescopes():
    ref.run_error_feedback("cuda")


def test_payload_length_is_checked_before_launch():
    from distributeddataparallel_amd._native import load

    short = torch.empty(128, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="payload must hold 132 bytes"):
        load().onebit_compress(torch.zeros(1000, device="cuda"), torch.zeros(1000, device="cuda"), short, 1024, 1)
