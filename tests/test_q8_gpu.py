"""The q8 HIP kernels (csrc/kernels/q8_comm.hip) against an fp64 reading of their payload.

Bounds (tests/_q8_ref.py): lo and scale bitwise min and (max - min) / 255; decode error at most
scale / 2 (1 + 1e-4) + 4 * 2^-23 max|x_block|; the fp32 mean of W payloads within
2^-22 mean_r(|lo_r| + 255 |scale_r|) of its fp64 value, the bf16 one within one ulp of the rounded
fp64 value; NaN / inf blocks decode to NaN and leave their neighbours alone."""
import pytest
import torch

import _q8_ref as ref

pytestmark = pytest.mark.gpu

N_BIG = 70003  # 137 blocks of 512: several workgroups, a short tail, every special block


@pytest.mark.parametrize("segments", [1, 3])
@pytest.mark.parametrize("block", [128, 512, 1024])
@pytest.mark.parametrize("n", [1, 511, 512, 513, 4 * 512 + 8, N_BIG])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_quantize(dtype, n, block, segments):
    ref.run_quantize("cuda", dtype, n, block, segments)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_misaligned_view(dtype):
    """A view one element into its storage: no 16-byte loads, same result."""
    ref.run_quantize("cuda", dtype, N_BIG, 512, 1, offset=1)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["mean", "concat"])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_dequantize_mean(world, mode, out_dtype):
    ref.run_dequantize_mean("cuda", world, mode, out_dtype, N_BIG)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_reduce_requantize(world):
    ref.run_reduce_requantize("cuda", world, N_BIG)


def test_payload_length_is_checked_before_launch():
    from distributeddataparallel_amd._native import load

    short = torch.empty(1032, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="payload must hold 1040 bytes"):
        load().q8_quantize(torch.zeros(1000, device="cuda"), short, 512, 1)
