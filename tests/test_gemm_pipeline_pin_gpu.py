"""Pins the outputs of every kernel built on the shared 4-phase LDS-DMA GEMM pipeline
(csrc/kernels/gemm_pipeline.h: gemm.hip's dense / conv / DGS2 modes and gemm_fp8.hip) to the bits
they had before the pipeline was factored out of the two files.

Every input is built on the CPU from a seeded generator (bf16 by rounding fp32 normals, FP8 bytes by
casting fp32 normals on the CPU, scales 0.5 and 2.0), moved to the device and run through the op;
the SHA-256 of each output tensor's bytes must equal tests/golden/gemm_pipeline_digests.json.
Bit equality holds for any tile width the host picks: the K-accumulation order does not depend on
BN and the epilogue partial sums depend only on the 256-row block tile.

The fixture is written by ``python tests/test_gemm_pipeline_pin_gpu.py --write`` on a build of the
commit whose arithmetic is to be kept. A digest that differs means the arithmetic changed: fix the
kernel, not the fixture."""
import hashlib
import json
import os
import sys
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_pipeline_digests.json")
FP8 = (torch.float8_e4m3fn, torch.float8_e5m2)
WIDE_M = 33 * 256 - 37  # 33 m-tiles x N = 1024: the 256 x 256 tile on 256 CUs, with an M tail

# (M, N, K): single K-tile (zero tile in front) | odd tile count, M tail, three narrow n-tiles |
# even tile count, N % 256 == 0 but the narrow tile | the wide tile
GEMM_SHAPES = [(1, 128, 64), (300, 384, 192), (513, 256, 128), (WIDE_M, 1024, 192)]
# epilogue variants: (name, epi, bias, residual / h, out aliases the residual)
GEMM_EPIS = [("none", 0, False, False, False), ("bias", 1, True, False, False), ("bias_gelu", 2, True, False, False),
             ("res", 3, False, True, False), ("res_bias_inplace", 3, True, True, True),
             ("dgelu", 4, True, True, False), ("stats", 5, False, False, False)]


def _C():
    from distributeddataparallel_amd._native import load

    return load()


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _bf16(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _gemm_nt(name, M, N, K, epi, bias, res, alias):
    g = _gen(name)
    a, w = _bf16(g, M, K).cuda(), _bf16(g, N, K, scale=K ** -0.5).cuda()
    b = _bf16(g, N).cuda() if bias else None
    r = _bf16(g, M, N, scale=2.0).cuda() if res else None
    return _C().gemm_nt(a, w, b, epi, r, r if alias else None)


def _gemm_fp8(name, M, N, K, af, bf, epi=0, alias=False):
    g = _gen(name)
    a = torch.randn(M, K, generator=g).to(FP8[af]).view(torch.uint8).cuda()
    b = torch.randn(N, K, generator=g).to(FP8[bf]).view(torch.uint8).cuda()
    sa, sb = torch.full((1,), 0.5).cuda(), torch.full((1,), 2.0).cuda()
    r = _bf16(g, M, N, scale=2.0).cuda() if epi else None
    return [_C().gemm_fp8_nt(a, b, sa, sb, af, bf, epi, r, r if alias else None)]


def _conv_fwd(name, B, C, H, N, stride, stats):
    g = _gen(name)
    x, w = _cl(_bf16(g, B, C, H, H)).cuda(), _cl(_bf16(g, N, C, 3, 3, scale=(9 * C) ** -0.5)).cuda()
    return _C().conv3x3_forward(x, w, stride, stats)


def _conv_dgrad_s2(name, B, Co, OH, Ci):
    g = _gen(name)
    dy = _cl(_bf16(g, B, Co, OH, OH)).cuda()
    w = _bf16(g, Co, Ci, 3, 3, scale=(9 * Co) ** -0.5)
    wr = _cl(w.flip(2, 3).permute(1, 0, 2, 3)).cuda()  # wr[ci][co][a][b] = w[co][ci][2-a][2-b]
    return [_C().conv3x3_dgrad_s2(dy, wr, 2 * OH, 2 * OH)]


def _cases():
    c = {}
    for M, N, K in GEMM_SHAPES:
        for en, epi, bias, res, alias in GEMM_EPIS:
            n = f"gemm_nt-{M}x{N}x{K}-{en}"
            c[n] = (_gemm_nt, (n, M, N, K, epi, bias, res, alias))
    for M, N, K in [(300, 384, 384), (256, 128, 128)]:
        for af in (0, 1):
            for bf in (0, 1):
                n = f"gemm_fp8-{M}x{N}x{K}-fmt{af}{bf}"
                c[n] = (_gemm_fp8, (n, M, N, K, af, bf))
    n = f"gemm_fp8-{WIDE_M}x1024x384-fmt10"
    c[n] = (_gemm_fp8, (n, WIDE_M, 1024, 384, 1, 0))
    for alias in (False, True):
        n = "gemm_fp8-300x256x256-fmt10-res" + ("_inplace" if alias else "")
        c[n] = (_gemm_fp8, (n, 300, 256, 256, 1, 0, 1, alias))
    # conv3x3_forward shapes that take conv3x3_gemm (stride 2, or stride 1 with W = 7 < the band
    # kernel's 14; N % 128 == 0, C / 64 a power of two), and the even-size DGS2 input gradient
    for stats in (False, True):
        n = "conv3x3-2x64x14x14-n128-s2" + ("-stats" if stats else "")
        c[n] = (_conv_fwd, (n, 2, 64, 14, 128, 2, stats))
    n = "conv3x3-8x128x7x7-n128-s1-stats"
    c[n] = (_conv_fwd, (n, 8, 128, 7, 128, 1, True))
    n = "conv3x3_dgrad_s2-2x64x7x7-cin128"
    c[n] = (_conv_dgrad_s2, (n, 2, 64, 7, 128))
    return c


CASES = _cases()


def _digests(name):
    fn, args = CASES[name]
    outs = fn(*args)
    torch.cuda.synchronize()
    return [hashlib.sha256(t.cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest() for t in outs]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_output_bits_pinned(name, golden):
    assert _digests(name) == golden[name]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_gemm_pipeline_pin_gpu.py --write")
    with open(GOLDEN, "w") as f:
        json.dump({n: _digests(n) for n in CASES}, f, indent=1)
        f.write("\n")
    print(f"wrote {len(CASES)} cases to {GOLDEN}")
