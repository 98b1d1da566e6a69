"""gemm_fp8_nt (csrc/kernels/gemm_fp8.hip): operand layout with exact integer data, accuracy on
quantized random data, the residual / out= epilogues and the host-side shape checks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = (torch.float8_e4m3fn, torch.float8_e5m2)


def _C():
    from distributeddataparallel_amd._native import load

    return load()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _one():
    return torch.ones(1, dtype=torch.float32, device="cuda")


def _tern(R, C, fmt, seed):
    """Entries from {-1, 0, 1} (exact in both formats) as FP8 bytes, and their fp32 values."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-1, 2, (R, C), generator=g).float()
    q = v.to(DT[fmt]).view(torch.uint8)
    assert torch.equal(q.view(DT[fmt]).float(), v)
    return q.cuda(), v.cuda()


@pytest.mark.parametrize("K", [128, 256, 384])
@pytest.mark.parametrize("N", [128, 256, 384])
def test_exact_integer_products(K, N):
    """The layout test: ternary operands, unit scales — every sum is an integer of magnitude
    <= 256, exact in fp32 and in bf16, so the output equals the fp32 reference bitwise. Covers odd
    and even K-tile counts, M tails, more than one tile in M and N, and all four format pairs
    (these grids all run the 256 x 128 tile; the 256 x 256 one has its own test below)."""
    C_ = _C()
    one = _one()
    for af in (0, 1):
        for bf in (0, 1):
            b, bv = _tern(N, K, bf, seed=100003 + K + N + bf)  # (never a's seed: no correlated rows)
            for M in (1, 100, 256, 300):
                a, av = _tern(M, K, af, seed=M + K + 7 * af)
                ref = av @ bv.t()
                assert ref.abs().max().item() <= 256
                y = C_.gemm_fp8_nt(a, b, one, one, af, bf)
                assert y.dtype == torch.bfloat16 and y.shape == (M, N)
                assert torch.equal(y.float(), ref), (M, N, K, af, bf)


def test_exact_wide_tile():
    """A grid where the 256 x 256 tile is chosen (N = 1024, 33 m-tiles: 132 wide tiles fill one
    round of the CUs where 264 narrow ones need two), with an M tail and an odd K-tile count."""
    C_ = _C()
    one = _one()
    M, N, K = 33 * 256 - 37, 1024, 384
    a, av = _tern(M, K, 1, seed=5)
    b, bv = _tern(N, K, 0, seed=6)
    ref = av @ bv.t()
    assert ref.abs().max().item() <= 256
    y = C_.gemm_fp8_nt(a, b, one, one, 1, 0)
    assert torch.equal(y.float(), ref)


@pytest.mark.parametrize("M,K,N", [(300, 384, 384), (513, 1024, 1024)])
@pytest.mark.parametrize("af,bf", [(0, 0), (1, 0)])
def test_random_quantized(M, K, N, af, bf):
    """N(0,1) data quantized by fp8_quantize (non-trivial scales) against the fp32 product of the
    dequantized bytes; 5e-3 is the project's bf16-output GEMM bound (tests/test_gemm_gpu.py)."""
    C_ = _C()
    g = torch.Generator().manual_seed(M + K)
    x = (3.0 * torch.randn(M - M % 16 + 16, K, generator=g)).to(torch.bfloat16).cuda()
    w = (0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16).cuda()
    a, _, sa = C_.fp8_quantize(x, C_.fp8_amax(x), af, False)
    b, _, sb = C_.fp8_quantize(w, C_.fp8_amax(w), bf, False)
    a = a[:M].contiguous()
    assert abs(sa.item() - 1) > 0.1 and abs(sb.item() - 1) > 0.1
    ref = (a.view(DT[af]).float() @ b.view(DT[bf]).float().t()) / (sa * sb)
    y = C_.gemm_fp8_nt(a, b, sa, sb, af, bf)
    r = _rel(y, ref)
    print(f"gemm_fp8_nt ({M},{K},{N}) fmt ({af},{bf}): rel {r:.2e}")
    assert r < 5e-3


def test_residual_and_out_epilogues():
    C_ = _C()
    one = _one()
    M, N, K = 300, 256, 256
    a, av = _tern(M, K, 1, seed=1)
    b, bv = _tern(N, K, 0, seed=2)
    prod = (av @ bv.t()).to(torch.bfloat16)
    res = torch.randn(M, N, device="cuda").to(torch.bfloat16)
    want = (res.float() + prod.float()).to(torch.bfloat16)
    # residual in a separate tensor
    y = C_.gemm_fp8_nt(a, b, one, one, 1, 0, 1, res)
    assert torch.equal(y, want)
    # residual aliasing out: the in-place accumulate
    acc = res.clone()
    r = C_.gemm_fp8_nt(a, b, one, one, 1, 0, 1, acc, acc)
    assert r.data_ptr() == acc.data_ptr() and torch.equal(acc, want)
    # out = a row slice of a larger buffer: the neighbours stay as they were
    big = torch.full((M + 16, N), 7.0, dtype=torch.bfloat16, device="cuda")
    C_.gemm_fp8_nt(a, b, one, one, 1, 0, 0, None, big[8:8 + M])
    assert torch.equal(big[8:8 + M], prod)
    assert (big[:8] == 7).all().item() and (big[8 + M:] == 7).all().item()


def test_rejects_name_the_dimension():
    C_ = _C()
    one = _one()
    z = lambda r, c: torch.zeros(r, c, dtype=torch.uint8, device="cuda")  # noqa: E731
    with pytest.raises(RuntimeError, match=r"K must be .* K = 192"):
        C_.gemm_fp8_nt(z(16, 192), z(128, 192), one, one, 0, 0)
    with pytest.raises(RuntimeError, match=r"N must be .* N = 64"):
        C_.gemm_fp8_nt(z(16, 128), z(64, 128), one, one, 0, 0)
