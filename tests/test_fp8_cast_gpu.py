"""fp8_amax / fp8_quantize (csrc/kernels/fp8_cast.hip) against torch's own FP8 casts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FMAX = (448.0, 57344.0)
DT = (torch.float8_e4m3fn, torch.float8_e5m2)
SHAPES = [(16, 16), (48, 80), (256, 384), (16000, 16)]


def _C():
    from distributeddataparallel_amd._native import load

    return load()


def _x(R, C, seed=0):
    g = torch.Generator().manual_seed(seed + R * 31 + C)
    # a wide range of magnitudes: FP8 subnormals, normals and the saturating maximum all occur
    x = torch.randn(R, C, generator=g) * torch.exp(2 * torch.randn(R, C, generator=g))
    return x.to(torch.bfloat16).cuda()


def _expect(x, scale, fmt):
    return (x.float().cpu() * scale.cpu()).clamp(-FMAX[fmt], FMAX[fmt]).to(DT[fmt]).view(torch.uint8)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("R,C", SHAPES)
def test_quantize_matches_torch_cast(R, C, fmt):
    C_ = _C()
    x = _x(R, C)
    amax = C_.fp8_amax(x)
    assert amax.dtype == torch.float32 and amax.shape == (1,)
    assert amax.item() == x.abs().max().float().item()
    q, qT, scale = C_.fp8_quantize(x, amax, fmt, True)
    assert abs(scale.item() * amax.item() / FMAX[fmt] - 1) < 1e-6
    assert q.dtype == torch.uint8 and q.shape == (R, C) and qT.shape == (C, R)
    assert torch.equal(q.cpu(), _expect(x, scale, fmt))
    assert torch.equal(qT, q.t().contiguous())
    # the element that holds amax saturates to +-FMAX exactly
    v = q.view(DT[fmt]).float().abs().max().item()
    assert v == FMAX[fmt]
    q2, none, scale2 = C_.fp8_quantize(x, amax, fmt, False)
    assert none is None and torch.equal(q2, q) and torch.equal(scale2, scale)


@pytest.mark.parametrize("fmt", [0, 1])
def test_zero_tensor(fmt):
    C_ = _C()
    x = torch.zeros(48, 80, dtype=torch.bfloat16, device="cuda")
    amax = C_.fp8_amax(x)
    q, qT, scale = C_.fp8_quantize(x, amax, fmt, True)
    assert amax.item() == 0.0 and scale.item() == 1.0
    assert not q.any().item() and not qT.any().item()


def test_rejects_shapes_off_the_16_grid():
    C_ = _C()
    x = torch.ones(10, 16, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="multiples of 16"):
        C_.fp8_quantize(x, C_.fp8_amax(x), 0, True)


def test_graph_capture_replays_the_eager_bytes():
    """No call syncs the host: amax + quantize capture into a graph (one stream, no parallel
    branches) and one replay on new input reproduces the eager bytes."""
    C_ = _C()
    x = _x(256, 384, seed=1)
    buf = torch.zeros_like(x)
    C_.fp8_quantize(buf, C_.fp8_amax(buf), 0, True)  # (kernels loaded before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        q, qT, scale = C_.fp8_quantize(buf, C_.fp8_amax(buf), 0, True)
    buf.copy_(x)
    g.replay()
    torch.cuda.synchronize()
    eq, eqT, escale = C_.fp8_quantize(x, C_.fp8_amax(x), 0, True)
    assert torch.equal(scale, escale) and torch.equal(q, eq) and torch.equal(qT, eqT)
