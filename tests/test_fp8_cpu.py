"""FP8 linear layers, CPU side: ``XDDP_FP8=emulate`` runs the FP8 recipe (per-tensor current
scaling, e4m3 activations / weights, e5m2 output gradients, fp32 accumulation, bf16 results) in
plain torch, so FP8 numerics, the switch and its fall-backs are checked without a GPU."""
import pytest
import torch

from distributeddataparallel_amd.ops import fp8 as F8
from distributeddataparallel_amd.ops.linear import linear, multi_linear


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _data(M, K, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    dy = torch.randn(M, N, generator=g).to(torch.bfloat16)
    return x, w, dy


def _run(x, w, dy, **kw):
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    y = linear(x, w, **kw)
    y.backward(dy)
    return y.detach(), x.grad, w.grad


@pytest.mark.parametrize("M,K,N", [(128, 128, 128), (256, 512, 384)])
def test_emulated_linear_vs_fp32(monkeypatch, M, K, N):
    """Relative Frobenius error of the emulated FP8 linear against fp32 matmuls of the same bf16
    inputs (N(0,1) inputs and gradients, N(0,1/K) weights): ~0.0375 for Y (two e4m3 operands),
    ~0.059 for dX and dW (one e5m2 operand). The bounds are those figures + 20 % for seed
    variation; the lower bound fails if quantization is silently off."""
    monkeypatch.setenv("XDDP_FP8", "emulate")
    x, w, dy = _data(M, K, N)
    y, dx, dw = _run(x, w, dy)
    xf, wf, df = x.float(), w.float(), dy.float()
    ey, edx, edw = _rel(y, xf @ wf.t()), _rel(dx, df @ wf), _rel(dw, df.t() @ xf)
    print(f"emulated fp8 linear ({M},{K},{N}): rel err Y {ey:.4f} dX {edx:.4f} dW {edw:.4f}")
    assert y.dtype == dx.dtype == dw.dtype == torch.bfloat16
    assert 0.01 < ey < 0.045
    assert 0.01 < edx < 0.07
    assert 0.01 < edw < 0.07


def test_emulated_multi_linear_and_residual(monkeypatch):
    """multi_linear quantizes x once and accumulates dX over the weights; linear's residual is
    added to the FP8 product: both agree with the per-weight emulated linears."""
    monkeypatch.setenv("XDDP_FP8", "emulate")
    x, w1, dy1 = _data(128, 256, 128, seed=1)
    _, w2, dy2 = _data(128, 256, 384, seed=2)
    xa = x.clone().requires_grad_(True)
    wa, wb = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    ya, yb = multi_linear(xa, wa, wb)
    torch.autograd.backward([ya, yb], [dy1, dy2])
    y1, dx1, dw1 = _run(x, w1, dy1)
    y2, dx2, dw2 = _run(x, w2, dy2)
    assert torch.equal(ya, y1) and torch.equal(yb, y2)
    assert torch.equal(wa.grad, dw1) and torch.equal(wb.grad, dw2)
    assert _rel(xa.grad, dx1.float() + dx2.float()) < 5e-3  # one extra bf16 rounding of the sum
    res = torch.randn(128, 128).to(torch.bfloat16).requires_grad_(True)
    yr = linear(x, w1, res)
    assert torch.equal(yr, (res.float() + y1.float()).to(torch.bfloat16))
    yr.backward(dy1)
    assert torch.equal(res.grad, dy1)


@pytest.mark.parametrize("M,K", [(128, 192), (100, 128)])
def test_fallback_is_bitwise_the_plain_path(monkeypatch, M, K):
    """K = 192 (not a multiple of 128) and tokens = 100 cannot take the FP8 path: the call falls
    back silently and equals the XDDP_FP8=0 result bit for bit."""
    x, w, dy = _data(M, K, 128)
    monkeypatch.setenv("XDDP_FP8", "0")
    ref = _run(x, w, dy)
    monkeypatch.setenv("XDDP_FP8", "emulate")
    got = _run(x, w, dy)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    ym = multi_linear(x, w, w)
    assert torch.equal(ym[0], ref[0]) and torch.equal(ym[1], ref[0])


def test_fp8_false_overrides_env(monkeypatch):
    """The LM head's ``fp8=False`` keeps the call in bf16 under XDDP_FP8; an eligible call without
    it does change (so the comparison is not vacuous)."""
    x, w, dy = _data(128, 128, 256)
    monkeypatch.setenv("XDDP_FP8", "0")
    ref = _run(x, w, dy)
    monkeypatch.setenv("XDDP_FP8", "emulate")
    off = _run(x, w, dy, fp8=False)
    on = _run(x, w, dy)
    for a, b in zip(off, ref):
        assert torch.equal(a, b)
    assert not torch.equal(on[0], ref[0])


@pytest.mark.parametrize("fmt", [F8.E4M3, F8.E5M2])
def test_saturation(fmt):
    """A tensor's own amax quantizes to ±FMAX exactly, not NaN (torch's cast of 500.0 to
    float8_e4m3fn is NaN: the emulation clamps first); zero input gives scale 1 and zero bytes."""
    dt = (torch.float8_e4m3fn, torch.float8_e5m2)[fmt]
    x = torch.randn(32, 48).to(torch.bfloat16)
    x[3, 5], x[7, 9] = 37.25, -37.25  # ±amax, both signs
    q, qT, scale = F8.quantize_reference(x, fmt)
    v = q.view(dt).float()
    assert torch.isfinite(v).all()
    assert v[3, 5].item() == F8.FMAX[fmt] and v[7, 9].item() == -F8.FMAX[fmt]
    assert abs(scale.item() * 37.25 / F8.FMAX[fmt] - 1) < 1e-6
    assert torch.equal(qT, q.t().contiguous())
    # a value that would overflow the format after scaling rounds up past FMAX without the clamp
    big = torch.tensor([[0.999 * 37.25]], dtype=torch.bfloat16).expand(16, 16).contiguous()
    qb, _, _ = F8.quantize_reference(big, fmt)
    assert torch.isfinite(qb.view(dt).float()).all()
    qz, qzT, sz = F8.quantize_reference(torch.zeros(16, 32, dtype=torch.bfloat16), fmt)
    assert sz.item() == 1.0 and not qz.any() and not qzT.any()
