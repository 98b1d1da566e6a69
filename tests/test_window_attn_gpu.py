"""Window attention on the GPU (window_attn.hip via ops/window_attention.py) against an fp64 CPU
reference with true -inf masking and autograd, taken from the bf16-rounded inputs.

Bounds (derived, not tuned): each result may differ from the reference by U[bf16] |ref| + 2^-8 A,
where A is the same formula on absolute values with the true P (``reference(absolute=True)``).
2^-8 is twice the round-to-nearest error of the one bf16 rounding each in-kernel MFMA operand (P,
dS) gets; the spare half covers fp32 accumulation over at most 64 terms and the exp. dbias is a
fixed-order fp32 sum of fp32 terms: U[bias dtype] |ref| + 64 2^-24 sum_w |dS|.
"""
import pytest
import torch

import _row_refs as R
from _window_attn_ref import make, reference

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from distributeddataparallel_amd.ops.window_attention import window_attention, window_attention_supported  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
# Bw, N, H, nW (0: no labels), bias dtype
CASES = [
    (1, 49, 1, 0, BF16),   # one window
    (8, 49, 3, 4, BF16),   # Swin shape with labels
    (6, 64, 2, 3, F32),    # no padding at all
    (5, 33, 2, 0, F32),    # just past one 32-row tile
    (3, 16, 1, 3, BF16),   # small window
    (2, 1, 1, 0, None),    # one token
    (67, 49, 3, 0, BF16),  # several chunks; neither the chunk size nor the waves per workgroup divides it
    (4, 49, 2, 2, None),   # labels without bias
]


def run(qkv, bias, labels, d_out, scale):
    """The op on the GPU; returns o, dqkv, dbias."""
    x = qkv.to(DEV).requires_grad_()
    b = None if bias is None else bias.to(DEV).requires_grad_()
    lab = None if labels is None else labels.to(DEV)
    assert window_attention_supported(x, b, lab), "the call would fall back to eager torch"
    o = window_attention(x, b, lab, scale)
    o.backward(d_out.to(DEV))
    return o.detach(), x.grad, None if b is None else b.grad


@pytest.mark.parametrize("Bw,N,H,nW,bias_dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_window_attention_within_the_derived_bounds(Bw, N, H, nW, bias_dtype):
    args = make(Bw, N, H, nW, bias_dtype)
    o, dqkv, dbias = run(*args)
    ro, rdqkv, rdbias, ds_abs = reference(*args)
    ao, adqkv, _, _ = reference(*args, absolute=True)
    assert o.dtype == BF16 and tuple(o.shape) == (Bw, N, H, 32)
    assert dqkv.dtype == BF16 and tuple(dqkv.shape) == (Bw, N, 3, H, 32)
    R.check("o", o.cpu(), ro, R.U[BF16] * ro.abs() + 2.0 ** -8 * ao)
    for c, name in enumerate(("dq", "dk", "dv")):
        R.check(name, dqkv[:, :, c].cpu(), rdqkv[:, :, c], R.U[BF16] * rdqkv[:, :, c].abs() + 2.0 ** -8 * adqkv[:, :, c])
    if bias_dtype is None:
        assert dbias is None
    else:
        assert dbias.dtype == bias_dtype and tuple(dbias.shape) == (H, N, N)
        R.check("dbias", dbias.cpu(), rdbias, R.U[bias_dtype] * rdbias.abs() + 64 * R.EPS32 * ds_abs)


def test_window_attention_is_repeatable_captures_and_takes_a_linear_view():
    qkv, bias, labels, d_out, scale = make(8, 49, 3, 4, BF16, seed=1)
    first, second = run(qkv, bias, labels, d_out, scale), run(qkv, bias, labels, d_out, scale)
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    x, b = qkv.to(DEV).requires_grad_(), bias.to(DEV).requires_grad_()
    lab, g = labels.to(DEV), d_out.to(DEV)

    def step():
        o = window_attention(x, b, lab, scale)
        return (o,) + torch.autograd.grad(o, (x, b), g)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = step()
    for _ in range(3):
        for t in out:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(out, first):
            assert torch.equal(u.detach(), v), "a replay differs from the eager result"

    # qkv as the view of a real nn.Linear output against a contiguous copy of it
    lin = torch.nn.Linear(96, 288).to(DEV, BF16)
    y = lin(torch.randn(8, 49, 96, device=DEV, dtype=BF16))
    view = y.view(8, 49, 3, 3, 32)
    copy = view.detach().clone().requires_grad_()
    assert window_attention_supported(view, b, lab)
    ov, oc = window_attention(view, b, lab, scale), window_attention(copy, b, lab, scale)
    gv, gc = torch.autograd.grad(ov, y, g)[0], torch.autograd.grad(oc, copy, g)[0]
    assert torch.equal(ov, oc) and torch.equal(gv.view_as(gc), gc)
