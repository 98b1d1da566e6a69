"""Depthwise convolution on the GPU (dwconv.hip via ops/dwconv.py) against F.conv2d(groups=C) and
its autograd in fp64 on the CPU: bitwise on small-integer inputs (every fp32 partial sum is an
integer below 2^24, so any summation order is exact: every tap, pixel, halo zero, tile and slab
edge and the slot fold), within the fp32-accumulation bound on real values, repeatable, and
capturable in a HIP graph.
"""
import pytest
import torch
import torch.nn.functional as F

import _row_refs as R

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from distributeddataparallel_amd.ops.dwconv import depthwise_conv2d, dwconv_supported  # noqa: E402

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
SHAPES = [(1, 8, 1, 1), (2, 8, 3, 2), (2, 40, 7, 9), (3, 72, 14, 14), (2, 104, 9, 5), (2, 16, 35, 67)]
CASES = [(s, k, b, BF16) for s in SHAPES for k in (3, 5, 7) for b in (False, True)]
CASES += [(s, 7, True, dt) for s in ((2, 40, 7, 9), (2, 16, 35, 67)) for dt in (F16, F32)]


def ids(v):
    return NAME.get(v, "x".join(map(str, v)) if isinstance(v, tuple) else str(v))


def make(shape, k, bias, dtype, integers, seed=0):
    """x, w, bias (or None), dy on the CPU, already rounded to dtype."""
    gen = torch.Generator().manual_seed(seed)
    C = shape[1]
    if integers:
        draw = lambda size, m: torch.randint(-m, m + 1, size, generator=gen).to(dtype)  # noqa: E731
        return draw(shape, 4), draw((C, 1, k, k), 3), draw((C,), 3) if bias else None, draw(shape, 4)
    draw = lambda size: torch.randn(size, generator=gen).to(dtype)  # noqa: E731
    return draw(shape), draw((C, 1, k, k)), draw((C,)) if bias else None, draw(shape)


def reference(x, w, b, dy):
    """fp64 y, dx, dw, db of F.conv2d(groups=C)."""
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    b64 = None if b is None else b.double().requires_grad_()
    y = F.conv2d(x64, w64, b64, padding=w.shape[2] // 2, groups=x.shape[1])
    y.backward(dy.double())
    return y.detach(), x64.grad, w64.grad, None if b is None else b64.grad


def run(x, w, b, dy, as_view=False):
    """The op on the GPU; returns y, dx, dw, db."""
    if as_view:  # as models/convnext.py passes it: an NHWC tensor permuted back
        xg = x.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2).requires_grad_()
    else:
        xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    wg = w.to(DEV).requires_grad_()
    bg = None if b is None else b.to(DEV).requires_grad_()
    assert dwconv_supported(xg, wg), "the call would fall back to F.conv2d"
    y = depthwise_conv2d(xg, wg, bg)
    y.backward(dy.to(DEV).contiguous(memory_format=torch.channels_last))
    return y.detach(), xg.grad, wg.grad, None if bg is None else bg.grad


@pytest.mark.parametrize("shape,k,bias,dtype", CASES + [((3, 72, 14, 14), 7, True, "view")], ids=ids)
def test_dwconv_exact_on_integers(shape, k, bias, dtype):
    view = dtype == "view"
    dtype = BF16 if view else dtype
    x, w, b, dy = make(shape, k, bias, dtype, integers=True)
    got = run(x, w, b, dy, as_view=view)
    for name, g, r in zip(("y", "dx", "dw", "db"), got, reference(x, w, b, dy)):
        if r is not None:
            assert g.dtype == dtype and g.shape == r.shape
            assert torch.equal(g.cpu(), r.to(dtype)), f"{name} differs from the fp64 reference"


@pytest.mark.parametrize("shape,k,bias,dtype", CASES, ids=ids)
def test_dwconv_real_values_within_the_fp32_bound(shape, k, bias, dtype):
    x, w, b, dy = make(shape, k, bias, dtype, integers=False)
    got = run(x, w, b, dy)
    ref = reference(x, w, b, dy)
    scale = reference(x.abs(), w.abs(), None if b is None else b.abs(), dy.abs())  # the same sums of absolute values
    B, _, H, W = shape
    for name, g, r, s, c in zip(("y", "dx", "dw", "db"), got, ref, scale, (k * k + 1, k * k + 1, B * H * W, B * H * W)):
        if r is not None:
            R.check(f"{name}", g.cpu(), r, R.U[dtype] * r.abs() + c * R.EPS32 * s)


def test_dwconv_backward_is_repeatable_and_captures():
    x, w, b, dy = make((3, 72, 14, 14), 7, True, BF16, integers=False, seed=1)
    first, second = run(x, w, b, dy), run(x, w, b, dy)
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    wg, bg = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    dyg = dy.to(DEV).contiguous(memory_format=torch.channels_last)

    def step():
        y = depthwise_conv2d(xg, wg, bg)
        return (y,) + torch.autograd.grad(y, (xg, wg, bg), dyg)

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
