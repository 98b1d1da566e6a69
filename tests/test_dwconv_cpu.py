"""ops/dwconv.py and models/convnext.py without a GPU: the CPU path is nn.Conv2d bit for bit, the
path switch, ConvNeXt-T's parameter count and a small model's forward and backward."""
import torch
import torch.nn as nn

from distributeddataparallel_amd.models import ConvNeXt, convnext_tiny
from distributeddataparallel_amd.ops import DepthwiseConv2d
from distributeddataparallel_amd.ops.dwconv import dwconv_supported


def test_depthwise_conv2d_on_cpu_is_nn_conv2d():
    torch.manual_seed(0)
    for k, bias in ((3, False), (7, True)):
        ours, ref = DepthwiseConv2d(16, k, bias=bias), nn.Conv2d(16, 16, k, padding=k // 2, groups=16, bias=bias)
        assert {n: tuple(p.shape) for n, p in ours.state_dict().items()} == \
            {n: tuple(p.shape) for n, p in ref.state_dict().items()}
        ref.load_state_dict(ours.state_dict())
        x = torch.randn(2, 16, 9, 5).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(2, 16, 9, 5)
        grads = []
        for m in (ours, ref):
            xi = x.clone().requires_grad_()
            y = m(xi)
            grads.append((y.detach(),) + torch.autograd.grad(y, (xi, *m.parameters()), dy))
        for u, v in zip(*grads):
            assert torch.equal(u, v)


def test_path_switch(monkeypatch):
    x = torch.zeros(1, 8, 4, 4).contiguous(memory_format=torch.channels_last)
    w = torch.zeros(8, 1, 3, 3)
    assert not dwconv_supported(x, w)  # a CPU tensor
    monkeypatch.setenv("XDDP_DWCONV", "0")
    assert not dwconv_supported(x.to("meta"), w.to("meta"))
    if torch.cuda.is_available():
        assert not dwconv_supported(x.cuda(), w.cuda())
        monkeypatch.setenv("XDDP_DWCONV", "1")
        assert dwconv_supported(x.cuda(), w.cuda())


def test_convnext_tiny_parameter_count():
    with torch.device("meta"):
        model = convnext_tiny()
    # stem 4,896; blocks 8 d^2 + 58 d each; downsamples 74,112 + 295,680 + 1,181,184; head 770,536
    assert sum(p.numel() for p in model.parameters()) == 28_589_128


def test_small_convnext_trains():
    torch.manual_seed(0)
    model = ConvNeXt(depths=(1, 1), dims=(8, 16), num_classes=10)
    x = torch.randn(2, 3, 16, 16).contiguous(memory_format=torch.channels_last)
    out = model(x)
    assert out.shape == (2, 10)
    loss = nn.functional.cross_entropy(out, torch.tensor([1, 7]))
    loss.backward()
    assert torch.isfinite(loss).item()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
