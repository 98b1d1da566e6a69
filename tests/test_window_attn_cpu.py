"""Window attention off the GPU: the eager fallback against the fp64 reference, Swin-T's parameter
count, the shifted-window labels against the standard 0 / -100 mask, and swin_tiny end to end."""
import pytest
import torch

import _row_refs as R
from _window_attn_ref import make, reference
from distributeddataparallel_amd.models import swin_t, swin_tiny
from distributeddataparallel_amd.models.swin import shift_labels
from distributeddataparallel_amd.ops import window_attention


@pytest.mark.parametrize("Bw,N,H,nW,D", [(6, 49, 3, 3, 32), (2, 20, 2, 0, 24)])
def test_eager_fallback_within_the_fp32_bound(Bw, N, H, nW, D):
    """fp32 inputs, so no storage rounding: every result is a chain of fp32 sums of at most 64 terms,
    bounded by 64 x 2^-24 x the same sums of absolute values. dbias sums dS = P (dP - delta), a
    difference formed in fp32, so its terms' magnitude is G = P (|dP| + |delta|), not |dS|."""
    qkv, bias, labels, d_out, scale = args = make(Bw, N, H, nW, torch.float32, dtype=torch.float32, D=D)
    x, b = qkv.clone().requires_grad_(), bias.clone().requires_grad_()
    o = window_attention(x, b, labels, scale)
    o.backward(d_out)
    ro, rdqkv, rdbias, _ = reference(*args)
    ao, adqkv, _, g_sum = reference(*args, absolute=True)
    assert o.dtype == torch.float32 and tuple(o.shape) == (Bw, N, H, D)
    R.check("o", o.detach(), ro, 64 * R.EPS32 * ao)
    R.check("dqkv", x.grad, rdqkv, 64 * R.EPS32 * adqkv)
    R.check("dbias", b.grad, rdbias, 64 * R.EPS32 * g_sum)


def test_swin_t_parameter_count():
    assert sum(p.numel() for p in swin_t().parameters()) == 28_288_354


def test_shift_labels_reproduce_the_standard_mask():
    H = W = 14
    ws, shift = 7, 3
    img = torch.zeros(H, W)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    win = img.view(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    diff = win[:, None, :] - win[:, :, None]
    mask = torch.zeros_like(diff).masked_fill(diff != 0, -100.0)  # the usual [nW, N, N] table
    lab = shift_labels(H, W, ws, shift)
    assert lab.dtype == torch.int32 and tuple(lab.shape) == (4, 49)
    assert torch.equal(lab[:, :, None] == lab[:, None, :], mask == 0)
    assert (mask != 0).any()


def test_swin_tiny_trains_on_the_cpu():
    torch.manual_seed(0)
    model = swin_tiny(num_classes=10)
    assert model.stages[0][1].labels is not None and model.stages[1][1].labels is None
    x = torch.randn(2, 3, 32, 32).contiguous(memory_format=torch.channels_last)
    loss = torch.nn.functional.cross_entropy(model(x), torch.tensor([1, 7]))
    loss.backward()
    assert torch.isfinite(loss)
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
