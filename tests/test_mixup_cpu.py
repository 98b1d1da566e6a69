"""data.Mixup and the two-label cross-entropy without a GPU: the host-side plan (determinism, boxes,
the corrected lam, per-sample draws, the identity), the torch form of the mixing rule against an
explicit per-sample loop in both memory formats, and the CPU fallback of ops.cross_entropy for a
MixedTarget against the fp64 reference and bounds of tests/_mix_refs.py."""
import numpy as np
import pytest
import torch

import _mix_refs as M
import _row_refs as R

from distributeddataparallel_amd.data import Mixup, mix_images
from distributeddataparallel_amd.ops import CrossEntropyLoss, MixedTarget
from distributeddataparallel_amd.ops.cross_entropy import cross_entropy

H, W = 32, 24


def draws(mixer, n, B=4):
    return [mixer.draw(B, H, W, "cpu") for _ in range(n)]


def test_draw_is_deterministic_from_the_seed():
    a, b, c = (draws(Mixup(seed=s, mode="elem"), 20) for s in (11, 11, 12))
    for p, q in zip(a, b):
        assert np.array_equal(p.host_lam, q.host_lam) and np.array_equal(p.host_box, q.host_box)
    assert any(not np.array_equal(p.host_lam, q.host_lam) for p, q in zip(a, c))


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_draw_boxes_lie_inside_the_image_and_lam_is_the_kept_share(mode):
    mixer = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, seed=3)
    cut = mix = 0
    for _ in range(200):
        plan = mixer.draw(4, H, W, "cpu")  # (its tensors are the mixer's persistent ones: look before the next draw)
        n = 4 if mode == "elem" else 1
        assert plan.host_lam.shape == (n,) and plan.host_box.shape == (n, 4)
        assert plan.lam.dtype == torch.float32 and plan.box.dtype == torch.int32
        assert np.array_equal(plan.lam.numpy(), plan.host_lam) and np.array_equal(plan.box.numpy(), plan.host_box)
        for lam, (y0, y1, x0, x1) in zip(plan.host_lam, plan.host_box):
            assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W and 0.0 <= lam <= 1.0
            area = int(y1 - y0) * int(x1 - x0)
            if area:
                cut += 1
                assert lam == np.float32(1.0 - area / (H * W))
            else:
                mix += 1
                assert (y0, y1, x0, x1) == (0, 0, 0, 0)
    assert cut > 50 and mix > 50  # switch_prob = 0.5 picks both


def test_draw_elem_gives_independent_draws_per_sample():
    plan = Mixup(mode="elem", seed=5).draw(16, H, W, "cpu")
    assert len(set(plan.host_lam.tolist())) > 8
    assert Mixup(mode="batch", seed=5).draw(16, H, W, "cpu").host_lam.shape == (1,)


def test_draw_rewrites_the_same_tensors():
    """What a captured apply() reads: the plan's tensors stay where they are from draw to draw."""
    mixer = Mixup(mode="elem", seed=5)
    p = mixer.draw(4, H, W, "cpu")
    q = mixer.draw(4, H, W, torch.device("cpu"))
    assert p.lam.data_ptr() == q.lam.data_ptr() and p.box.data_ptr() == q.box.data_ptr()
    assert torch.equal(p.lam, q.lam) and not np.array_equal(p.host_lam, q.host_lam)


def test_draw_prob_0_is_the_identity_plan():
    mixer = Mixup(prob=0.0, mode="elem", seed=1)
    plan = mixer.draw(6, H, W, "cpu")
    assert (plan.host_lam == 1).all() and not plan.host_box.any()
    x = M.make_images((6, 3, 8, 8), torch.bfloat16)
    labels = torch.arange(6)
    out, target = mixer.apply(x, labels)
    assert torch.equal(out, x) and torch.equal(target.a, labels) and torch.equal(target.b, labels.flip(0))


def test_only_one_alpha_picks_that_method():
    assert all(not p.host_box.any() for p in draws(Mixup(mixup_alpha=0.8, cutmix_alpha=0.0, seed=2), 30))
    plans = draws(Mixup(mixup_alpha=0.0, cutmix_alpha=1.0, seed=2), 30)
    assert all(p.host_box.any() or p.host_lam[0] == 1 for p in plans) and any(p.host_box.any() for p in plans)
    with pytest.raises(ValueError):
        Mixup(mixup_alpha=0.0, cutmix_alpha=0.0)
    with pytest.raises(ValueError):
        Mixup(mode="pair")


def loop_mix(x, partner, lam, box):
    """The rule, one sample and one pixel row at a time."""
    B = x.shape[0]
    out = torch.empty_like(x)
    for i in range(B):
        j = B - 1 - i if partner is None else int(partner[i])
        w = lam[i if lam.numel() > 1 else 0]
        y0, y1, x0, x1 = (int(v) for v in box[i if box.shape[0] > 1 else 0])
        if y1 > y0 and x1 > x0:
            out[i] = x[i]
            out[i, :, y0:y1, x0:x1] = x[j, :, y0:y1, x0:x1]
        elif w == 1:
            out[i] = x[i]
        elif w == 0:
            out[i] = x[j]
        else:
            out[i] = (w * x[i].float() + (1 - w) * x[j].float()).to(x.dtype)
    return out


@pytest.mark.parametrize("fmt", [torch.contiguous_format, torch.channels_last], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cpu_apply_equals_a_per_sample_loop(dtype, fmt):
    B = 5
    x = M.make_images((B, 3, 9, 11), dtype).contiguous(memory_format=fmt)
    x[4, 0, 0, 0] = float("nan")  # sample 0's partner; must not leak under a zero weight
    lam = torch.tensor([1.0, 0.3, 0.0, 0.7, 0.25])
    box = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [2, 7, 3, 11], [0, 9, 0, 11]], dtype=torch.int32)
    for partner in (None, torch.tensor([1, 2, 3, 4, 0], dtype=torch.int32)):
        for lm, bx in ((lam, box), (lam[1:2], box[3:4]), (lam[1:2], box[:1])):
            before = x.clone()
            out = mix_images(x, partner, lm, bx)
            assert out.stride() == x.stride() and out.dtype == x.dtype
            assert torch.equal(out.nan_to_num(nan=7.0), loop_mix(x, partner, lm, bx).nan_to_num(nan=7.0))
            assert torch.equal(x.nan_to_num(nan=7.0), before.nan_to_num(nan=7.0))
    out = mix_images(x, None, lam, box)
    assert not torch.isnan(out[0]).any() and torch.equal(out[2], x[2])  # lam = 1 keeps x[0]; 2 is its own partner


@pytest.mark.parametrize("kind", M.LAMS)
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("C,dtype,eps,z", [(10, torch.float32, 0.0, 0.0), (1000, torch.bfloat16, 0.1, 1e-4),
                                          (1025, torch.float16, 0.1, 1e-4)])
def test_cpu_fallback_within_the_bounds(C, dtype, eps, z, reduction, kind):
    x, a, b = M.make_case(C, dtype)
    lam = M.make_lam(kind)
    g = M.g_rows() if reduction == "none" else 3.0
    ref = M.mixed_ref(x, a, b, lam, -100, eps, z, reduction, g)
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, MixedTarget(a, b, lam), label_smoothing=eps, z_loss=z, reduction=reduction)
    out.backward(g if torch.is_tensor(g) else torch.tensor(g))
    R.check_elem("fallback loss", out.detach().reshape(-1), ref["reduced"].reshape(-1), torch.float32,
                 M.MC["reduced"], ref["reduced_scale"].reshape(-1))
    R.check_elem("fallback grad", x1.grad, ref["grad"], dtype, M.MC[M.grad_key(eps, C)], ref["grad_scale"])
    for row in (M.ROW_A_IGNORED, M.ROW_B_IGNORED):
        assert not x1.grad[row].any()


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_cpu_fallback_lam_1_is_the_hard_target_fallback_on_a(reduction):
    x, a, b = M.make_case(10, torch.float32)
    b = torch.where(b == -100, torch.zeros_like(b), b)  # keep = a != ignore_index, as for the hard call
    a = torch.where(a == b, (a + 1) % 10, a)  # (an ignored a stays ignored: b >= 0)
    x[torch.arange(M.ROWS), b] = float("-inf")  # the zero-weight target's logit
    outs = []
    for target in (MixedTarget(a, b, torch.ones(1)), a, MixedTarget(b, a, torch.zeros(M.ROWS)),
                   MixedTarget(a, b, 1.0)):
        x1 = x.clone().requires_grad_()
        out = cross_entropy(x1, target, label_smoothing=0.0, z_loss=1e-4, reduction=reduction)
        out.sum().backward()
        outs.append((out.detach(), x1.grad))
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    for out, grad in outs[1:]:
        assert torch.equal(out, outs[0][0]) and torch.equal(grad, outs[0][1])


def test_module_takes_a_mixed_target():
    x, a, b = M.make_case(10, torch.float32)
    t = MixedTarget(a, b, M.make_lam("rows"))
    mod = CrossEntropyLoss(label_smoothing=0.1, reduction="sum")
    assert torch.equal(mod(x, t), cross_entropy(x, t, label_smoothing=0.1, reduction="sum"))


def test_bad_lam_and_shapes_raise_value_error():
    x, a, b = M.make_case(10, torch.float32)
    for lam in (torch.ones(2), torch.ones(M.ROWS + 1), torch.ones(0)):
        with pytest.raises(ValueError, match="lam"):
            cross_entropy(x, MixedTarget(a, b, lam))
    with pytest.raises(ValueError):
        cross_entropy(x, MixedTarget(a, b[:-1], torch.ones(1)))
    with pytest.raises(ValueError):
        cross_entropy(x, MixedTarget(a, b, torch.ones(1)), reduction="avg")
    img = M.make_images((3, 3, 4, 4), torch.float32)
    with pytest.raises(ValueError):
        mix_images(img, None, torch.ones(2), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        mix_images(img, None, torch.ones(1), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        mix_images(img[0], None, torch.ones(1), torch.zeros(1, 4, dtype=torch.int32))
