"""Mixup / CutMix on the GPU: the image-mixing kernel (mixup.hip via data/mixup.py) against torch
indexing (bitwise for the copies and for lam in {0, 1}) and the fp64 bound of tests/_mix_refs.py,
the two-label cross-entropy (cross_entropy_mixed.hip via ops/cross_entropy.py) against the fp64
reference and per-element bounds over _mix_refs.cases() and bitwise against the hard-target
kernels at lam in {0, 1}, the whole step in a HIP graph, and the hard-target path unchanged.
"""
import pytest
import torch
import torch.nn.functional as F

import _mix_refs as M
import _row_refs as R

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from distributeddataparallel_amd._native import load  # noqa: E402
from distributeddataparallel_amd.data import Mixup, mix_images  # noqa: E402
from distributeddataparallel_amd.ops import CrossEntropyLoss, MixedTarget  # noqa: E402
from distributeddataparallel_amd.ops.cross_entropy import check_targets, cross_entropy  # noqa: E402

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
FORMATS = {"nchw": torch.contiguous_format, "nhwc": torch.channels_last}


def ids(v):
    return NAME.get(v, "x".join(map(str, v)) if isinstance(v, tuple) else str(v))


def fresh_flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def f32(values):
    return torch.tensor(values, dtype=F32, device=DEV).reshape(-1)


def boxes(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV).reshape(-1, 4)


# ---- the mixing kernel -----------------------------------------------------------------------------
def shared_plans(H, W):
    """(name, lam, box) with one lam and one box for the batch."""
    empty = [0, 0, 0, 0]
    out = [(f"mixup lam={lam}", [lam], empty) for lam in (0.0, 1.0, 0.3)]
    out.append(("empty box with a height", [0.3], [0, H, 2, 2]))
    out.append(("full image", [0.0], [0, H, 0, W]))
    for y in (0, H - 1):
        for x in (0, W - 1):
            out.append((f"pixel ({y}, {x})", [1 - 1 / (H * W)], [y, y + 1, x, x + 1]))
    out.append(("top border", [0.5], [0, H // 2, 1, W - 1]))
    out.append(("bottom border", [0.5], [H // 2, H, 1, W - 1]))
    out.append(("left border", [0.5], [1, H - 1, 0, W // 2]))
    out.append(("right border", [0.5], [1, H - 1, W // 2, W]))
    return out


def per_sample_plan(B, H, W):
    lam = M.image_lams(B)[1].tolist()
    box = [[1, H - 1, 2, W], [0, 0, 0, 0], [H - 1, H, 0, 1]][:B]
    if B > 1:
        lam[-1] = 1.0 if box[B - 1] == [0, 0, 0, 0] else lam[-1]
    return ("per sample", lam, box)


def check_mix(tag, out, x, partner, lam, box):
    """Every sample of out against the rule: copies bitwise, the blend within the _mix_refs bound."""
    B = x.shape[0]
    assert out.dtype == x.dtype and out.shape == x.shape and out.stride() == x.stride(), f"{tag}: layout"
    for i in range(B):
        j = B - 1 - i if partner is None else int(partner[i])
        w = float(lam[i if lam.numel() > 1 else 0])
        y0, y1, x0, x1 = box[i if box.shape[0] > 1 else 0].tolist()
        if y1 > y0 and x1 > x0:
            want = x[i].clone()
            want[:, y0:y1, x0:x1] = x[j, :, y0:y1, x0:x1]
            assert torch.equal(out[i], want), f"{tag}: CutMix sample {i} is not the copy"
        elif w in (0.0, 1.0):
            assert torch.equal(out[i], x[i] if w == 1.0 else x[j]), f"{tag}: lam = {w} sample {i} is not bitwise"
        else:
            ref, scale = M.mix_ref(x[[i, j]], torch.tensor([1, 0], device=DEV), f32([w]))
            R.check_elem(f"{tag} sample {i}", out[i], ref[0], x.dtype, M.MC["mix"], scale[0])


def run_plans(tag, x, partners):
    B, _, H, W = x.shape
    before = x.clone()
    for name, lam, box in shared_plans(H, W) + [per_sample_plan(B, H, W)]:
        lam, box = f32(lam), boxes(box)
        for partner in partners:
            out = mix_images(x, partner, lam, box)
            check_mix(f"{tag} {name} partner={'flip' if partner is None else 'perm'}", out, x, partner, lam, box)
    assert torch.equal(x, before), f"{tag}: x was written"


@pytest.mark.parametrize("fmt", FORMATS, ids=str)
@pytest.mark.parametrize("shape,dtype", M.image_cases(), ids=ids)
def test_mix_images_shapes_and_plans(shape, dtype, fmt):
    """B in {1, 2, 3} (the middle sample of 3 is its own partner), [B, 3, 5, 7] on the scalar
    kernel, the others on the 16-B kernel (rows of 7 .. 672 elements that the 8-element groups
    straddle), both memory formats; shared and per-sample plans, the flip and a permutation."""
    B = shape[0]
    x = M.make_images(shape, dtype, DEV).contiguous(memory_format=FORMATS[fmt])
    perm = torch.tensor([(i + 1) % B for i in range(B)], dtype=torch.int32, device=DEV)
    run_plans(f"{ids(shape)} {NAME[dtype]} {fmt}", x, [None, perm])


@pytest.mark.parametrize("fmt", FORMATS, ids=str)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=ids)
def test_mix_images_unaligned_base(dtype, fmt):
    """x[1:] of a larger batch (a sample of 105 elements: every sample misaligned differently), and
    a view one element into a buffer at a sample size the 16-B kernel would take."""
    big = M.make_images((4, 3, 5, 7), dtype, DEV).contiguous(memory_format=FORMATS[fmt])
    x = big[1:]
    assert x.data_ptr() % 16 != 0
    run_plans(f"x[1:] {NAME[dtype]} {fmt}", x, [None])
    n = 2 * 3 * 32 * 32
    flat = M.make_images((n + 8,), dtype, DEV)
    x = flat[1:n + 1].view(2, 3, 32, 32)
    if fmt == "nhwc":
        x = flat[1:n + 1].view(2, 32, 32, 3).permute(0, 3, 1, 2)
    assert x.data_ptr() % 16 != 0 and x.is_contiguous(memory_format=FORMATS[fmt])
    run_plans(f"offset view {NAME[dtype]} {fmt}", x, [None])


@pytest.mark.parametrize("fmt", FORMATS, ids=str)
@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (3, 3, 32, 32)], ids=ids)
def test_mix_images_zero_weight_does_not_leak(shape, fmt):
    for dtype in (BF16, F32):
        x = M.make_images(shape, dtype, DEV).contiguous(memory_format=FORMATS[fmt])
        x[2] = float("nan")
        x[1, 0, 0, 0] = float("inf")
        empty = boxes([0, 0, 0, 0])
        out = mix_images(x, None, f32([1.0]), empty)  # sample 0 keeps x[0]; its partner is all NaN
        assert torch.equal(out[0], x[0]) and torch.equal(out[1], x[1])
        out = mix_images(x, None, f32([0.0]), empty)  # sample 2 (all NaN) becomes x[0]
        assert torch.equal(out[2], x[0]) and torch.equal(out[1], x[1])
        out = mix_images(x, None, f32([1.0, 0.5, 0.0]), empty)
        assert torch.equal(out[0], x[0]) and torch.equal(out[2], x[0])


def test_mix_images_refuses_what_is_not_dense():
    x = M.make_images((2, 3, 8, 16), BF16, DEV)
    lam, box = f32([0.3]), boxes([0, 0, 0, 0])
    with pytest.raises(RuntimeError, match="dense"):
        load().mix_images(x[:, :, :, ::2], None, lam, box)
    with pytest.raises(RuntimeError, match="partner"):
        load().mix_images(x, torch.zeros(2, dtype=torch.long, device=DEV), lam, box)
    sliced = x[:, :, :, ::2]
    out = mix_images(sliced, None, lam, box)  # the Python layer makes it dense
    check_mix("made dense", out, sliced.contiguous(), None, lam, box)
    x0 = torch.empty(0, 3, 8, 8, device=DEV, dtype=BF16)
    assert mix_images(x0, None, lam, box).shape == x0.shape


def test_mixup_object_on_the_gpu():
    mixer = Mixup(mode="elem", seed=4)
    x = M.make_images((3, 3, 32, 32), BF16, DEV).contiguous(memory_format=torch.channels_last)
    labels = torch.tensor([1, 2, 3], device=DEV)
    where = None
    for _ in range(4):
        out, target = mixer(x, labels)
        plan = mixer.plan
        where = where or (plan.lam.data_ptr(), plan.box.data_ptr())
        assert where == (plan.lam.data_ptr(), plan.box.data_ptr()), "the plan's device tensors moved"
        assert torch.equal(plan.lam.cpu(), torch.from_numpy(plan.host_lam))
        assert torch.equal(plan.box.cpu(), torch.from_numpy(plan.host_box))
        check_mix("Mixup()", out, x, None, plan.lam, plan.box)
        assert torch.equal(target.a, labels) and torch.equal(target.b, labels.flip(0)) and target.lam is plan.lam


# ---- the two-label cross-entropy ---------------------------------------------------------------------
def check_forward(tag, x, a, b, lam, ii, eps, z, ref, rows=None):
    """cross_entropy_mixed_forward called directly: per-row loss and lse, and no bad-target flag."""
    flag = fresh_flag()
    loss, lse = load().cross_entropy_mixed_forward(x, a, b, lam, ii, eps, z, 0, flag)
    sel = slice(None) if rows is None else rows
    R.check_elem(f"{tag} lse", lse[sel], ref["lse"][sel], F32, R.C["xent_lse"], ref["lse_scale"][sel])
    R.check_elem(f"{tag} loss", loss[sel], ref["loss"][sel], F32, M.MC["loss"], ref["loss_scale"][sel])
    assert int(flag) == 0, f"{tag}: bad-target flag set"
    return loss, lse


def check_op(tag, x, a, b, lam, ii, eps, z, reduction, g, ref):
    """ops.cross_entropy on a MixedTarget: the reduced loss and every element of the gradient."""
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, MixedTarget(a, b, lam), ii, label_smoothing=eps, z_loss=z, reduction=reduction)
    assert out.dtype == F32 and out.shape == ref["reduced"].shape
    out.backward(g if torch.is_tensor(g) else torch.tensor(g, device=DEV))
    R.check_elem(f"{tag} {reduction}", out.detach().reshape(-1), ref["reduced"].reshape(-1), F32, M.MC["reduced"],
                 ref["reduced_scale"].reshape(-1))
    assert x1.grad.dtype == x.dtype
    R.check_elem(f"{tag} grad", x1.grad, ref["grad"], x.dtype, M.MC[M.grad_key(eps, x.shape[1])], ref["grad_scale"])
    return out.detach(), x1.grad


@pytest.mark.parametrize("C,dtype,eps,z", M.cases(), ids=ids)
def test_mixed_xent_edges(C, dtype, eps, z):
    """33 rows (the last narrow block has three idle waves); a == b, the two ends of the row, a or b
    ignored; lam 0.3, 0, 1 and per row (with exact 0, 1 and 0.5); two ignore_index values; every
    reduction with g in {1, 3} and a per-row g for "none"."""
    g_rows = M.g_rows().to(DEV)
    for ii in M.IGNORE:
        x, a, b = M.make_case(C, dtype, ii, device=DEV)
        for kind in M.LAMS:
            lam = M.make_lam(kind, device=DEV)
            tag = f"C={C} {NAME[dtype]} eps={eps} z={z} ii={ii} lam={kind}"
            for reduction, g in M.REDUCTIONS:
                g = g_rows if g is None else g
                ref = M.mixed_ref(x, a, b, lam, ii, eps, z, reduction, g)
                if reduction == "none":
                    loss, _ = check_forward(tag, x, a, b, lam, ii, eps, z, ref)
                    for row in (M.ROW_A_IGNORED, M.ROW_B_IGNORED):
                        assert loss[row].item() == 0.0, "an ignored row got a loss"
                _, grad = check_op(f"{tag} g={'rows' if torch.is_tensor(g) else g}", x, a, b, lam, ii, eps, z,
                                   reduction, g, ref)
                assert not grad[M.ROW_A_IGNORED].any() and not grad[M.ROW_B_IGNORED].any(), "an ignored row got a gradient"
    check_targets(block=True)


def hard_pair(C, dtype, ii, mask):
    """A case whose b is never ignored (keep is then a != ignore_index, as for the hard call), with
    -inf at b's logit wherever b != a (the zero-weight target when lam = 1)."""
    x, a, b = M.make_case(C, dtype, ii, device=DEV)
    b = torch.where(b == ii, torch.full_like(b, C - 1), b)
    if mask and C > 1:
        rows = (a != b).nonzero()[:, 0]
        x[rows, b[rows]] = float("-inf")
    return x, a, b


@pytest.mark.parametrize("mask", [False, True], ids=["finite", "masked"])
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=ids)
@pytest.mark.parametrize("C", [1, 10, 1000, 1024, 1025, 4099])
def test_mixed_xent_lam_0_and_1_are_the_hard_target_kernels_bitwise(C, dtype, mask):
    C_ = load()
    g1, g_rows = f32([3.0]), M.g_rows().to(DEV)
    for ii in M.IGNORE:
        x, a, b = hard_pair(C, dtype, ii, mask)
        for eps, z in ((0.0, 1e-4), (0.0, 0.0)) if mask else M.TERMS:
            for red in (0, 1, 2):
                hard = C_.cross_entropy_rows_forward(x, a, ii, eps, z, red, fresh_flag())
                g = g_rows if red == 0 else g1
                dhard = C_.cross_entropy_rows_backward(x, a, hard[1], g, hard[3] if red == 2 else None, ii, eps, z)
                assert torch.isfinite(hard[0]).all() and torch.isfinite(dhard).all()
                for first, second, lam in ((a, b, f32([1.0])), (b, a, f32([0.0])), (a, b, torch.ones(M.ROWS, device=DEV)),
                                           (b, a, torch.zeros(M.ROWS, device=DEV))):
                    flag = fresh_flag()
                    got = C_.cross_entropy_mixed_forward(x, first, second, lam, ii, eps, z, red, flag)
                    assert len(got) == len(hard) and int(flag) == 0
                    for k, (u, v) in enumerate(zip(got, hard)):
                        assert torch.equal(u, v), f"C={C} ii={ii} eps={eps} z={z} reduction={red}: output {k} differs"
                    d = C_.cross_entropy_mixed_backward(x, first, second, lam, got[1], g, got[3] if red == 2 else None,
                                                        ii, eps, z)
                    assert torch.equal(d, dhard), f"C={C} ii={ii} eps={eps} z={z} reduction={red}: gradient differs"


@pytest.mark.parametrize("C,dtype", [(1000, BF16), (10, F32), (4099, F32)], ids=ids)
def test_mixed_xent_op_lam_1_is_the_hard_target_op_bitwise(C, dtype):
    """Through ops.cross_entropy, at arguments that take cross_entropy_rows.hip for the hard target."""
    x, a, b = hard_pair(C, dtype, -100, True)
    for reduction in ("none", "sum", "mean"):
        runs = []
        for target in (a, MixedTarget(a, b, f32([1.0])), MixedTarget(b, a, 0.0)):
            x1 = x.clone().requires_grad_()
            out = cross_entropy(x1, target, z_loss=1e-4, reduction=reduction)
            out.sum().backward()
            runs.append((out.detach(), x1.grad))
        assert torch.isfinite(runs[0][0]).all()
        for out, grad in runs[1:]:
            assert torch.equal(out, runs[0][0]) and torch.equal(grad, runs[0][1])


@pytest.mark.parametrize("dtype", [BF16, F32], ids=ids)
@pytest.mark.parametrize("C", [1000, 4099])
def test_mixed_xent_masked_logits(C, dtype):
    """-inf spans at the start and the end of rows 0 .. 15, as test_xent_heads_masked_logits. eps = 0:
    finite loss, masked columns get exactly 0; a masked target gives +inf under a positive weight and
    nothing under a zero weight."""
    x, a, b = M.make_case(C, dtype, device=DEV)
    lo, hi = 300, C - 259
    x[:16, :lo] = float("-inf")
    x[:16, hi:] = float("-inf")
    gen = torch.Generator().manual_seed(2)
    a = torch.randint(lo, hi, a.shape, generator=gen).to(DEV)
    b = torch.randint(lo, hi, b.shape, generator=gen).to(DEV)
    lam = M.make_lam("rows", device=DEV)
    ref = M.mixed_ref(x, a, b, lam, -100, 0.0, 1e-4, "mean", 3.0)
    assert torch.isfinite(ref["loss"]).all()
    tag = f"masked C={C} {NAME[dtype]}"
    check_forward(tag, x, a, b, lam, -100, 0.0, 1e-4, ref)
    _, grad = check_op(tag, x, a, b, lam, -100, 0.0, 1e-4, "mean", 3.0, ref)
    assert (grad[:16, :lo] == 0).all() and (grad[:16, hi:] == 0).all(), "a masked column got a gradient"
    # masked targets: rows 0 .. 3 positively weighted (+inf), rows ROW_LAM0 / ROW_LAM1 under the zero weight
    a[:2] = 0
    b[2:4] = C - 1
    a[M.ROW_LAM0] = 1
    b[M.ROW_LAM1] = C - 2
    assert ((lam[:4] > 0) & (lam[:4] < 1)).all()
    ref = M.mixed_ref(x, a, b, lam, -100, 0.0, 0.0, "none", 1.0)
    assert torch.isinf(ref["loss"][:4]).all() and torch.isfinite(ref["loss"][4:]).all()
    loss, _ = check_forward(tag + " masked targets", x, a, b, lam, -100, 0.0, 0.0, ref, rows=slice(4, None))
    assert (loss[:4] == float("inf")).all()
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, MixedTarget(a, b, lam), reduction="none")
    out[4:].sum().backward()
    assert torch.equal(out.detach(), loss) and not x1.grad[:4].any()
    R.check_elem(tag + " masked targets grad", x1.grad[4:], ref["grad"][4:], dtype, M.MC["grad"], ref["grad_scale"][4:])
    # eps > 0: the smoothing term makes every masked row +inf, as for the hard target
    loss, _ = load().cross_entropy_mixed_forward(x, a, b, lam, -100, 0.1, 0.0, 0, fresh_flag())
    assert (loss[:16] == float("inf")).all() and torch.isfinite(loss[16:]).all()


@pytest.mark.parametrize("C", [10, 1025])
def test_mixed_xent_bad_target(C):
    check_targets(block=True)  # clean slate
    x, a, b = M.make_case(C, F32, device=DEV)
    lam = M.make_lam("rows", device=DEV)
    b[M.ROW_A_IGNORED] = C + 5  # on an ignored row: nothing happens
    a[M.ROW_B_IGNORED] = -7
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, MixedTarget(a, b, lam), reduction="none")
    out.sum().backward()
    check_targets(block=True)
    assert torch.isfinite(out).all() and torch.isfinite(x1.grad).all()
    assert not out[M.ROW_A_IGNORED].item() and not x1.grad[M.ROW_A_IGNORED].any()
    for bad_row, value in ((10, C), (M.ROW_LAM1, -1)):  # (the second under a zero weight: still an error)
        b2 = b.clone()
        b2[bad_row] = value
        others = torch.arange(M.ROWS, device=DEV) != bad_row
        x1 = x.clone().requires_grad_()
        out = cross_entropy(x1, MixedTarget(a, b2, lam), reduction="none")
        out[others].sum().backward()
        assert torch.isnan(out[bad_row]).item() and torch.isfinite(out[others]).all()
        assert not x1.grad[bad_row].any() and x1.grad[0].any()
        with pytest.raises(IndexError, match="out of bounds"):
            check_targets(block=True)
        check_targets(block=True)  # the flag was consumed
    assert torch.isnan(cross_entropy(x, MixedTarget(a, b2, lam))).item()  # the mean shows it at once
    with pytest.raises(IndexError):
        check_targets(block=True)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=ids)
@pytest.mark.parametrize("C", [10, 1025])
def test_mixed_xent_one_row_and_no_rows(C, dtype):
    x, a, b = M.make_case(C, dtype, rows=1, device=DEV)
    for lam in (f32([0.3]), f32([1.0])):
        ref = M.mixed_ref(x, a, b, lam, -100, 0.1, 1e-4, "mean", 3.0)
        check_forward(f"C={C} one row", x, a, b, lam, -100, 0.1, 1e-4, ref)
        check_op(f"C={C} one row", x, a, b, lam, -100, 0.1, 1e-4, "mean", 3.0, ref)
    x0 = torch.empty(0, C, device=DEV, dtype=dtype, requires_grad=True)
    t0 = torch.empty(0, device=DEV, dtype=torch.long)
    for reduction in ("none", "sum", "mean"):
        out = cross_entropy(x0, MixedTarget(t0, t0, f32([0.3])), label_smoothing=0.1, reduction=reduction)
        assert out.shape == ((0,) if reduction == "none" else ()) and not out.any()
        out.sum().backward()
        assert x0.grad.shape == (0, C)
    with pytest.raises(ValueError, match="lam"):
        cross_entropy(x, MixedTarget(a, b, torch.ones(2, device=DEV)))


def test_mixed_xent_all_rows_ignored_and_module():
    x, a, b = M.make_case(1000, BF16, device=DEV)
    lam = M.make_lam("rows", device=DEV)
    for reduction in ("none", "sum", "mean"):
        x1 = x.clone().requires_grad_()
        out = cross_entropy(x1, MixedTarget(a, torch.full_like(b, -100), lam), label_smoothing=0.1, reduction=reduction)
        out.sum().backward()
        assert not out.any() and torch.isfinite(out).all() and not x1.grad.any()
    mod = CrossEntropyLoss(ignore_index=3, label_smoothing=0.1, z_loss=1e-4, reduction="sum")
    x, a, b = M.make_case(1000, BF16, 3, device=DEV)
    t = MixedTarget(a, b, lam)
    assert torch.equal(mod(x, t), cross_entropy(x, t, 3, label_smoothing=0.1, z_loss=1e-4, reduction="sum"))


def test_mixed_xent_fallback_not_taken_and_repeatable(monkeypatch):
    def boom(*args, **kwargs):
        raise AssertionError("F.cross_entropy called: the fallback was taken")

    monkeypatch.setattr(torch.nn.functional, "cross_entropy", boom)
    for rows, C, dtype in ((32, 10, F32), (256, 1000, BF16), (64, 4099, F32)):
        x, a, b = M.make_case(C, dtype, rows=rows, device=DEV)
        lam = torch.rand(rows, generator=torch.Generator().manual_seed(3)).to(DEV)
        runs = []
        for _ in range(2):
            x1 = x.clone().requires_grad_()
            out = cross_entropy(x1, MixedTarget(a, b, lam), label_smoothing=0.1, z_loss=1e-4)
            out.backward()
            runs.append((out.detach().clone(), x1.grad))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        ref = M.mixed_ref(x, a, b, lam, -100, 0.1, 1e-4, "mean", 1.0)
        R.check_elem(f"[{rows}, {C}]", runs[0][1], ref["grad"], dtype, M.MC[M.grad_key(0.1, C)], ref["grad_scale"])


# ---- capture, and the hard-target path --------------------------------------------------------------
def test_mixup_step_captures_in_a_hip_graph():
    """Mixup.apply, a linear layer, the two-label loss and the backward in one graph; a draw before
    each replay changes the mix, and each replay is the eager step on that plan, bitwise."""
    B, C = 8, 10
    torch.manual_seed(0)
    x = M.make_images((B, 3, 8, 8), F32, DEV).contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(1)).to(DEV)
    lin = torch.nn.Linear(3 * 8 * 8, C).to(DEV)
    mixer = Mixup(mode="elem", seed=9)

    def step():
        lin.zero_grad(set_to_none=True)
        xm, target = mixer.apply(x, labels)
        loss = cross_entropy(lin(xm.flatten(1)), target, label_smoothing=0.1)
        loss.backward()
        return xm, loss

    mixer.draw(B, 8, 8, DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm up outside the capture
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    lin.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        xm, loss = step()
    wgrad = lin.weight.grad
    replays = []
    for _ in range(2):
        plan = mixer.draw(B, 8, 8, DEV)
        graph.replay()
        torch.cuda.synchronize()
        got = (xm.clone(), loss.detach().clone(), wgrad.clone())
        check_mix("replayed mix", got[0], x, None, plan.lam, plan.box)
        eager_x, eager_loss = step()  # eager, on the same plan
        assert torch.equal(got[0], eager_x) and torch.equal(got[1], eager_loss.detach())
        assert torch.equal(got[2], lin.weight.grad)
        assert torch.isfinite(got[1]).item()
        replays.append(got)
    assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[0][1], replays[1][1])
    check_targets(block=True)


@pytest.mark.parametrize("C,dtype", [(1000, BF16), (10, F32)], ids=ids)
def test_hard_target_path_is_untouched_by_the_mixed_op(C, dtype):
    """cross_entropy(x, a) gives the same bits before and after the two-label op ran, and those of
    the kernels it has always run."""
    x, a, b = M.make_case(C, dtype, device=DEV)

    def hard():
        x1 = x.clone().requires_grad_()
        out = cross_entropy(x1, a)
        out.backward(torch.tensor(3.0, device=DEV))
        return out.detach().clone(), x1.grad.clone()

    before = hard()
    x2 = x.clone().requires_grad_()
    cross_entropy(x2, MixedTarget(a, b, f32([0.3])), label_smoothing=0.1).backward()
    after = hard()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    if dtype == BF16:  # C % 8 == 0 and default arguments: cross_entropy.hip
        loss_rows, lse = load().cross_entropy_forward(x, a, -100, fresh_flag())
        count = (a != -100).sum().clamp_min(1).to(F32)
        grad = load().cross_entropy_backward(x, a, lse, (torch.tensor(3.0, device=DEV) / count).reshape(1), -100)
        assert torch.equal(before[0], loss_rows.sum() / count)
    else:
        out = load().cross_entropy_rows_forward(x, a, -100, 0.0, 0.0, 2, fresh_flag())
        grad = load().cross_entropy_rows_backward(x, a, out[1], f32([3.0]), out[3], -100, 0.0, 0.0)
        assert torch.equal(before[0], out[2])
    assert torch.equal(before[1], grad)
    ref = F.cross_entropy(x.float(), a)
    assert abs(before[0].item() - ref.item()) <= 1e-5 * abs(ref.item()) + 1e-6
