"""Cross-entropy for every head (cross_entropy_rows.hip via ops/cross_entropy.py): fp32 / bf16 / fp16
logits at the widths where the kernels turn over, label smoothing, z-loss and the three reductions,
against the fp64 reference and per-element bounds of tests/_xent_refs.py; the bf16 LM-head path
with default arguments must stay bit for bit what it was.
"""
import pytest
import torch
import torch.nn.functional as F

import _row_refs as R
import _xent_refs as X

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from distributeddataparallel_amd._native import load  # noqa: E402
from distributeddataparallel_amd.ops import CrossEntropyLoss  # noqa: E402
from distributeddataparallel_amd.ops import cross_entropy as xent_mod  # noqa: E402
from distributeddataparallel_amd.ops.cross_entropy import check_targets, cross_entropy  # noqa: E402

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}


def fresh_flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def check_forward(tag, x, t, ii, eps, z, ref, rows=None):
    """cross_entropy_rows_forward called directly: per-row loss and lse, and no bad-target flag."""
    flag = fresh_flag()
    loss, lse = load().cross_entropy_rows_forward(x, t, ii, eps, z, 0, flag)
    sel = slice(None) if rows is None else rows
    R.check_elem(f"{tag} lse", lse[sel], ref["lse"][sel], F32, R.C["xent_lse"], ref["lse_scale"][sel])
    R.check_elem(f"{tag} loss", loss[sel], ref["loss"][sel], F32, X.XC["loss"], ref["loss_scale"][sel])
    assert int(flag) == 0, f"{tag}: bad-target flag set"
    return loss, lse


def check_op(tag, x, t, ii, eps, z, reduction, g, ref):
    """ops.cross_entropy: the reduced loss and every element of the gradient."""
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, t, ii, label_smoothing=eps, z_loss=z, reduction=reduction)
    assert out.dtype == F32 and out.shape == ref["reduced"].shape
    out.backward(g if torch.is_tensor(g) else torch.tensor(g, device=DEV))
    R.check_elem(f"{tag} {reduction}", out.detach().reshape(-1), ref["reduced"].reshape(-1), F32, X.XC["reduced"],
                 ref["reduced_scale"].reshape(-1))
    assert x1.grad.dtype == x.dtype
    R.check_elem(f"{tag} grad", x1.grad, ref["grad"], x.dtype, X.XC[X.grad_key(eps, x.shape[1])], ref["grad_scale"])
    check_targets(block=True)
    return out.detach(), x1.grad


@pytest.mark.parametrize("C,dtype,eps,z", X.cases(), ids=lambda v: NAME.get(v, str(v)))
def test_xent_heads_edges(C, dtype, eps, z):
    """33 rows (the last narrow block has three idle waves; 8 rows at 50257), targets on column 0,
    column C - 1, a valid class and ignore_index, two ignore_index values, upstream g in {1, 3}."""
    for ii in (-100, 3):
        x, t = X.make_case(C, dtype, ii, device=DEV)
        for g in (1.0, 3.0):
            ref = X.xent_heads_ref(x, t, ii, eps, z, "mean", g)
            tag = f"C={C} {NAME[dtype]} eps={eps} z={z} ii={ii} g={g}"
            loss, _ = check_forward(tag, x, t, ii, eps, z, ref)
            _, grad = check_op(tag, x, t, ii, eps, z, "mean", g, ref)
            assert loss[5].item() == 0.0 and not grad[5].any(), "an ignored row got a loss or a gradient"
            if C == 1:
                assert not loss.any() and not grad.any()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
@pytest.mark.parametrize("C", [10, 1025])
def test_xent_heads_one_row_and_no_rows(C, dtype):
    x, t = X.make_case(C, dtype, rows=1, device=DEV)
    ref = X.xent_heads_ref(x, t, -100, 0.1, 1e-4, "mean", 3.0)
    check_forward(f"C={C} one row", x, t, -100, 0.1, 1e-4, ref)
    check_op(f"C={C} one row", x, t, -100, 0.1, 1e-4, "mean", 3.0, ref)
    x0 = torch.empty(0, C, device=DEV, dtype=dtype, requires_grad=True)
    t0 = torch.empty(0, device=DEV, dtype=torch.long)
    for reduction in ("none", "sum", "mean"):
        out = cross_entropy(x0, t0, label_smoothing=0.1, reduction=reduction)
        assert out.shape == ((0,) if reduction == "none" else ()) and not out.any()
        out.sum().backward()
        assert x0.grad.shape == (0, C)


@pytest.mark.parametrize("C,dtype", [(1000, BF16), (1025, F32), (10, F32)], ids=lambda v: NAME.get(v, str(v)))
def test_xent_heads_reductions(C, dtype):
    eps, z = 0.1, 1e-4
    x, t = X.make_case(C, dtype, device=DEV)
    g_rows = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)
    for reduction, g in (("none", g_rows), ("sum", 3.0), ("mean", 3.0)):
        ref = X.xent_heads_ref(x, t, -100, eps, z, reduction, g)
        check_op(f"C={C} {NAME[dtype]}", x, t, -100, eps, z, reduction, g, ref)
    for ii in (-100, 3):  # every row ignored: 0 and a zero gradient, also for the mean (divisor 1)
        ta = torch.full_like(t, ii)
        for reduction in ("none", "sum", "mean"):
            x1 = x.clone().requires_grad_()
            out = cross_entropy(x1, ta, ii, label_smoothing=eps, z_loss=z, reduction=reduction)
            out.sum().backward()
            assert not out.any() and not x1.grad.any(), f"{reduction}: all rows ignored"
    check_targets(block=True)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
@pytest.mark.parametrize("C", [1000, 4099])
def test_xent_heads_masked_logits(C, dtype):
    """-inf spans at the start and the end of rows 0 .. 15 (in the wide kernel: a first chunk of
    -inf, chunks of all -inf, -inf in the scalar head and tail). eps = 0: finite loss, masked
    columns get exactly 0. eps = 0.1: those rows' loss is +inf, as in torch. Rows 16 .. 32 are
    within bounds either way."""
    x, t = X.make_case(C, dtype, device=DEV)
    lo, hi = 300, C - 259
    x[:16, :lo] = float("-inf")
    x[:16, hi:] = float("-inf")
    t = torch.randint(lo, hi, t.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    ref = X.xent_heads_ref(x, t, -100, 0.0, 1e-4, "mean", 3.0)
    assert torch.isfinite(ref["loss"]).all()
    tag = f"masked C={C} {NAME[dtype]}"
    check_forward(tag, x, t, -100, 0.0, 1e-4, ref)
    _, grad = check_op(tag, x, t, -100, 0.0, 1e-4, "mean", 3.0, ref)
    assert (grad[:16, :lo] == 0).all() and (grad[:16, hi:] == 0).all(), "a masked column got a gradient"
    ref = X.xent_heads_ref(x, t, -100, 0.1, 0.0, "none", 1.0)
    assert torch.isinf(ref["loss"][:16]).all() and torch.isfinite(ref["loss"][16:]).all()
    loss, _ = check_forward(tag + " eps=0.1", x, t, -100, 0.1, 0.0, ref, rows=slice(16, None))
    assert (loss[:16] == float("inf")).all()
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, t, label_smoothing=0.1, reduction="none")
    out[16:].sum().backward()
    assert torch.equal(out.detach(), loss) and not x1.grad[:16].any()
    R.check_elem(tag + " eps=0.1 grad", x1.grad[16:], ref["grad"][16:], dtype, X.XC[X.grad_key(0.1, C)],
                 ref["grad_scale"][16:])


@pytest.mark.parametrize("C", [1000, 4099])
def test_xent_heads_all_masked_row_is_contained(C):
    """A row that is -inf everywhere has no finite loss; it sets no flag and disturbs no other row."""
    x, t = X.make_case(C, BF16, device=DEV)
    x[7] = float("-inf")
    others = torch.arange(x.shape[0], device=DEV) != 7
    y = x.clone()
    y[7] = 0
    check_forward(f"C={C} one row all -inf", x, t, -100, 0.0, 0.0, X.xent_heads_ref(y, t), rows=others)


def test_xent_heads_bad_target():
    check_targets(block=True)  # clean slate
    x, t = X.make_case(10, F32, device=DEV)
    t[2] = 10
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, t, reduction="none")
    out[torch.arange(33, device=DEV) != 2].sum().backward()
    assert torch.isnan(out[2]).item() and torch.isfinite(out[:2]).all() and torch.isfinite(out[3:]).all()
    assert not x1.grad[2].any() and x1.grad[0].any()
    with pytest.raises(IndexError, match="out of bounds"):
        check_targets(block=True)
    check_targets(block=True)  # the flag was consumed
    assert int(xent_mod._flag(x.device)[0]) == 0
    assert torch.isnan(cross_entropy(x, t)).item()  # the mean shows it at once
    with pytest.raises(IndexError):
        check_targets(block=True)


def test_xent_heads_fallback_not_taken(monkeypatch):
    """The reference workload's fp32 [32, 10] head and the bf16 [256, 1000] ImageNet head with
    label smoothing run the HIP kernels: torch's cross entropy is never called."""
    def boom(*a, **k):
        raise AssertionError("F.cross_entropy called: the fallback was taken")

    monkeypatch.setattr(torch.nn.functional, "cross_entropy", boom)
    for rows, C, dtype, eps in ((32, 10, F32, 0.0), (256, 1000, BF16, 0.1)):
        x, t = X.make_case(C, dtype, rows=rows, device=DEV)
        ref = X.xent_heads_ref(x, t, -100, eps, 0.0, "mean", 1.0)
        check_op(f"[{rows}, {C}] {NAME[dtype]}", x, t, -100, eps, 0.0, "mean", 1.0, ref)


@pytest.mark.parametrize("C", [2056, 4096])
def test_xent_heads_default_path_untouched(C):
    """bf16, C % 8 == 0, default arguments: bitwise the composition the op has always run."""
    x, t = X.make_case(C, BF16, device=DEV)
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, t)
    out.backward(torch.tensor(3.0, device=DEV))
    loss_rows, lse = load().cross_entropy_forward(x, t, -100, fresh_flag())
    count = (t != -100).sum().clamp_min(1).to(F32)
    gscale = (torch.tensor(3.0, device=DEV) / count).reshape(1)
    grad = load().cross_entropy_backward(x, t, lse, gscale, -100)
    assert torch.equal(out.detach(), loss_rows.sum() / count)
    assert torch.equal(x1.grad, grad)


def test_xent_heads_repeatable():
    for C, dtype in ((1000, BF16), (4099, F32)):
        x, t = X.make_case(C, dtype, rows=256, device=DEV)
        runs = []
        for _ in range(2):
            x1 = x.clone().requires_grad_()
            out = cross_entropy(x1, t, label_smoothing=0.1, z_loss=1e-4)
            out.backward()
            runs.append((out.detach().clone(), x1.grad))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_xent_heads_captures_in_hip_graph():
    """Forward and backward at [256, 1000] bf16 with smoothing inside a HIP-graph capture; replays
    on fresh inputs match the eager result bitwise."""
    rows, C = 256, 1000
    x0, t0 = X.make_case(C, BF16, rows=rows, device=DEV, seed=2)
    x = x0.clone().requires_grad_(True)
    t = t0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm up outside the capture
        for _ in range(2):
            x.grad = None
            cross_entropy(x, t, label_smoothing=0.1).backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        loss = cross_entropy(x, t, label_smoothing=0.1)
        loss.backward()
    for seed in (3, 4):
        xn, tn = X.make_case(C, BF16, rows=rows, device=DEV, seed=seed)
        with torch.no_grad():
            x.copy_(xn)
        t.copy_(tn)
        g.replay()
        torch.cuda.synchronize()
        b = xn.clone().requires_grad_(True)
        eager = cross_entropy(b, tn, label_smoothing=0.1)
        eager.backward()
        assert torch.equal(loss.detach(), eager.detach()) and torch.equal(x.grad, b.grad)
        ref = X.xent_heads_ref(xn, tn, -100, 0.1, 0.0, "mean", 1.0)
        R.check_elem("replayed mean", loss.detach().reshape(1), ref["reduced"].reshape(1), F32, X.XC["reduced"],
                     ref["reduced_scale"].reshape(1))


def test_xent_heads_module_matches_function():
    x, t = X.make_case(1000, BF16, ignore_index=3, device=DEV)
    mod = CrossEntropyLoss(ignore_index=3, label_smoothing=0.1, z_loss=1e-4, reduction="sum")
    a, b = x.clone().requires_grad_(), x.clone().requires_grad_()
    la = mod(a, t)
    lb = cross_entropy(b, t, 3, label_smoothing=0.1, z_loss=1e-4, reduction="sum")
    la.backward()
    lb.backward()
    assert torch.equal(la.detach(), lb.detach()) and torch.equal(a.grad, b.grad)
