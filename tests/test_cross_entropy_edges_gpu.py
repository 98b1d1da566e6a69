"""Softmax cross-entropy kernels (cross_entropy.hip) at their row-length and value edges: per-row
loss and lse and every element of the gradient against an fp64 reference on the same bf16 logits.
The gradient's bound is per element (one bf16 ulp of (softmax - onehot) g / count plus an fp32
term), so the softmax tail counts: a backward that wrote zeros off the target column fails.
Bounds and their measured constants: tests/_row_refs.py.
"""
import pytest
import torch

import _row_refs as R

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from distributeddataparallel_amd._native import load  # noqa: E402
from distributeddataparallel_amd.ops import cross_entropy as xent_mod  # noqa: E402
from distributeddataparallel_amd.ops.cross_entropy import check_targets, cross_entropy  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def fresh_flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def check_forward(tag, x, t, ignore_index, ref, rows=None):
    """cross_entropy_forward called directly: per-row loss and lse, and no bad-target flag."""
    flag = fresh_flag()
    loss, lse = load().cross_entropy_forward(x, t, ignore_index, flag)
    sel = slice(None) if rows is None else rows
    R.check_elem(f"{tag} lse", lse[sel], ref["lse"][sel], F32, R.C["xent_lse"], ref["lse_scale"][sel])
    R.check_elem(f"{tag} loss", loss[sel], ref["loss"][sel], F32, R.C["xent_loss"], ref["loss_scale"][sel])
    assert int(flag) == 0, f"{tag}: bad-target flag set"
    return loss, lse


def check_op(tag, x, t, ignore_index, g, ref):
    """ops.cross_entropy: the mean, and every element of the bf16 gradient."""
    x1 = x.clone().requires_grad_()
    m = cross_entropy(x1, t, ignore_index)
    m.backward(torch.tensor(g, device=DEV))
    R.check_elem(f"{tag} mean", m.detach().reshape(1), ref["mean"].reshape(1), F32, R.C["xent_loss"],
                 (ref["loss_scale"].sum() / ref["count"]).reshape(1))
    R.check_elem(f"{tag} grad", x1.grad, ref["grad"], BF16, R.C["xent_grad"], ref["grad_scale"])
    check_targets(block=True)
    return x1.grad


# V = 8: one thread holds data, 255 are empty; 2048: every thread one trip; 2056: exactly one
# thread takes a second trip; 4104: one thread a third; 128256: the Llama-3 vocabulary.
@pytest.mark.parametrize("g", [1.0, 3.0])
@pytest.mark.parametrize("ignore_index", [-100, 3])
@pytest.mark.parametrize("V", [8, 2048, 2056, 4104, 128256])
def test_cross_entropy_edges(V, ignore_index, g):
    torch.manual_seed(0)
    rows = 8 if V == 128256 else 33
    x = torch.randn(rows, V, device=DEV).to(BF16)
    t = torch.randint(0, V, (rows,), device=DEV)
    t[0], t[1], t[2], t[3] = 0, V - 1, V - 8, V - 3  # first and last column, the last 8-wide vector
    t[4], t[5] = 3, -100  # 3 is a valid class: ignored only when it is the ignore_index
    if ignore_index != -100:
        t[5] = ignore_index
    ref = R.xent_ref(x, t, ignore_index, g)
    assert ref["count"].item() == rows - (1 if ignore_index == -100 else int((t == 3).sum()))
    tag = f"xent V={V} ii={ignore_index} g={g}"
    check_forward(tag, x, t, ignore_index, ref)
    grad = check_op(tag, x, t, ignore_index, g, ref)
    assert not grad[5].any(), "an ignored row got a gradient"


@pytest.mark.parametrize("ignore_index", [-100, 3])
def test_cross_entropy_all_rows_ignored(ignore_index):
    """Every target is ignore_index: the divisor is clamp_min(1), so the loss is a finite 0 and the
    gradient all zeros (F.cross_entropy returns NaN here: 0 / 0), and no flag is set."""
    torch.manual_seed(0)
    x = torch.randn(33, 2056, device=DEV).to(BF16).requires_grad_()
    t = torch.full((33,), ignore_index, device=DEV)
    check_targets(block=True)
    m = cross_entropy(x, t, ignore_index)
    m.backward()
    assert m.item() == 0.0
    assert not x.grad.any()
    check_targets(block=True)
    assert int(xent_mod._flag(x.device)[0]) == 0
    flag = fresh_flag()
    loss, _ = load().cross_entropy_forward(x.detach(), t, ignore_index, flag)
    assert not loss.any() and int(flag) == 0


@pytest.mark.parametrize("V", [2056, 128256])
def test_cross_entropy_large_common_offset(V):
    """logits = 3e4 + N(0, 1) rounded to bf16 (steps of 128 up there, so two or three distinct
    values per row): lse and loss to the same fp32 bound, relative to |lse|."""
    torch.manual_seed(0)
    rows = 8 if V == 128256 else 33
    x = (3e4 + torch.randn(rows, V, device=DEV)).to(BF16)
    t = torch.randint(0, V, (rows,), device=DEV)
    check_forward(f"xent offset V={V}", x, t, -100, R.xent_ref(x, t))


# -inf in whole aligned 8-wide chunks: a vocabulary padded to a multiple of 128 and masked
# (columns 4000 .. 4095), and a thread whose first chunk is empty (columns 0 .. 63: threads 0 .. 7
# start at -inf, and the per-thread loop used to form exp(-inf - -inf) = NaN there).
@pytest.mark.parametrize("lo,hi", [(4000, 4096), (0, 64)])
def test_cross_entropy_masked_logits(lo, hi):
    torch.manual_seed(0)
    rows, V = 33, 4096
    x = torch.randn(rows, V, device=DEV).to(BF16)
    x[:, lo:hi] = float("-inf")
    t = torch.randint(64, 4000, (rows,), device=DEV)
    ref = R.xent_ref(x, t, -100, 3.0)
    assert torch.isfinite(ref["loss"]).all()
    tag = f"xent -inf [{lo}, {hi})"
    check_forward(tag, x, t, -100, ref)
    grad = check_op(tag, x, t, -100, 3.0, ref)
    assert (grad[:, lo:hi] == 0).all(), "a masked column got a gradient"


def test_cross_entropy_all_masked_row_is_contained():
    """A row that is -inf everywhere has no finite loss (NaN in torch too); it must raise no flag
    and leave the other rows as they are."""
    torch.manual_seed(0)
    rows, V = 33, 4096
    x = torch.randn(rows, V, device=DEV).to(BF16)
    x[7] = float("-inf")
    t = torch.randint(0, V, (rows,), device=DEV)
    others = torch.arange(rows, device=DEV) != 7
    y = x.clone()
    y[7] = 0
    ref = R.xent_ref(y, t)
    check_forward("xent one row all -inf", x, t, -100, ref, rows=others)
