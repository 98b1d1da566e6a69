"""The fp64 Mixup / CutMix references and bounds of tests/_mix_refs.py, checked without a GPU: fp32
torch stays within a quarter of every bound (the constants are 4 x its measured error), and the
reference is the hard-target reference of tests/_xent_refs.py where the two targets agree or one
weight is 0."""
import pytest
import torch

import _mix_refs as M
import _xent_refs as X


def test_fp32_torch_within_a_quarter_of_each_bound():
    worst = M.measure(quarter_of=M.MC)
    print({k: round(v, 2) for k, v in worst.items()})


@pytest.mark.parametrize("kind,which", [("1", "a"), ("0", "b")])
@pytest.mark.parametrize("eps,z", M.TERMS)
@pytest.mark.parametrize("C", [1, 10, 1025])
def test_reference_is_the_hard_target_reference_at_lam_0_and_1(C, eps, z, kind, which):
    x, a, b = M.make_case(C, torch.float32)
    keep = (a != -100) & (b != -100)
    t = torch.where(keep, a if which == "a" else b, torch.full_like(a, -100))
    ref = M.mixed_ref(x, a, b, M.make_lam(kind), -100, eps, z, "mean", 3.0)
    hard = X.xent_heads_ref(x, t, -100, eps, z, "mean", 3.0)
    for key in ("lse", "loss", "loss_scale", "reduced", "grad", "grad_scale"):
        assert torch.equal(ref[key], hard[key]), key


def test_reference_leaves_a_zero_weight_out():
    x, a, b = M.make_case(10, torch.float32)
    x[torch.arange(M.ROWS), b.clamp_min(0)] = float("-inf")  # (an ignored b: column 0, on a row that is not kept)
    a = torch.where(a == b, (a + 1) % 10, a)
    ref = M.mixed_ref(x, a, b, M.make_lam("1"))
    assert torch.isfinite(ref["loss"]).all() and torch.isfinite(ref["grad"]).all()
    ref = M.mixed_ref(x, a, b, M.make_lam("0.3"))
    keep = (a != -100) & (b != -100)
    assert torch.isinf(ref["loss"][keep]).all() and not ref["loss"][~keep].any()


def test_cases_cover_what_they_claim():
    cases = M.cases()
    assert {c[0] for c in cases} == set(M.WIDTHS) and {c[1:3] for c in cases if c[0] == 10} >= {
        (torch.float16, 0.0), (torch.float16, 0.1)}
    x, a, b = M.make_case(1000, torch.bfloat16, 3)
    assert a[M.ROW_SAME] == b[M.ROW_SAME] and (a[M.ROW_ENDS], b[M.ROW_ENDS]) == (0, 999)
    assert a[M.ROW_A_IGNORED] == 3 and b[M.ROW_B_IGNORED] == 3 and a[M.ROW_CLASS3] == 3
    lam = M.make_lam("rows")
    assert (lam[M.ROW_LAM0], lam[M.ROW_LAM1], lam[M.ROW_LAM_HALF]) == (0.0, 1.0, 0.5)
    assert ((lam >= 0) & (lam <= 1)).all()
