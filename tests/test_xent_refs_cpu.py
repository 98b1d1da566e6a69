"""The fp64 cross-entropy reference and bounds of tests/_xent_refs.py, checked without a GPU: fp32
torch stays within a quarter of every bound (the constants are 4 x its measured error), the
reference is torch's own fp64 cross entropy at z = 0, and the CPU fallback of ops.cross_entropy
computes the same thing for every reduction."""
import pytest
import torch
import torch.nn.functional as F

import _row_refs as R
import _xent_refs as X

from distributeddataparallel_amd.ops.cross_entropy import cross_entropy


def test_fp32_torch_within_a_quarter_of_each_bound():
    worst = X.measure(quarter_of=X.XC)
    print({k: round(v, 2) for k, v in worst.items()})


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("C", [1, 10, 1000, 4099])
def test_reference_is_torch_fp64_at_z0(C, reduction, eps):
    x, t = X.make_case(C, torch.float32, ignore_index=3)
    ref = X.xent_heads_ref(x, t, 3, eps, 0.0, reduction, 1.0)
    x64 = x.double().requires_grad_()
    out = F.cross_entropy(x64, t, ignore_index=3, label_smoothing=eps, reduction=reduction)
    out.sum().backward()
    torch.testing.assert_close(ref["reduced"], out.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["grad"], x64.grad, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("eps,z", [(0.0, 0.0)] + X.TERMS)
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("C,dtype", [(10, torch.float32), (1000, torch.bfloat16), (1025, torch.float16)])
def test_cpu_fallback_matches_reference(C, dtype, reduction, eps, z):
    x, t = X.make_case(C, dtype)
    g = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(1)) if reduction == "none" else 3.0
    ref = X.xent_heads_ref(x, t, -100, eps, z, reduction, g)
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, t, label_smoothing=eps, z_loss=z, reduction=reduction)
    out.backward(g if torch.is_tensor(g) else torch.tensor(g))
    R.check_elem("fallback loss", out.detach().reshape(-1), ref["reduced"].reshape(-1), torch.float32,
                 X.XC["reduced"], ref["reduced_scale"].reshape(-1))
    R.check_elem("fallback grad", x1.grad, ref["grad"], dtype, X.XC[X.grad_key(eps, C)], ref["grad_scale"])


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_cpu_fallback_all_rows_ignored_gives_zero(reduction):
    """The divisor rule (kept rows, at least 1) holds whenever an argument is not the default; with
    every argument at its default the fallback is F.cross_entropy itself, NaN here, as before."""
    x, _ = X.make_case(10, torch.float32)
    t = torch.full((x.shape[0],), 3)
    x1 = x.clone().requires_grad_()
    out = cross_entropy(x1, t, 3, label_smoothing=0.1, z_loss=1e-4, reduction=reduction)
    out.sum().backward()
    assert not out.any() and torch.isfinite(out).all() and not x1.grad.any()
    ref = X.xent_heads_ref(x, t, 3, 0.1, 1e-4, reduction, 1.0)
    assert not ref["reduced"].any() and not ref["grad"].any()
    if reduction != "mean":
        assert not cross_entropy(x, t, 3, reduction=reduction).any()
