"""The bounds of tests/_row_refs.py are satisfiable and sharp, shown on the CPU with fp32 torch in
the kernels' place (results rounded to the storage type, as a kernel stores them) at reduced sizes:
fp32 torch passes every check, a copy with one element 4 ulp of a 16-bit storage type off fails, and
a column sum with one row left out fails (in fp32 too). For fp32 storage the element bound is 4 x
fp32 torch's own worst error in units of the operation's terms, which is more than 4 fp32 ulp of
most results, so that perturbation is applied to the 16-bit types only.
"""
import pytest
import torch

import _row_refs as R

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, F16, F32]


def ulp(v, dt):
    """Spacing of dt at v (v a Python float)."""
    t = torch.tensor(v, dtype=torch.float64).to(dt)
    return (torch.nextafter(t.abs(), torch.tensor(float("inf"), dtype=dt)).double() - t.abs().double()).item()


def off_by_4ulp(t, ref, dt):
    """A copy of t (stored as dt) with the element of largest |ref| moved by 4 ulp of dt."""
    i = int(ref.abs().flatten().argmax())
    p = t.clone().double().flatten()
    p[i] += 4 * ulp(p[i].item(), dt)
    return p.reshape(t.shape), i


def expect_fail(fn):
    with pytest.raises(AssertionError, match="out of bound"):
        fn()


def norm_case(dt, rms, res):
    torch.manual_seed(0)
    rows, D = 301, 264
    x = (torch.randn(rows, D) * 3 + 1).to(dt)
    w = torch.empty(D).uniform_(0.5, 1.5).to(dt)
    b = None if rms else torch.empty(D).uniform_(-0.5, 0.5).to(dt)
    dy = torch.randn(rows, D).to(dt)
    r = torch.randn(rows, D).to(dt) if res else None
    ref = R.norm_ref(x, w, b, 1e-5, rms, dy, r)
    t32 = R.norm_torch32(x, w, b, 1e-5, rms, dy, r)
    got = {k: (v.to(dt) if k not in ("mean", "rstd") else v) for k, v in t32.items()}
    return x, dy, r, ref, t32, got


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rms,res", [(False, False), (False, True), (True, True)])
def test_norm_bounds_pass_and_reject(dt, rms, res):
    x, dy, r, ref, t32, got = norm_case(dt, rms, res)
    R.check_norm("cpu norm", got, ref, dt, dt)
    for k in ("y", "dx") if dt != F32 else ():
        bad, _ = off_by_4ulp(got[k], ref[k], dt)
        expect_fail(lambda: R.check_norm("cpu norm", {k: bad}, ref, dt, dt))
    # a column sum that misses one row: the fp32 column sum of rows 1 .. of the fp32 terms
    xh = (x.double() - ref["mean"][:, None]) * ref["rstd"][:, None]
    terms = {"dgamma": dy.double() * xh}
    if not rms:
        terms["dbeta"] = dy.double()
        if res:
            terms["sres"], terms["sdx"] = r.double(), ref["dx"]
    for k, tm in terms.items():
        col = int(ref[k].abs().argmin())  # where the 16-bit ulp of the sum itself hides least
        row = int(tm[:, col].abs().argmax())
        bad = got[k].clone().double()
        bad[col] = (t32[k][col].double() - tm[row, col]).to(dt).double()
        expect_fail(lambda: R.check_norm("cpu norm", {k: bad}, ref, dt, dt))


def test_norm_large_offset_two_pass_passes_one_pass_fails():
    torch.manual_seed(0)
    x = 100 + 0.01 * torch.randn(37, 1024)
    ref = R.norm_ref(x, None, None, 1e-5, False)
    mean = x.mean(-1, keepdim=True)
    two = torch.rsqrt(((x - mean) ** 2).mean(-1) + 1e-5)
    one = torch.rsqrt((x * x).mean(-1) - mean[:, 0] ** 2 + 1e-5)
    R.check_norm("two-pass", {"rstd": two, "mean": mean[:, 0]}, ref, F32, F32)
    expect_fail(lambda: R.check_norm("one-pass", {"rstd": one}, ref, F32, F32))


@pytest.mark.parametrize("V", [8, 2056])
def test_xent_bounds_pass_and_reject(V):
    torch.manual_seed(0)
    x = torch.randn(33, V).to(BF16)
    t = torch.randint(0, V, (33,))
    t[5] = -100
    ref = R.xent_ref(x, t, -100, 3.0)
    o = R.xent_torch32(x, t, -100, 3.0)
    R.check_elem("cpu lse", o["lse"], ref["lse"], F32, R.C["xent_lse"], ref["lse_scale"])
    R.check_elem("cpu loss", o["loss"], ref["loss"], F32, R.C["xent_loss"], ref["loss_scale"])
    grad = o["grad"].to(BF16)
    R.check_elem("cpu grad", grad, ref["grad"], BF16, R.C["xent_grad"], ref["grad_scale"])
    bad, _ = off_by_4ulp(grad, ref["grad"], BF16)
    expect_fail(lambda: R.check_elem("cpu grad", bad, ref["grad"], BF16, R.C["xent_grad"], ref["grad_scale"]))
    # the softmax tail counts: zeros everywhere but the target column fail
    onehot = torch.zeros_like(ref["grad"]).scatter_(1, t.clamp_min(0)[:, None], 1.0).bool()
    tail0 = torch.where(onehot, grad.double(), torch.zeros_like(ref["grad"]))
    expect_fail(lambda: R.check_elem("cpu grad", tail0, ref["grad"], BF16, R.C["xent_grad"], ref["grad_scale"]))
    # a per-row lse 16 fp32 ulp off fails (the fp32 bound is 4 x torch's own error, about 6 ulp)
    bad = o["lse"].clone().double()
    bad[0] += 16 * ulp(bad[0].item(), F32)
    expect_fail(lambda: R.check_elem("cpu lse", bad, ref["lse"], F32, R.C["xent_lse"], ref["lse_scale"]))


@pytest.mark.parametrize("dt", DTYPES)
def test_elementwise_bounds_pass_and_reject(dt):
    torch.manual_seed(0)
    a, b, g = (3 * torch.randn(65, 264)).to(dt), torch.randn(65, 264).to(dt), torch.randn(65, 264).to(dt)
    ref, o = R.swiglu_ref(a, b, g), R.swiglu_torch32(a, b, g)
    for k, c in (("h", "swiglu"), ("da", "swiglu_da"), ("db", "swiglu_db")):
        got = o[k].to(dt)
        R.check_elem(f"cpu swiglu {k}", got, ref[k], dt, R.C[c], ref[k + "_scale"])
        if dt != F32:
            bad, _ = off_by_4ulp(got, ref[k], dt)
            expect_fail(lambda: R.check_elem(f"cpu swiglu {k}", bad, ref[k], dt, R.C[c], ref[k + "_scale"]))
    ref, o = R.gelu_ref(a, g), R.gelu_torch32(a, g)
    for k, c in (("y", "gelu"), ("dh", "dgelu")):
        got = o[k].to(dt)
        R.check_elem(f"cpu gelu {k}", got, ref[k], dt, R.C[c], ref[k + "_scale"])
        if dt != F32:
            bad, _ = off_by_4ulp(got, ref[k], dt)
            expect_fail(lambda: R.check_elem(f"cpu gelu {k}", bad, ref[k], dt, R.C[c], ref[k + "_scale"]))
    x = torch.randn(2, 19, 3, 64).to(dt)
    inv = 1.0 / (500000.0 ** (torch.arange(0, 64, 2).float() / 64))
    ang = torch.outer(torch.arange(80).float(), inv)
    pos = torch.randint(0, 80, (2, 19), dtype=torch.int32)
    for bw in (False, True):
        y, sc = R.rope_ref(x, ang.cos(), ang.sin(), pos, bw)
        got = R.rope_torch32(x, ang.cos(), ang.sin(), pos, bw).to(dt)
        R.check_elem("cpu rope", got, y, dt, R.C["rope"], sc)
        if dt != F32:
            bad, _ = off_by_4ulp(got, y, dt)
            expect_fail(lambda: R.check_elem("cpu rope", bad, y, dt, R.C["rope"], sc))


@pytest.mark.parametrize("dt", [BF16, F32])
def test_bias_colsum_bound_pass_and_reject(dt):
    torch.manual_seed(1)
    g, h = torch.randn(301, 64).to(dt), (2 * torch.randn(301, 64)).to(dt)
    ref = R.gelu_ref(h, g)
    dh32 = R.gelu_torch32(h, g)["dh"]
    for name, tm, t32 in (("plain", g.double(), g.float()), ("gelu", ref["dh"], dh32)):
        cref, cabs = tm.sum(0), tm.abs().sum(0)
        got = t32.sum(0).to(dt)
        R.check_colsum(f"cpu bias {name}", got, cref, cabs, dt, R.C["bias_col"])
        col = int(cref.abs().argmin())
        row = int(tm[:, col].abs().argmax())
        bad = got.clone().double()
        bad[col] = (t32.sum(0)[col].double() - tm[row, col]).to(dt).double()
        expect_fail(lambda: R.check_colsum(f"cpu bias {name}", bad, cref, cabs, dt, R.C["bias_col"]))


def test_nan_and_inf_never_pass():
    ref = torch.ones(4, dtype=torch.float64)
    for v in (float("nan"), float("inf")):
        got = torch.ones(4)
        got[2] = v
        expect_fail(lambda: R.check_elem("cpu nan", got, ref, BF16, 4.0))
