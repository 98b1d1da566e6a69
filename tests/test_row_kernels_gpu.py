"""Row kernels where their loops turn over: LayerNorm / RMSNorm (layer_norm.hip), RoPE, SwiGLU,
GELU and bias_grad (transformer.hip), each against an fp64 reference of the same operation on the
same rounded inputs, per element (per column for column sums). Bounds and their measured constants:
tests/_row_refs.py; tests/test_row_refs_cpu.py shows fp32 torch meeting them and small
perturbations missing them.
"""
import pytest
import torch

import _row_refs as R

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from distributeddataparallel_amd._native import load  # noqa: E402
from distributeddataparallel_amd.ops.layer_norm import rms_norm_with_skip  # noqa: E402

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def rows_per_pass():
    """Rows one pass of ln_backward's grid covers: 2 blocks per CU, 4 rows per block."""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4


def norm_inputs(rows, D, dt, wdt, rms, res):
    torch.manual_seed(0)
    x = (torch.randn(rows, D, device=DEV) * 3 + 1).to(dt)
    w = torch.empty(D, device=DEV).uniform_(0.5, 1.5).to(wdt)
    b = None if rms else torch.empty(D, device=DEV).uniform_(-0.5, 0.5).to(wdt)
    dy = torch.randn(rows, D, device=DEV).to(dt)
    r = torch.randn(rows, D, device=DEV).to(dt) if res else None
    return x, w, b, dy, r


def run_norm(rows, D, dt, wdt, rms, res, add_bias=False):
    """ln_forward + ln_backward called directly, every output against fp64 autograd of
    norm(x) . dy (+ x . res): y, mean, rstd, dx, dgamma, dbeta and, LayerNorm with res, the two sums."""
    C = load()
    x, w, b, dy, r = norm_inputs(rows, D, dt, wdt, rms, res)
    eps = 1e-5
    ab = torch.randn(D, device=DEV).to(wdt) if add_bias else None
    y, mean, rstd, xb = C.ln_forward(x, w, b, eps, rms, ab)
    dx, dg, db, sres, sdx = C.ln_backward(dy, x, w, None if rms else mean, rstd, rms, True, not rms, r)
    ref = R.norm_ref(x, w, b, eps, rms, dy, r)
    tag = f"{'rms' if rms else 'ln'} {rows}x{D} {dt}/{wdt} res={res}"
    got = {"y": y, "rstd": rstd, "dx": dx, "dgamma": dg}
    if not rms:
        got.update(mean=mean, dbeta=db)
        if res:
            got.update(sres=sres, sdx=sdx)
    else:
        assert sres is None or not sres.numel()
    assert dg.dtype == wdt and dx.dtype == dt
    R.check_norm(tag, got, ref, dt, wdt)
    if add_bias and wdt == dt:  # exact: x + b rounded once
        assert torch.equal(xb, (x.double() + ab.double()).to(dt)), f"{tag}: xb is not (x + b) rounded once"
    elif add_bias:  # an fp32 b: the fp32 sum is rounded before the store rounds it again (one fp32 rounding)
        s = x.double() + ab.double()
        R.check_elem(f"{tag} xb", xb, s, dt, 1.0, x.double().abs() + ab.double().abs())


# Narrow rows (D <= 1024), 3 passes + 5 rows: in the bf16 residual form all three slots run, s0 is
# refilled, the look-ahead clamps to the last row and the last block is ragged; fp32 / fp16 take
# the generic pipelined loop (the row + step prefetch and its register copy).
@pytest.mark.parametrize("dt", [BF16, F32, F16])
@pytest.mark.parametrize("D", [512, 1024])
def test_layernorm_narrow_residual_form(D, dt):
    run_norm(3 * rows_per_pass() + 5, D, dt, dt, False, True)


@pytest.mark.parametrize("dt", [BF16, F32, F16])
@pytest.mark.parametrize("D", [512, 1024])
def test_rmsnorm_narrow_with_skip(D, dt):
    """rms_norm_with_skip (the skip's gradient added inside the backward kernel: RES without the
    sums) against fp64 autograd of rms_norm(x) . dy + x . dskip: dx and dgamma."""
    rows = 3 * rows_per_pass() + 5
    x, w, _, dy, r = norm_inputs(rows, D, dt, dt, True, True)
    x1, w1 = x.clone().requires_grad_(), w.clone().requires_grad_()
    y, skip = rms_norm_with_skip(x1, (D,), w1, 1e-5)
    torch.autograd.backward([y, skip], [dy, r])
    ref = R.norm_ref(x, w, None, 1e-5, True, dy, r)
    R.check_norm(f"rms_skip {rows}x{D} {dt}", {"y": y.detach(), "dx": x1.grad, "dgamma": w1.grad}, ref, dt, dt)


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("D", [512, 1024])
def test_norm_narrow_no_residual(D, rms):
    run_norm(3 * rows_per_pass() + 5, D, BF16, BF16, rms, False)


# Wide rows (D > 1024): the one-row-at-a-time loop makes a third, ragged trip; dgamma / dbeta
# accumulate in registers across the trips.
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("D", [2048, 4096])
def test_norm_wide_rows(D, rms, res, dt):
    run_norm(2 * rows_per_pass() + 3, D, dt, dt, rms, res)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("rms", [False, True])
def test_norm_widest(rms, dt):
    run_norm(9, 8192, dt, dt, rms, False, add_bias=not rms)


# D where vectors-per-lane is rounded up to a power of two (NV = 2, 4, 4, 8, 16 for 520 .. 5120)
# and whole k slots, or most of one, fail c < D; with mean / rstd and the add_bias output.
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("D", [520, 1032, 1536, 3072, 5120])
def test_norm_masked_vector_slots(D, rms, dt):
    run_norm(37, D, dt, dt, rms, False, add_bias=True)


@pytest.mark.parametrize("D", [64, 1024, 2048, 4096])
def test_norm_forward_extras_each_nv(D):
    """mean, rstd and the exact add_bias output at NV = 1, 2, 4, 8 (16: test_norm_widest)."""
    run_norm(37, D, BF16, BF16, False, True, add_bias=True)


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("D", [1024, 4096])
def test_norm_bf16_activations_fp32_weights(D, rms):
    """T != W: dgamma / dbeta come back fp32 and get the fp32 bound."""
    run_norm(37, D, BF16, F32, rms, False, add_bias=True)


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("D", [1024, 4096])
def test_norm_large_common_offset(D, rms):
    """x = 100 +- 0.01 in fp32: the two-pass variance must not cancel (forward outputs)."""
    C = load()
    torch.manual_seed(0)
    x = 100 + 0.01 * torch.randn(37, D, device=DEV)
    w = torch.empty(D, device=DEV).uniform_(0.5, 1.5)
    b = None if rms else torch.empty(D, device=DEV).uniform_(-0.5, 0.5)
    y, mean, rstd, _ = C.ln_forward(x, w, b, 1e-5, rms)
    ref = R.norm_ref(x, w, b, 1e-5, rms)
    got = {"y": y, "rstd": rstd}
    if not rms:
        got["mean"] = mean
    R.check_norm(f"offset rms={rms} D={D}", got, ref, F32, F32)


# ---- RoPE ------------------------------------------------------------------------------------
def rope_tables(n, Dh):
    inv = 1.0 / (500000.0 ** (torch.arange(0, Dh, 2, device=DEV).float() / Dh))
    ang = torch.outer(torch.arange(n, device=DEV).float(), inv)
    return ang.cos().contiguous(), ang.sin().contiguous()


def check_rope(tag, x, cos, sin, pos):
    C = load()
    for bw in (False, True):
        got = C.rope(x, cos, sin, bw, pos)
        ref, sc = R.rope_ref(x, cos, sin, pos, bw)
        R.check_elem(f"rope {tag} bwd={bw} pos={pos is not None}", got, ref, x.dtype, R.C["rope"], sc)


def test_rope_grid_stride_wrap():
    """[1, 2050, 32, 128] bf16 = 1,049,600 vectors: 1024 more than the grid's 4096 x 256 threads, so
    the first 1024 threads make a second trip; with positions that differ from arange there."""
    torch.manual_seed(0)
    B, S, H, Dh = 1, 2050, 32, 128
    assert B * S * H * Dh // 8 > 4096 * 256
    x = torch.randn(B, S, H, Dh, device=DEV).to(BF16)
    cos, sin = rope_tables(S, Dh)
    check_rope("wrap", x, cos, sin, None)
    pos = torch.arange(S, device=DEV, dtype=torch.int32)[None].contiguous()
    pos[0, 2040:] = torch.tensor([7, 0, 1999, 3, 2049, 11, 5, 1024, 2, 1], device=DEV, dtype=torch.int32)
    check_rope("wrap", x, cos, sin, pos)


@pytest.mark.parametrize("dt", [BF16, F16, F32])
@pytest.mark.parametrize("shape", [(2, 13, 1, 8), (3, 5, 3, 64), (2, 130, 4, 128)])
def test_rope_dtypes_small(shape, dt):
    """Dh = 8 is one vector per row, H = 1 one row per token."""
    torch.manual_seed(0)
    B, S, H, Dh = shape
    x = torch.randn(shape, device=DEV).to(dt)
    cos, sin = rope_tables(4 * S, Dh)
    check_rope(f"{shape} {dt}", x, cos, sin, None)
    pos = torch.randint(0, 4 * S, (B, S), device=DEV, dtype=torch.int32)
    check_rope(f"{shape} {dt}", x, cos, sin, pos)


# ---- SwiGLU / GELU -----------------------------------------------------------------------------
def check_swiglu(tag, a, b, g, where=None):
    C = load()
    dt = a.dtype
    h = C.swiglu_forward(a, b)
    da, db = C.swiglu_backward(g, a, b)
    ref = R.swiglu_ref(a, b, g)
    for name, got, k, c in (("h", h, "h", "swiglu"), ("da", da, "da", "swiglu_da"), ("db", db, "db", "swiglu_db")):
        r, bound = ref[k], R.elem_bound(ref[k], dt, R.C[c], ref[k + "_scale"])
        if where is not None:  # only where the storage type holds the reference as a finite number
            m = R.finite_in(r, dt)
            assert m.float().mean() > 0.5
            got, r, bound = got[m], r[m], bound[m]
        R.check(f"swiglu {tag} {name}", got, r, bound)


def check_gelu(tag, x, g, where=None):
    C = load()
    dt = x.dtype
    y = C.gelu_forward(x)
    _, dh = C.bias_grad(g, x, torch.zeros(x.shape[-1], device=DEV, dtype=dt))
    ref = R.gelu_ref(x, g)
    for name, got, k, c in (("y", y, "y", "gelu"), ("dh", dh, "dh", "dgelu")):
        r, bound = ref[k], R.elem_bound(ref[k], dt, R.C[c], ref[k + "_scale"])
        if where is not None:
            m = R.finite_in(r, dt)
            got, r, bound = got[m], r[m], bound[m]
        R.check(f"gelu {tag} {name}", got, r, bound)


def test_swiglu_gelu_grid_stride_wrap():
    """[1025, 8192] bf16 = 1,049,600 vectors, 1024 past the grid cap: every element of swiglu
    forward, da, db and of gelu_forward."""
    torch.manual_seed(0)
    a = (2 * torch.randn(1025, 8192, device=DEV)).to(BF16)
    b = torch.randn(1025, 8192, device=DEV).to(BF16)
    g = torch.randn(1025, 8192, device=DEV).to(BF16)
    assert a.numel() // 8 > 4096 * 256
    check_swiglu("wrap", a, b, g)
    y = load().gelu_forward(a)
    ref = R.gelu_ref(a)
    R.check_elem("gelu wrap y", y, ref["y"], BF16, R.C["gelu"], ref["y_scale"])


@pytest.mark.parametrize("dt", [BF16, F16, F32])
@pytest.mark.parametrize("shape", [(1, 8), (7, 24), (513, 1032)])
def test_swiglu_gelu_dtypes_small(shape, dt):
    torch.manual_seed(0)
    a = (3 * torch.randn(shape, device=DEV)).to(dt)
    b = torch.randn(shape, device=DEV).to(dt)
    g = torch.randn(shape, device=DEV).to(dt)
    check_swiglu(f"{shape} {dt}", a, b, g)
    check_gelu(f"{shape} {dt}", a, g)


def test_swiglu_gelu_saturating_values():
    """a over 0, +-tiny, +-20, +-88, +-100 (where __expf(-a) overflows to inf) and the largest
    finite bf16, against b and g of mixed sign and size: forward, da and db each against fp64, in
    bf16. Every element whose reference the type can hold (which covers every element where fp32
    torch stays finite) must be finite and in bound: no NaN from inf / inf or 0 x inf."""
    big = torch.finfo(BF16).max
    av = [0.0, 1e-30, -1e-30, 1e-3, -1e-3, 0.5, -0.5, 3.0, -3.0, 20.0, -20.0, 60.0, -60.0, 88.0, -88.0, 89.0, -89.0,
          100.0, -100.0, 104.0, -104.0, 1e4, -1e4, 1e30, -1e30, big, -big]
    bv = [1.0, -1.0, 0.37, -2.5, 1e-3, -300.0, 0.0, 1e30]
    gv = [1.0, -0.5, 7.0, -1e-2]
    a, b, g = torch.meshgrid(torch.tensor(av), torch.tensor(bv), torch.tensor(gv), indexing="ij")
    a, b, g = (t.reshape(-1, 8).to(DEV).to(BF16).contiguous() for t in (a, b, g))
    check_swiglu("sweep", a, b, g, where=True)
    check_gelu("sweep", a, g, where=True)


# ---- bias_grad ---------------------------------------------------------------------------------
# rgroups = min(rows, ceil(524288 / (N / 8))): (3001, 4096) -> 1024 partial rows, 3 rows per thread;
# (20000, 64) -> 20000 partial rows into colsum_partials (its 8-deep unrolled loop and the tail);
# (5, 8) -> one thread per row; (8229, 1024) -> 4096 row groups, 2 or 3 rows per thread.
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("rows,N", [(3001, 4096), (20000, 64), (5, 8), (8229, 1024)])
def test_bias_grad_per_column(rows, N, dt):
    C = load()
    torch.manual_seed(1)
    g = torch.randn(rows, N, device=DEV).to(dt)
    h = (2 * torch.randn(rows, N, device=DEV)).to(dt)
    bias = torch.zeros(N, device=DEV, dtype=dt)
    db, none = C.bias_grad(g, None, bias)
    assert none is None or not none.numel()
    g64 = g.double()
    R.check_colsum(f"bias_grad {rows}x{N} {dt} plain", db, g64.sum(0), g64.abs().sum(0), dt, R.C["bias_col"])
    db1, dh = C.bias_grad(g, h, bias)
    ref = R.gelu_ref(h, g)
    R.check_elem(f"bias_grad {rows}x{N} {dt} dh", dh, ref["dh"], dt, R.C["dgelu"], ref["dh_scale"])
    # the kernel sums its fp32 dh, not the stored one: the column terms are the reference's
    R.check_colsum(f"bias_grad {rows}x{N} {dt} gelu", db1, ref["dh"].sum(0), ref["dh"].abs().sum(0), dt,
                   R.C["bias_col"])
