"""The 32-bit multi-tensor kernels (multi_tensor.hip) where they turn over: the lane vector switch,
one 2048-element iteration, the 8192-element chunk, Adam's whole-chunk path, the 40-segment table and
zero-numel tensors, 16-byte alignment (one misaligned pointer flips a whole launch to the scalar
template), every dtype pair, every optimizer option, and guard bands around every tensor.

The copy family is compared bit for bit with ``_mt_refs.ref_scale_copy``; the L2 norm and one
optimizer step from explicit state are compared per element with fp64 references under the bounds of
tests/_mt_refs.py (constants measured from fp32 torch on the CPU: tests/test_mt_refs_cpu.py).

Every tensor of a list is a slice of one arena with >= 64 bytes of guard on both sides. Output guards
hold a fixed bit pattern and must come back byte-identical; input guards hold NaN, so an over-read
shows up as a NaN norm or a set flag.
"""
import functools
import math

import pytest
import torch

import _mt_refs as M

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from distributeddataparallel_amd._native import load  # noqa: E402
from distributeddataparallel_amd.optim import (FusedAdam, FusedSGD, clip_grad_norm_,  # noqa: E402
                                               grad_norm)

DEV = "cuda"
BF16, F16, F32, F64 = M.BF16, M.F16, M.F32, M.F64
GUARD_BYTES = 64
PATTERN = 0xA5  # every guard byte of an output (a finite number in every float type)
ALIGN_MODES = ["aligned", "misaligned", "one"]
INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def guarded(numel, dtype, misalign_elems=0, nan_guard=False):
    """A one-tensor arena: ``.views[0]`` has ``numel`` elements, >= 64 guard bytes on both sides, and
    starts ``misalign_elems`` elements past a 16-byte boundary."""
    return Arena([numel], dtype, [misalign_elems], nan_guard)


class Arena:
    """The tensors of one list as slices of one allocation: [guard] t0 [guard] t1 ... [guard]. Tensor i
    starts ``mis[i]`` elements past a 16-byte boundary (1: element-aligned only)."""

    def __init__(self, sizes, dtype, mis=None, nan_guard=False):
        isz = torch.empty(0, dtype=dtype).element_size()
        ge, a = GUARD_BYTES // isz, max(16 // isz, 1)
        mis = [0] * len(sizes) if mis is None else mis
        self.sizes, self.starts, pos = list(sizes), [], ge
        for n, m in zip(sizes, mis):
            s = (pos + a - 1) // a * a + m
            self.starts.append(s)
            pos = s + n + ge
        self.base = torch.empty(pos + a, dtype=dtype, device=DEV)
        assert self.base.data_ptr() % 16 == 0
        if nan_guard:
            self.base.fill_(float("nan"))
        else:
            self.base.view(torch.uint8).fill_(PATTERN)
        self.views = [self.base[s:s + n] for s, n in zip(self.starts, sizes)]
        for v, m in zip(self.views, mis):
            assert v.numel() == 0 or (v.data_ptr() % 16 == 0) == (m == 0)
        idx = [torch.arange(s, s + n) for s, n in zip(self.starts, sizes)]
        self.idx = (torch.cat(idx) if idx else torch.zeros(0, dtype=torch.int64)).to(DEV)
        self.snap = None

    def set(self, flat):
        """Fill the tensors from one flat tensor (their concatenation) and remember every byte."""
        self.base[self.idx] = flat.to(device=DEV, dtype=self.base.dtype)
        self.snap = self.base.clone()
        return self

    def interior(self):
        return self.base[self.idx]

    def assert_unchanged(self, what):
        assert torch.equal(self.base.view(torch.uint8), self.snap.view(torch.uint8)), f"{what}: input was written"

    def assert_guards(self, what):
        g = self.base.clone()
        g[self.idx] = self.snap[self.idx]
        assert torch.equal(g.view(torch.uint8), self.snap.view(torch.uint8)), f"{what}: a guard byte changed"


def mis_for(mode, sizes, which=True):
    """Per-tensor misalignment of one arena. ``one``: only the last non-empty tensor, and only in the
    arena that passes ``which=True`` (so exactly one pointer of the launch is misaligned)."""
    if mode == "aligned":
        return [0] * len(sizes)
    if mode == "misaligned":
        return [1] * len(sizes)
    late = max((i for i, n in enumerate(sizes) if n), default=len(sizes) - 1)
    return [int(which and i == late) for i in range(len(sizes))]


def same_bits(got, exp, what):
    """Bit equality on every non-NaN element and equal NaN positions (payloads may differ)."""
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    nan = torch.isnan(exp)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    it = INT[got.element_size()]
    g, e = got.contiguous().view(it)[~nan], exp.contiguous().view(it)[~nan]
    if not torch.equal(g, e):
        i = int((g != e).nonzero()[0])
        raise AssertionError(f"{what}: {int((g != e).sum())} of {g.numel()} elements differ; first at non-NaN index "
                             f"{i}: got bits {int(g[i]):#x}, expected {int(e[i]):#x}")


@functools.lru_cache(maxsize=None)
def copy_flat(kind, src_dt, dst_dt):
    return torch.cat([M.copy_input(n, src_dt, dst_dt, i) for i, n in enumerate(M.sizes(kind))] + [torch.zeros(0, dtype=src_dt)])


def run_scale_copy(kind, src_dt, dst_dt, scale, with_st, mode, flat=None, what=""):
    C = load()
    sz = M.sizes(kind)
    src = Arena(sz, src_dt, mis_for(mode, sz, False), nan_guard=True).set(copy_flat(kind, src_dt, dst_dt) if flat is None else flat)
    dst = Arena(sz, dst_dt, mis_for(mode, sz, True)).set(torch.zeros(sum(sz)))
    st = torch.tensor([0.7], device=DEV) if with_st else None
    C.mt_scale_copy(src.views, dst.views, scale, st)
    tag = f"scale_copy {what}{kind} {src_dt}->{dst_dt} x{scale:.3g} st={with_st} {mode}"
    same_bits(dst.interior(), M.ref_scale_copy(src.interior(), dst_dt, scale, st), tag)
    dst.assert_guards(tag)
    src.assert_unchanged(tag)


# ---- copy family: bit-exact ----------------------------------------------------------------------
@pytest.mark.parametrize("dst_dt", [F32, BF16, F16])
@pytest.mark.parametrize("src_dt", [F32, BF16, F16])
def test_scale_copy_bit_exact(src_dt, dst_dt):
    for scale in (1.0, 0.5, 1 / 3):
        for with_st in (False, True):
            for mode in ALIGN_MODES:
                run_scale_copy("set", src_dt, dst_dt, scale, with_st, mode)
    for kind in ("one", "t40", "t41", "t83", "zeros"):
        for mode in ("aligned", "one"):
            run_scale_copy(kind, src_dt, dst_dt, 1 / 3, True, mode)


@pytest.mark.parametrize("dst_dt", [F32, BF16, F16])
def test_scale_copy_subnormals_match_torch_on_the_device(dst_dt):
    """fp32 subnormal inputs and results that are subnormal in the destination: the kernel neither
    flushes nor rounds them differently from torch's own fp32 multiply and cast on the same GPU."""
    sz = M.sizes("set")
    flat = torch.cat([M.subnormal_input(n, i) for i, n in enumerate(sz)])
    for scale in (1.0, 0.5, 1 / 3):
        for mode in ("aligned", "misaligned"):
            run_scale_copy("set", F32, dst_dt, scale, False, mode, flat, "subnormal ")
    x = flat.to(DEV)
    assert bool((x != 0).all()) and bool(((x * 0.5).to(dst_dt) != 0).any())  # the device's torch does not flush


@pytest.mark.parametrize("src_dt,dst_dt", [(F64, F64), (F64, F32), (F32, F64), (BF16, F64)])
def test_scale_copy_fp64_kernel(src_dt, dst_dt):
    """scale = 1/3 is not an fp32 number: an fp32-precision product fails on the fp64 outputs."""
    for with_st in (False, True):
        for mode in ALIGN_MODES:
            run_scale_copy("set", src_dt, dst_dt, 1 / 3, with_st, mode)
    run_scale_copy("t41", src_dt, dst_dt, 1 / 3, False, "aligned")
    run_scale_copy("t83", src_dt, dst_dt, 1 / 3, True, "aligned")
    if dst_dt == F64:
        x = copy_flat("set", src_dt, dst_dt).to(DEV)
        lo = (x.float() * torch.tensor(1 / 3, dtype=F32, device=DEV)).double()
        assert not torch.equal(lo, M.ref_scale_copy(x, F64, 1 / 3))


def _offsets(sz, rounded):
    offs, o = [], 3  # (3: even the first segment of the tight layout is misaligned)
    for n in sz:
        if rounded:
            o = (o + 15) // 16 * 16
        offs.append(o)
        o += n
    return offs, o + 5


@pytest.mark.parametrize("rounded", [False, True])
@pytest.mark.parametrize("t_dt,f_dt,scale", [(F32, BF16, 1 / 2), (F32, BF16, 1 / 3), (F32, F32, 1.0), (BF16, BF16, 1.0),
                                             (F16, F32, 1 / 3)])
def test_pack_and_unpack_as_ddp_uses_them(t_dt, f_dt, scale, rounded):
    """tensors -> flat (pack, scale = 1 / world) and flat -> tensors (unpack, with a scale), offsets
    packed tightly or rounded to 16 elements: the gaps between segments and flat's guards untouched."""
    C = load()
    for kind in ("set", "t41", "t83"):
        sz = M.sizes(kind)
        offs, total = _offsets(sz, rounded)
        tag = f"{kind} {t_dt}<->{f_dt} x{scale:.3g} rounded={rounded}"
        ts = Arena(sz, t_dt, nan_guard=True).set(copy_flat(kind, t_dt, f_dt))
        flat = guarded(total, f_dt).set(torch.zeros(total))
        flat.base.view(torch.uint8).fill_(PATTERN)  # the gaps hold the pattern too
        flat.snap = flat.base.clone()
        C.mt_pack(ts.views, flat.views[0], offs, scale)
        exp = flat.snap.clone()
        for v, o in zip(ts.views, offs):
            exp[flat.starts[0] + o: flat.starts[0] + o + v.numel()] = M.ref_scale_copy(v, f_dt, scale)
        same_bits(flat.base, exp, "pack " + tag)
        ts.assert_unchanged("pack " + tag)
        # and back, with the inverse scale, from a flat full of fresh values
        fsrc = guarded(total, f_dt, nan_guard=True).set(M.copy_input(total, f_dt, t_dt, 7))
        out = Arena(sz, t_dt).set(torch.zeros(sum(sz)))
        C.mt_unpack(fsrc.views[0], offs, out.views, 1 / scale)
        exp = out.snap.clone()
        for s, n, o in zip(out.starts, sz, offs):
            exp[s:s + n] = M.ref_scale_copy(fsrc.views[0][o:o + n], t_dt, 1 / scale)
        same_bits(out.base, exp, "unpack " + tag)
        fsrc.assert_unchanged("unpack " + tag)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_scale_copy_in_place_equals_out_of_place(dt):
    """mt_scale_copy(lst, lst, 1.0, coef), as clip_grad_norm_ calls it: src and dst alias exactly."""
    C = load()
    coef = torch.tensor([0.37], device=DEV)
    for kind, mode in [("set", m) for m in ALIGN_MODES] + [("t41", "aligned"), ("t83", "one")]:
        sz = M.sizes(kind)
        a = Arena(sz, dt, mis_for(mode, sz)).set(copy_flat(kind, dt, dt))
        b = Arena(sz, dt, mis_for(mode, sz)).set(copy_flat(kind, dt, dt))
        out = Arena(sz, dt, mis_for(mode, sz)).set(torch.zeros(sum(sz)))
        exp = M.ref_scale_copy(a.interior(), dt, 1.0, coef)
        C.mt_scale_copy(b.views, out.views, 1.0, coef)
        C.mt_scale_copy(a.views, a.views, 1.0, coef)
        same_bits(a.interior(), out.interior(), f"in place vs out of place {kind} {dt} {mode}")
        same_bits(a.interior(), exp, f"in place {kind} {dt} {mode}")
        a.assert_guards(f"in place {kind} {dt} {mode}")


def test_copy_bytes_many_segments_and_guards():
    C = load()
    sz = [n + (i % 3) for i, n in enumerate(M.sizes("t83"))]  # byte counts, odd ones among them
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (sum(sz),), dtype=torch.uint8, generator=g)
    for mode in ALIGN_MODES:
        src = Arena(sz, torch.uint8, mis_for(mode, sz, False)).set(data)
        dst = Arena(sz, torch.uint8, mis_for(mode, sz, True)).set(torch.zeros(sum(sz), dtype=torch.uint8))
        C.mt_copy_bytes(src.views, dst.views)
        assert torch.equal(dst.interior(), src.interior()), mode
        dst.assert_guards(f"copy_bytes {mode}")
        src.assert_unchanged(f"copy_bytes {mode}")


def test_scale_copy_equal_strides_copy_in_memory_order_and_different_strides_raise():
    C = load()
    a = torch.randn(4, 6, 5, 5, device=DEV).contiguous(memory_format=torch.channels_last)
    b = torch.empty_like(a, dtype=BF16)
    assert a.stride() == b.stride() and not a.is_contiguous()
    p = torch.randn(6, 5, 4, device=DEV).permute(2, 0, 1)
    q = torch.empty_like(p, dtype=F16)
    assert p.stride() == q.stride() and not p.is_contiguous()
    C.mt_scale_copy([a], [b], 1 / 3)
    C.mt_scale_copy([p], [q], 0.5)
    same_bits(b, M.ref_scale_copy(a, BF16, 1 / 3), "channels_last")
    same_bits(q, M.ref_scale_copy(p, F16, 0.5), "permuted")
    with pytest.raises(RuntimeError, match="identical memory order"):
        C.mt_scale_copy([a], [torch.empty(a.shape, device=DEV)], 1.0)
    with pytest.raises(RuntimeError, match="identical memory order"):
        C.mt_scale_copy([p], [a.new_empty(p.shape).permute(0, 2, 1).contiguous().permute(0, 2, 1)], 1.0)


# ---- L2 norm -------------------------------------------------------------------------------------
def norm_expect(ts, dt, max_norm):
    s, sc = M.ref_sumsq(ts)
    if dt == F64:  # summed in fp64: the norm is rounded to fp32 once; the coefficient adds max_norm's own
        # rounding to fp32, the sum's and the quotient's
        norm = s.sqrt()
        coef = (max_norm / (norm + 1e-6)).clamp(max=1.0) if max_norm > 0 else torch.ones_like(norm)
        n = sum(t.numel() for t in ts)
        return norm, (M.EPS32 + (n + 2) * 2.0 ** -53) * norm, coef, (4 * M.EPS32 * coef if max_norm > 0 else 0 * coef)
    return M.norm_bounds(s, sc, max_norm, M.C["l2norm"])


@functools.lru_cache(maxsize=None)
def norm_flat(kind, dt):
    return torch.cat([M.norm_input(n, dt, i) for i, n in enumerate(M.sizes(kind))] + [torch.zeros(0, dtype=dt)])


@pytest.mark.parametrize("dt", [F32, BF16, F16, F64])
def test_l2norm_lists_alignment_determinism(dt):
    C = load()
    for kind in M.LISTS:
        for mode in ALIGN_MODES:
            sz = M.sizes(kind)
            a = Arena(sz, dt, mis_for(mode, sz), nan_guard=True).set(norm_flat(kind, dt))
            out = torch.full((2,), float("nan"), device=DEV)
            out2 = torch.full((2,), float("nan"), device=DEV)
            C.mt_l2norm(a.views, out, 1.0)
            C.mt_l2norm(a.views, out2, 1.0)
            norm, nb, coef, cb = norm_expect(a.views, dt, 1.0)
            tag = f"l2norm {kind} {dt} {mode}"
            M.check(tag + " norm", out[0], norm, nb)
            M.check(tag + " coef", out[1], coef, cb)
            assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), tag + ": two calls differ"
            a.assert_unchanged(tag)
            if kind == "zeros":
                assert out.tolist() == [0.0, 1.0]
            if kind in ("t41", "t83") and mode == "aligned":  # the second launch's partials land after the first's
                one = guarded(sum(sz), dt, nan_guard=True).set(norm_flat(kind, dt))
                C.mt_l2norm(one.views, out2, 1.0)
                M.check(tag + " vs the concatenation", out[0], out2[0].double(), nb)


@pytest.mark.parametrize("dt", [F32, BF16, F64])
def test_l2norm_without_max_norm_gives_coefficient_one(dt):
    """max_norm = 0: out[1] is 1 (it was left unwritten), from mt_l2norm and from grad_norm on the
    single-dtype and on the mixed-dtype path; an empty list and a list of zero-numel tensors: [0, 1]."""
    C = load()
    ts = [M.norm_input(n, dt, i).to(DEV) for i, n in enumerate(M.sizes("set"))]
    for lst in (ts, [], [t[:0] for t in ts[:3]]):
        for max_norm in (0.0, 1.0):
            out = torch.full((2,), float("nan"), device=DEV)
            C.mt_l2norm(lst, out, max_norm)
            if max_norm == 0 or not sum(t.numel() for t in lst):
                assert out[1].item() == 1.0, (len(lst), max_norm, out.tolist())
            if not sum(t.numel() for t in lst):
                assert out[0].item() == 0.0

    def params(dts):
        ps = []
        for i, n in enumerate(M.sizes("set")):
            p = torch.nn.Parameter(torch.zeros(n, device=DEV, dtype=dts[i % len(dts)]))
            p.grad = M.norm_input(n, p.dtype, i).to(DEV)
            ps.append(p)
        return ps

    for dts in ([dt], [dt, F32 if dt != F32 else BF16]):
        ps = params(dts)
        for _ in range(3):  # whatever block the allocator hands grad_norm's torch.empty(2) held this before
            junk = torch.full((2,), 777.0, device=DEV)
            del junk
            nc = grad_norm(ps)
            s, sc = M.ref_sumsq([p.grad for p in ps])
            assert nc.shape == (2,) and nc[1].item() == 1.0, nc.tolist()
            M.check(f"grad_norm {dts}", nc[0], s.sqrt(), M.norm_bounds(s, sc, 0.0, M.C["l2norm"] + 4)[1])


def test_l2norm_fp64_beyond_fp32_range():
    """fp64 entries of magnitude 1e30: their squares overflow fp32, the norm does not. The fp64
    instantiation sums in fp64 (an fp32-range-only norm returned inf); out is fp32: one rounding."""
    C = load()
    sz = M.sizes("t41")
    flat = norm_flat("t41", F64).clone()
    flat[::97] *= 1e30
    flat[5] = -3e36
    for mode in ALIGN_MODES:
        a = Arena(sz, F64, mis_for(mode, sz), nan_guard=True).set(flat)
        out = torch.full((2,), float("nan"), device=DEV)
        C.mt_l2norm(a.views, out, 1e30)
        norm, nb, coef, cb = norm_expect(a.views, F64, 1e30)
        assert math.isfinite(norm.item()) and norm.item() > 1e36
        M.check(f"l2norm fp64 1e30 {mode} norm", out[0], norm, nb)
        M.check(f"l2norm fp64 1e30 {mode} coef", out[1], coef, cb)


@pytest.mark.parametrize("dts", [[BF16], [F32, BF16]])
def test_clip_grad_norm_low_precision_and_mixed(dts):
    ps, gs = [], []
    for i, n in enumerate(M.sizes("set")):
        p = torch.nn.Parameter(torch.zeros(n, device=DEV, dtype=dts[i % len(dts)]))
        p.grad = M.norm_input(n, p.dtype, i).to(DEV)
        gs.append(p.grad.clone())
        ps.append(p)
    max_norm = 2.5
    total = clip_grad_norm_(ps, max_norm)
    s, sc = M.ref_sumsq(gs)
    norm, nb, coef, cb = M.norm_bounds(s, sc, max_norm, M.C["l2norm"] + 4)  # (+ 4: the mixed path's torch ops)
    assert coef.item() < 1.0
    M.check(f"clip {dts} norm", total.reshape(()), norm, nb)
    for i, (p, g) in enumerate(zip(ps, gs)):
        ref = g.double() * coef
        # the coefficient's error carried, the fp32 product's rounding, the storage rounding
        M.check(f"clip {dts} grad {i}", p.grad, ref, M.elem_bound(ref, p.dtype, (cb / coef / M.EPS32).item() + 1))


# ---- non-finite check ----------------------------------------------------------------------------
def clean_flat(kind, dt):
    flat = norm_flat(kind, dt).clone()
    fi = torch.finfo(dt)
    flat[0], flat[1], flat[2], flat[3] = fi.max, -fi.max, fi.smallest_normal / 4, -fi.smallest_normal / 2
    flat[-1], flat[-2] = -fi.max, fi.smallest_normal / 8
    if dt == F64:
        flat[10], flat[11] = 1e300, -1e300  # finite, beyond fp32's range
    return flat


@pytest.mark.parametrize("dt", [F32, BF16, F16, F64])
def test_nonfinite_every_position_class(dt):
    C = load()
    sz = M.sizes("t41")
    assert sz[3] == 8193 and sz[20] == 8191 and sz[40] == 16385
    plants = [(0, 0), (3, 0), (3, 8192), (20, 8190), (40, 8191), (40, 8192), (40, 16384), (40, 16380)]
    for mode in ("aligned", "misaligned"):
        a = Arena(sz, dt, mis_for(mode, sz), nan_guard=True).set(clean_flat("t41", dt))
        flag = torch.ones(1, dtype=torch.int32, device=DEV)  # a stale 1 must be cleared
        C.mt_nonfinite(a.views, flag)
        assert flag.item() == 0, f"{dt} {mode}: clean input (largest finite values, subnormals, NaN guards) flagged"
        for val in (float("nan"), float("inf"), float("-inf")):
            for ti, k in plants:
                keep = a.views[ti][k].clone()
                a.views[ti][k] = val
                flag.fill_(0)
                C.mt_nonfinite(a.views, flag)
                assert flag.item() == 1, f"{dt} {mode}: {val} at tensor {ti} element {k} not seen"
                a.views[ti][k] = keep
        flag.fill_(1)
        C.mt_nonfinite(a.views, flag)
        assert flag.item() == 0
        a.assert_unchanged(f"nonfinite {dt} {mode}")
    for lst in ([], [a.views[0][:0]]):
        flag.fill_(1)
        C.mt_nonfinite(lst, flag)
        assert flag.item() == 0
    z = Arena(M.sizes("t83"), dt, nan_guard=True).set(clean_flat("t83", dt))
    flag.fill_(1)
    C.mt_nonfinite(z.views, flag)
    assert flag.item() == 0
    z.views[-2][-1] = float("inf")  # the last element of the last segment of the second table
    C.mt_nonfinite(z.views, flag)
    assert flag.item() == 1


# ---- fused SGD -----------------------------------------------------------------------------------
GS = None


def gs_tensor():
    global GS
    if GS is None:
        GS = torch.tensor([M.GRAD_SCALE], device=DEV)
    return GS


@functools.lru_cache(maxsize=None)
def sgd_flat(kind, pdt, gdt, master):
    ps, ms, gs, bs = [], [], [], []
    for i, n in enumerate(M.sizes(kind)):
        p, m, g = M.opt_inputs(n, pdt, gdt, i, master)
        ps.append(p), ms.append(m if master else p.float()), gs.append(g), bs.append(M.sgd_state(n, i))
    return torch.cat(ps), torch.cat(ms), torch.cat(gs), torch.cat(bs)


def run_sgd(kind, pdt, gdt, master, row, mode):
    C = load()
    o = M.sgd_opts(row)
    gs = gs_tensor() if o.pop("gs") else None
    kw = dict(lr=M.SGD_LR, grad_scale=gs, **o)
    sz = M.sizes(kind)
    fp, fm, fg, fb = sgd_flat(kind, pdt, gdt, master)
    mom = kw["momentum"] != 0
    P = Arena(sz, pdt, mis_for(mode, sz, False)).set(fp)
    G = Arena(sz, gdt, mis_for(mode, sz, True), nan_guard=True).set(fg)
    B = Arena(sz, F32, mis_for(mode, sz, False)).set(torch.full_like(fb, float("nan")) if kw["first"] else fb)
    W = Arena(sz, F32, mis_for(mode, sz, False)).set(fm) if master else None
    ref = M.ref_sgd_step(P.interior(), G.interior(), B.interior(), master=W.interior() if master else None, **kw)
    args = (kw["lr"], kw["momentum"], kw["dampening"], kw["weight_decay"], kw["nesterov"], kw["maximize"], kw["first"], gs)
    if master:
        C.fused_sgd_master(W.views, G.views, B.views if mom else [], P.views, *args)
    else:
        C.fused_sgd(P.views, G.views, B.views if mom else [], *args)
    tag = f"sgd {kind} p={pdt} g={gdt} master={master} {row} {mode}"
    if master:
        M.check(tag + " master", W.interior(), ref["p"], M.elem_bound(ref["p"], F32, M.C["sgd_p"], ref["p_scale"]))
        assert torch.equal(P.interior().view(torch.int16), W.interior().to(pdt).view(torch.int16)), \
            tag + ": model param is not the rounded master"
        W.assert_guards(tag + " master")
    else:
        M.check(tag + " p", P.interior(), ref["p"], M.elem_bound(ref["p"], pdt, M.C["sgd_p"], ref["p_scale"]))
    if mom:
        M.check(tag + " buf", B.interior(), ref["buf"], M.elem_bound(ref["buf"], F32, M.C["sgd_buf"], ref["buf_scale"]))
        B.assert_guards(tag + " buf")
    else:
        B.assert_unchanged(tag + " buf (no momentum)")
    P.assert_guards(tag + " p")
    G.assert_unchanged(tag + " grad")


@pytest.mark.parametrize("pdt,gdt", M.SGD_PAIRS)
def test_fused_sgd_one_step(pdt, gdt):
    for row in M.SGD_TABLE:
        for mode in ALIGN_MODES:
            run_sgd("set", pdt, gdt, False, row, mode)
    run_sgd("t41", pdt, gdt, False, M.SGD_TABLE[5], "aligned")
    run_sgd("t83", pdt, gdt, False, M.SGD_TABLE[4], "one")


@pytest.mark.parametrize("mdt,gdt", M.MASTER_PAIRS)
def test_fused_sgd_master_one_step(mdt, gdt):
    for row in M.SGD_TABLE:
        for mode in ALIGN_MODES:
            run_sgd("set", mdt, gdt, True, row, mode)
    run_sgd("t41", mdt, gdt, True, M.SGD_TABLE[5], "aligned")
    run_sgd("t83", mdt, gdt, True, M.SGD_TABLE[4], "one")


# ---- fused Adam / AdamW, 32-bit states -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adam_flat(kind, pdt, gdt, master, zero):
    cols = [[], [], [], [], []]
    for i, n in enumerate(M.sizes(kind)):
        p, m, g, ea, es = M.adam_inputs(n, pdt, gdt, i, master, zero)
        for c, x in zip(cols, (p, m if master else p.float(), g, ea, es)):
            c.append(x)
    return tuple(torch.cat(c) for c in cols)


def run_adam(kind, pdt, gdt, master, row, mode, sz=None, flats=None, bounded=True):
    C = load()
    o = M.adam_opts(row)
    gs = gs_tensor() if o.pop("gs") else None
    zero = o.pop("zero_state")
    kw = dict(grad_scale=gs, **M.ADAM_HP, **o)
    sz = M.sizes(kind) if sz is None else sz
    fp, fm, fg, fa, fs = adam_flat(kind, pdt, gdt, master, zero) if flats is None else flats
    P = Arena(sz, pdt, mis_for(mode, sz, False)).set(fp)
    G = Arena(sz, gdt, mis_for(mode, sz, False), nan_guard=True).set(fg)
    A = Arena(sz, F32, mis_for(mode, sz, True)).set(fa)
    S = Arena(sz, F32, mis_for(mode, sz, False)).set(fs)
    W = Arena(sz, F32, mis_for(mode, sz, False)).set(fm) if master else None
    ref = M.ref_adam_step(P.interior(), G.interior(), A.interior(), S.interior(),
                          master=W.interior() if master else None, **kw)
    C.fused_adam(P.views, G.views, A.views, S.views, W.views if master else [], kw["lr"], kw["beta1"], kw["beta2"],
                 kw["eps"], kw["weight_decay"], kw["step"], kw["decoupled"], kw["maximize"], gs)
    tag = f"adam {kind} p={pdt} g={gdt} master={master} {row} {mode}"
    if not bounded:
        return P, A, S
    if master:
        M.check(tag + " master", W.interior(), ref["p"], M.elem_bound(ref["p"], F32, M.C["adam_p"], ref["p_scale"]))
        assert torch.equal(P.interior().view(torch.int16), W.interior().to(pdt).view(torch.int16)), \
            tag + ": model param is not the rounded master"
        W.assert_guards(tag + " master")
    else:
        M.check(tag + " p", P.interior(), ref["p"], M.elem_bound(ref["p"], pdt, M.C["adam_p"], ref["p_scale"]))
    M.check(tag + " m", A.interior(), ref["m"], M.elem_bound(ref["m"], F32, M.C["adam_m"], ref["m_scale"]))
    M.check(tag + " v", S.interior(), ref["v"], M.elem_bound(ref["v"], F32, M.C["adam_v"], ref["v_scale"]))
    assert bool(torch.isfinite(P.interior()).all())
    for X, name in ((P, "p"), (A, "m"), (S, "v")):
        X.assert_guards(f"{tag} {name}")
    G.assert_unchanged(tag + " grad")
    return P, A, S


@pytest.mark.parametrize("pdt,gdt,master", [(p, g, False) for p, g in M.SGD_PAIRS] + [(p, g, True) for p, g in M.MASTER_PAIRS])
def test_fused_adam_one_step(pdt, gdt, master):
    for row in M.ADAM_TABLE:
        for mode in ALIGN_MODES:
            run_adam("set", pdt, gdt, master, row, mode)
    run_adam("t41", pdt, gdt, master, M.ADAM_TABLE[1], "aligned")
    run_adam("t83", pdt, gdt, master, M.ADAM_TABLE[2], "one")


def _paths_flats(sz, row):
    zero = M.adam_opts(row)["zero_state"]
    cols = [[], [], [], [], []]
    for i, n in enumerate(sz):
        p, _, g, ea, es = M.adam_inputs(n, F32, F32, i, False, zero)
        for c, x in zip(cols, (p, p, g, ea, es)):
            c.append(x)
    full = tuple(torch.cat(c) for c in cols)
    keep = torch.cat([torch.arange(n) < n - 1 for n in sz])
    return full, tuple(f[keep] for f in full), keep


@pytest.mark.parametrize("row", [M.ADAM_TABLE[1], M.ADAM_TABLE[2], M.ADAM_TABLE[5]])
def test_fused_adam_three_load_paths_agree_bitwise(row):
    """fp32 parameters: whole chunks of an aligned list take the all-loads-first path, its ragged last
    chunks the per-iteration vector path, the misaligned list the scalar path, and the same tensors cut
    one element short turn their whole last chunk into a ragged one. Each is within the bound (run_adam)
    and, the arithmetic being one function, they agree bit for bit on the elements they share."""
    sz = [8192, 16384, 16385, 3 * 8192 + 5]
    full, short, keep = _paths_flats(sz, row)
    runs = [("aligned", sz, full), ("misaligned", sz, full), ("aligned", [n - 1 for n in sz], short)]
    a, b, c = (run_adam("paths", F32, F32, False, row, mode, s, f, bounded=False) for mode, s, f in runs)
    k = keep.to(DEV)
    for x, y, z, name in zip(a, b, c, ("p", "m", "v")):
        same_bits(y.interior(), x.interior(), f"scalar vs vector paths, {name}")
        same_bits(z.interior(), x.interior()[k], f"per-iteration vs whole-chunk path, {name}")


@pytest.mark.parametrize("row", [M.ADAM_TABLE[1], M.ADAM_TABLE[2], M.ADAM_TABLE[5]])
def test_fused_adam_three_load_paths_within_bound(row):
    """The same three runs, each against the fp64 reference."""
    sz = [8192, 16384, 16385, 3 * 8192 + 5]
    run_adam("set", F32, F32, False, row, "aligned", sz, _paths_flats(sz, row)[0])
    run_adam("set", F32, F32, False, row, "misaligned", sz, _paths_flats(sz, row)[0])
    run_adam("set", F32, F32, False, row, "aligned", [n - 1 for n in sz], _paths_flats(sz, row)[1])


# ---- the optimizer classes' plumbing (what the kernel-level calls bypass) ------------------------
def _parity(make_fused, make_torch, ref_step, c):
    sz = [n for n in M.sizes("set") if n]
    ps = [torch.nn.Parameter(M.opt_inputs(n, F32, F32, i, False)[0].to(DEV)) for i, n in enumerate(sz)]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    o1, o2 = make_fused(ps), make_torch(qs)
    for k in range(3):
        pre = [q.detach().clone() for q in qs]
        state = [{n: v.clone() for n, v in o2.state[q].items() if torch.is_tensor(v)} for q in qs]
        for i, (p, q) in enumerate(zip(ps, qs)):
            g = M.opt_inputs(p.numel(), F32, F32, 100 * k + i, False)[2].to(DEV)
            p.grad, q.grad = g.clone(), g.clone()
        o1.step()
        o2.step()
        for i, (p, q) in enumerate(zip(ps, qs)):
            scale = ref_step(pre[i], q.grad, state[i], k)
            M.check(f"step {k} param {i}", p.detach(), q.detach().double(), 3 * c * M.EPS32 * scale)


def test_fused_sgd_class_dampening_maximize_matches_torch():
    kw = dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=1e-2, maximize=True)

    def scale(pre, g, st, k):
        return M.ref_sgd_step(pre, g, st.get("momentum_buffer"), nesterov=False, first=k == 0, **kw)["p_scale"]

    _parity(lambda ps: FusedSGD(ps, **kw), lambda qs: torch.optim.SGD(qs, foreach=False, **kw), scale, M.C["sgd_p"])


def test_fused_adam_class_coupled_decay_maximize_matches_torch():
    kw = dict(lr=1e-3, weight_decay=0.1, maximize=True)

    def scale(pre, g, st, k):
        z = torch.zeros_like(pre)
        return M.ref_adam_step(pre, g, st.get("exp_avg", z), st.get("exp_avg_sq", z), beta1=0.9, beta2=0.999, eps=1e-8,
                               step=k + 1, decoupled=False, **kw)["p_scale"]

    _parity(lambda ps: FusedAdam(ps, **kw), lambda qs: torch.optim.Adam(qs, foreach=False, **kw), scale, M.C["adam_p"])


# ---- replica checksum (the basics are in test_replicas_gpu.py) -----------------------------------
def _checksum_list():
    dts = [F32, BF16, F16, F64, torch.int32]
    out = []
    for i, n in enumerate(M.sizes("t83")):
        dt = dts[i % len(dts)]
        x = M.norm_input(n, F32, i)
        out.append((x * 100).to(dt) if dt == torch.int32 else x.to(dt))
    return out


def test_checksum_many_mixed_tensors():
    C = load()
    cpu = _checksum_list()
    a = [t.to(DEV) for t in cpu]
    b = [t.to(DEV).clone() for t in cpu]
    ca, cb = C.mt_checksum(a), C.mt_checksum(b)
    assert torch.equal(ca.view(torch.int64), cb.view(torch.int64)), "equal bytes in two allocations, different checksums"
    total = sum(t.double().sum() for t in cpu).item()
    mag = sum(t.double().abs().sum() for t in cpu).item()
    n = sum(t.numel() for t in cpu)
    print(f"checksum sum: |err| / bound = {abs(ca[0].item() - total) / (n * 2.0 ** -53 * mag):.3f}")
    assert abs(ca[0].item() - total) <= n * 2.0 ** -53 * mag
    sz = M.sizes("t83")
    big = max(range(len(sz)), key=lambda i: sz[i])
    assert sz[big] == 16385
    last_nz = max(i for i, m in enumerate(sz) if m)
    for ti, k in [(1, 0), (big, 0), (big, 8191), (big, 8192), (big, 16384), (big, 16380), (last_nz, sz[last_nz] - 1)]:
        t = b[ti]
        it = INT[t.element_size()]
        t.view(it)[k] ^= 1
        c2 = C.mt_checksum(b)
        assert c2[1].item() != ca[1].item() and c2[2].item() != ca[2].item(), f"bit flip at tensor {ti} element {k} not seen"
        t.view(it)[k] ^= 1
    assert torch.equal(C.mt_checksum(b).view(torch.int64), ca.view(torch.int64))
    i, j = [(x, y) for x in range(len(sz)) for y in range(x + 1, len(sz))
            if sz[x] == sz[y] == 2049 and b[x].dtype == b[y].dtype][0]
    assert b[i].shape == b[j].shape and not torch.equal(b[i], b[j])
    b[i], b[j] = b[j], b[i]
    c3 = C.mt_checksum(b)
    assert (c3[1].item(), c3[2].item()) != (ca[1].item(), ca[2].item()), "swapping two tensors went unseen"
