"""``C.fused_adafactor`` (csrc/kernels/adafactor.hip) and ``FusedAdafactor`` on the GPU: one step from
explicit state against a plain fp64 implementation of the formulas, at the tile, vector, chunk and
table edges of the kernels. Inputs, reference and bound are in tests/_af_refs.py.
"""
import pytest
import torch

import distributeddataparallel_amd as xddp
from _af_refs import (BF16, CLIPS, F32, MIXED, OPTS, PAIRS, ROWS, TC, TR, VECS, close, kwargs, make, ref_step,
                      shapes_of_row, two_tables)
from distributeddataparallel_amd.optim import FusedAdafactor

pytestmark = pytest.mark.gpu
DEV = "cuda"


def guarded(x, pad):
    """``x`` on the GPU inside a buffer with ``pad`` sentinel elements on each side (pad 1: misaligned)."""
    buf = torch.full((x.numel() + 2 * pad,), 77.0, dtype=x.dtype, device=DEV)
    view = buf[pad:pad + x.numel()].view(x.shape)
    view.copy_(x)
    return view, buf


def gpu_step(tensors, opt, wdt, pad=8):
    """One fused step of a list of ``make`` tuples; returns per tensor the dict of device views after it."""
    C, kw, dev, bufs = xddp.native(), kwargs(opt, wdt), [], []
    for p, mw, g, st in tensors:
        d = {k: guarded(v, pad) for k, v in dict(st, p=p, g=g, **({"master": mw} if mw is not None else {})).items()}
        bufs += [b for _, b in d.values()]
        dev.append({k: v for k, (v, _) in d.items()})
    gs = kw.pop("gs")
    kw["grad_scale"] = None if gs is None else torch.tensor([gs], device=DEV)
    for matrix in (True, False):
        sel = [d for d in dev if (d["p"].dim() >= 2) == matrix]
        if sel:
            pick = lambda k: [d[k] for d in sel if k in d]  # noqa: E731
            C.fused_adafactor(pick("p"), pick("g"), pick("row_var"), pick("col_var"), pick("variance"),
                              pick("master"), **kw)
    torch.cuda.synchronize()
    for buf in bufs:  # the guard elements around every buffer are untouched
        assert bool((buf[:pad] == 77).all()) and bool((buf[buf.numel() - pad:] == 77).all())
    return dev


def check(tensors, opt, wdt, pad=8, clips=None):
    dev = gpu_step(tensors, opt, wdt, pad)
    for i, ((p, mw, g, st), d) in enumerate(zip(tensors, dev)):
        if p.numel() == 0:
            continue
        ref = ref_step(p if mw is None else mw, g, st, **kwargs(opt, wdt))
        if clips is not None:
            assert (ref["clip"] > 1) == clips, ref["clip"]
        assert torch.equal(d["g"].cpu(), g), "the gradient changed"
        close(d["p"], ref["w"], "w", f"param {i} {tuple(p.shape)}")
        if mw is not None:
            close(d["master"], ref["w"], "w", f"master {i}")
            assert torch.equal(d["p"], d["master"].to(p.dtype)), "the parameter is not the rounded master"
        for k in st:
            close(d[k], ref[k], k, f"{k} {i} {tuple(p.shape)}")
    return dev


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("o", [0, 1])
def test_tile_edges(r, o):
    check([make(s, i, F32, F32, False, OPTS[o]) for i, s in enumerate(shapes_of_row(r))], OPTS[o], F32)


@pytest.mark.parametrize("case", range(len(PAIRS)))
def test_dtype_pairs_and_options(case):
    (pdt, gdt, master), opt = PAIRS[case], OPTS[case % len(OPTS)]
    check([make(s, i, pdt, gdt, master, opt) for i, s in enumerate(MIXED + VECS)], opt, F32 if master else pdt)


@pytest.mark.parametrize("o", sorted(CLIPS))
def test_clip_regimes(o):
    for s in [(TR + 1, TC + 1), (8193,)]:
        check([make(s, 0, F32, BF16, False, OPTS[o])], OPTS[o], F32, clips=CLIPS[o])


def test_second_tables_and_alone_equals_list():
    tensors = two_tables(OPTS[2])
    dev = check(tensors, OPTS[2], F32)
    again = gpu_step(tensors, OPTS[2], F32)  # a step from the same state is bitwise repeatable
    alone = gpu_step([tensors[-1], tensors[42], tensors[83]], OPTS[2], F32)  # the last matrix, the last vector
    for a, b in list(zip(dev, again)) + [(dev[42], alone[1]), (dev[83], alone[2])]:
        assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("pdt,master", [(F32, False), (BF16, True)])
def test_misaligned_bases_take_the_scalar_path(pdt, master):
    shapes = [(TR + 1, 2 * TC + 8), (3, 9, 8), (8193,), (8,)]
    check([make(s, i, pdt, BF16, master, OPTS[2]) for i, s in enumerate(shapes)], OPTS[2], F32, pad=1)


@pytest.mark.parametrize("zero", ["row", "col", "grad", "param"])
@pytest.mark.parametrize("o", [0, 3])
def test_degenerate_inputs_stay_finite(zero, o):
    dev = check([make(s, i, F32, F32, False, OPTS[o], zero) for i, s in enumerate([(TR + 1, TC + 1), (2047,)])],
                OPTS[o], F32)
    assert all(bool(torch.isfinite(v).all()) for d in dev for v in d.values())


def test_nan_gradient_stays_in_its_tensor():
    tensors = [make(s, i, F32, F32, False, OPTS[0]) for i, s in enumerate([(70, 300), (70, 300), (9000,), (9000,)])]
    tensors[0][2][69, 299] = tensors[2][2][8999] = float("nan")
    dev = gpu_step(tensors, OPTS[0], F32)
    assert [bool(torch.isnan(d["p"]).all()) for d in dev] == [True, False, True, False]
    assert not any(bool(torch.isnan(d["p"]).any()) for d in dev[1::2])


def test_optimizer_step_has_no_host_sync_and_refuses_capture():
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda").to(BF16)) for s in [(3, 70, 40), (130, 264), (77,)]]
    opt = FusedAdafactor(ps, master_weights=True, weight_decay=0.01)
    for p in ps:
        p.grad = torch.randn_like(p)
    gs = torch.tensor([0.5], device="cuda")
    opt.step(grad_scale=gs)  # (allocates the states)
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step(grad_scale=gs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(p).all()) and torch.equal(p, opt.state[p]["master"].to(BF16)) for p in ps)
    before, graph = [p.detach().clone() for p in ps], torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(ps, before)) and opt.state[ps[0]]["step"] == 2
