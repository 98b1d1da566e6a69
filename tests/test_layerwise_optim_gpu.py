"""FusedLAMB / FusedLARS on the GPU (fused_lamb / fused_lars of multi_tensor.hip): one step from explicit
state against the fp64 references of tests/_lw_refs.py under the bounds measured there (fp32 torch on
the CPU: tests/test_lw_refs_cpu.py), on the lists where the kernels turn over (lane vector switch, one
iteration, one chunk and a fold over more than one partial, a ragged multi-chunk tensor, the 41st
tensor, zero-numel tensors at the table edges), every dtype pair, every option row, aligned and
misaligned pointers, inside guard bands; then the properties: zero tensors, NaN containment, bitwise
repeatability and independence of the list, FusedSGD equality, no host sync, graph capture.
"""
import functools

import pytest
import torch

import _lw_refs as L
import _mt_refs as M

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from test_multi_tensor_edges_gpu import ALIGN_MODES, Arena, mis_for, same_bits  # noqa: E402

from distributeddataparallel_amd._native import load  # noqa: E402
from distributeddataparallel_amd.optim import FusedLAMB, FusedLARS, FusedSGD, clip_grad_norm_  # noqa: E402

DEV = "cuda"
BF16, F16, F32 = M.BF16, M.F16, M.F32


@functools.lru_cache(maxsize=None)
def gs_tensor():
    return torch.tensor([M.GRAD_SCALE], device=DEV)


def _cat(ts, dtype):
    return torch.cat([t for t in ts] + [torch.zeros(0, dtype=dtype)])


@functools.lru_cache(maxsize=None)
def lamb_flat(kind, pdt, gdt, master, zero):
    ts = L.lamb_inputs(kind, pdt, gdt, master, zero)
    return (_cat([t[0] for t in ts], pdt), _cat([t[1] if master else t[0].float() for t in ts], F32),
            _cat([t[2] for t in ts], gdt), _cat([t[3] for t in ts], F32), _cat([t[4] for t in ts], F32))


@functools.lru_cache(maxsize=None)
def lars_flat(kind, pdt, gdt, master):
    ts = L.lars_inputs(kind, pdt, gdt, master)
    return (_cat([t[0] for t in ts], pdt), _cat([t[1] if master else t[0].float() for t in ts], F32),
            _cat([t[2] for t in ts], gdt), _cat([t[3] for t in ts], F32))


def check_ratios(tag, got, ref, c, sz):
    assert got.shape == (len(sz),) and got.dtype == F32
    L.check(tag + " ratios", got, ref["r"], L.ratio_bound(ref, c))
    for i, n in enumerate(sz):
        if n == 0:
            assert got[i].item() == 1.0, f"{tag}: the ratio of zero-numel tensor {i}"


def run_lamb(kind, pdt, gdt, master, row, mode):
    C = load()
    kw, gs, zero = L.lamb_opts(row)
    kw["grad_scale"] = gs_tensor() if gs else None
    sz = L.sizes(kind)
    fp, fm, fg, fa, fs = lamb_flat(kind, pdt, gdt, master, zero)
    P = Arena(sz, pdt, mis_for(mode, sz, False)).set(fp)
    G = Arena(sz, gdt, mis_for(mode, sz, False), nan_guard=True).set(fg)
    A = Arena(sz, F32, mis_for(mode, sz, True)).set(fa)
    S = Arena(sz, F32, mis_for(mode, sz, False)).set(fs)
    W = Arena(sz, F32, mis_for(mode, sz, False), nan_guard=True).set(fm) if master else None
    tensors = list(zip(P.views, W.views if master else [None] * len(sz), G.views, A.views, S.views))
    tag = f"lamb {kind} p={pdt} g={gdt} master={master} {row} {mode}"
    if not sum(sz):
        ratios = C.fused_lamb(P.views, G.views, A.views, S.views, W.views if master else [], kw["lr"], kw["beta1"],
                              kw["beta2"], kw["eps"], kw["weight_decay"], kw["step"], kw["bias_correction"],
                              kw["adapt"], kw["maximize"], kw["grad_scale"])
        assert ratios.tolist() == [1.0] * len(sz)
        return
    ref = L.ref_list(L.ref_lamb_step, tensors, **kw)
    ratios = C.fused_lamb(P.views, G.views, A.views, S.views, W.views if master else [], kw["lr"], kw["beta1"],
                          kw["beta2"], kw["eps"], kw["weight_decay"], kw["step"], kw["bias_correction"], kw["adapt"],
                          kw["maximize"], kw["grad_scale"])
    check_ratios(tag, ratios, ref, L.C["lamb_r"], sz)
    if master:
        L.check(tag + " master", W.interior(), ref["p"], L.elem_bound(ref["p"], F32, L.C["lamb_p"], ref["p_scale"]))
        assert torch.equal(P.interior().view(torch.int16), W.interior().to(pdt).view(torch.int16)), \
            tag + ": model param is not the rounded master"
        W.assert_guards(tag + " master")
    else:
        L.check(tag + " p", P.interior(), ref["p"], L.elem_bound(ref["p"], pdt, L.C["lamb_p"], ref["p_scale"]))
    L.check(tag + " m", A.interior(), ref["m"], L.elem_bound(ref["m"], F32, L.C["lamb_m"], ref["m_scale"]))
    L.check(tag + " v", S.interior(), ref["v"], L.elem_bound(ref["v"], F32, L.C["lamb_v"], ref["v_scale"]))
    assert bool(torch.isfinite(P.interior()).all()) and bool(torch.isfinite(ratios).all())
    for X, name in ((P, "p"), (A, "m"), (S, "v")):
        X.assert_guards(f"{tag} {name}")
    G.assert_unchanged(tag + " grad")
    zp, zg = L.zero_roles(kind)
    if zp is not None:  # an all-zero parameter: ratio 1, and it moves whenever its gradient or decay says so
        assert ratios[zp].item() == 1.0 and bool(P.views[zp].any()), tag
        if zero and kw["weight_decay"] == 0:  # an all-zero gradient on zero state: u = 0, ratio 1
            assert ratios[zg].item() == 1.0, tag


def run_lars(kind, pdt, gdt, master, row, mode):
    C = load()
    kw, gs = L.lars_opts(row)
    kw["grad_scale"] = gs_tensor() if gs else None
    mom = kw["momentum"] != 0
    sz = L.sizes(kind)
    fp, fm, fg, fb = lars_flat(kind, pdt, gdt, master)
    P = Arena(sz, pdt, mis_for(mode, sz, False)).set(fp)
    G = Arena(sz, gdt, mis_for(mode, sz, True), nan_guard=True).set(fg)
    B = Arena(sz, F32, mis_for(mode, sz, False)).set(torch.full_like(fb, float("nan")) if kw["first"] else fb)
    W = Arena(sz, F32, mis_for(mode, sz, False), nan_guard=True).set(fm) if master else None
    tensors = list(zip(P.views, W.views if master else [None] * len(sz), G.views, B.views))
    tag = f"lars {kind} p={pdt} g={gdt} master={master} {row} {mode}"
    args = (B.views if mom else [], W.views if master else [], kw["lr"], kw["momentum"], kw["dampening"],
            kw["weight_decay"], kw["nesterov"], kw["maximize"], kw["first"], kw["trust_coefficient"], kw["eps"],
            kw["grad_scale"])
    if not sum(sz):
        assert C.fused_lars(P.views, G.views, *args).tolist() == [1.0] * len(sz)
        return
    ref = L.ref_list(L.ref_lars_step, tensors, **kw)
    ratios = C.fused_lars(P.views, G.views, *args)
    check_ratios(tag, ratios, ref, L.C["lars_r"], sz)
    if master:
        L.check(tag + " master", W.interior(), ref["p"], L.elem_bound(ref["p"], F32, L.C["lars_p"], ref["p_scale"]))
        assert torch.equal(P.interior().view(torch.int16), W.interior().to(pdt).view(torch.int16)), \
            tag + ": model param is not the rounded master"
        W.assert_guards(tag + " master")
    else:
        L.check(tag + " p", P.interior(), ref["p"], L.elem_bound(ref["p"], pdt, L.C["lars_p"], ref["p_scale"]))
    if mom:
        L.check(tag + " buf", B.interior(), ref["buf"], L.elem_bound(ref["buf"], F32, L.C["lars_buf"], ref["buf_scale"]))
        B.assert_guards(tag + " buf")
    else:
        B.assert_unchanged(tag + " buf (no momentum)")
    assert bool(torch.isfinite(P.interior()).all()) and bool(torch.isfinite(ratios).all())
    P.assert_guards(tag + " p")
    G.assert_unchanged(tag + " grad")
    zp, zg = L.zero_roles(kind)
    if zp is not None:
        assert ratios[zp].item() == 1.0 and ratios[zg].item() == 1.0, tag


@pytest.mark.parametrize("pdt,gdt,master", L.ALL_PAIRS)
def test_fused_lamb_one_step(pdt, gdt, master):
    for kind, row in L.cases(L.LAMB_TABLE, L.LAMB_EXTRA):
        for mode in (ALIGN_MODES if kind == "set" else ("aligned", "one")):
            run_lamb(kind, pdt, gdt, master, row, mode)
    run_lamb("zeros", pdt, gdt, master, L.LAMB_TABLE[0], "aligned")


@pytest.mark.parametrize("pdt,gdt,master", L.ALL_PAIRS)
def test_fused_lars_one_step(pdt, gdt, master):
    for kind, row in L.cases(L.LARS_TABLE, L.LARS_EXTRA):
        for mode in (ALIGN_MODES if kind == "set" else ("aligned", "one")):
            run_lars(kind, pdt, gdt, master, row, mode)
    run_lars("zeros", pdt, gdt, master, L.LARS_TABLE[0], "aligned")


# ---- the optimizer classes ------------------------------------------------------------------------
def make_params(kind, pdt=F32, gdt=F32, seed=0):
    ps = []
    for i, n in enumerate(L.sizes(kind)):
        p, _, g = M.opt_inputs(n, pdt, gdt, seed + i, False)
        q = torch.nn.Parameter(p.to(DEV))
        q.grad = g.to(DEV)
        ps.append(q)
    return ps


def make_opt(name, ps, **kw):
    if name == "lamb":
        return FusedLAMB(ps, lr=1e-2, weight_decay=0.1, **kw)
    return FusedLARS(ps, lr=0.1, momentum=0.9, weight_decay=0.01, trust_coefficient=0.02, **kw)


def state_bits(opt, ps):
    out = []
    for p in ps:
        out.append(p.detach().clone())
        out += [v.clone() for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
    return out


def two_steps(name, ps, **kw):
    opt = make_opt(name, ps, **kw)
    opt.step()
    opt.step(grad_scale=gs_tensor())
    return opt


@pytest.mark.parametrize("name", ["lamb", "lars"])
def test_same_step_twice_is_bitwise_equal_and_a_tensor_alone_equals_it_in_the_list(name):
    a, b = make_params("t41", BF16, BF16), make_params("t41", BF16, BF16)
    oa, ob = two_steps(name, a, master_weights=True), two_steps(name, b, master_weights=True)
    for i, (x, y) in enumerate(zip(state_bits(oa, a), state_bits(ob, b))):
        same_bits(x, y, f"{name}: two runs, tensor {i}")
    ra, rb = oa.trust_ratios(), ob.trust_ratios()
    assert all(r.dim() == 0 and r.dtype == F32 and r.is_cuda for r in ra.values()) and len(ra) == len(a)
    same_bits(torch.stack([ra[p] for p in a]), torch.stack([rb[p] for p in b]), f"{name}: ratios of two runs")
    alone = make_params("t41", BF16, BF16)
    for i, p in enumerate(alone):  # every tensor in an optimizer of its own: another list, another table slot
        o = two_steps(name, [p], master_weights=True)
        for x, y in zip(state_bits(o, [p]), state_bits(oa, [a[i]])):
            same_bits(x, y, f"{name}: tensor {i} alone vs in the list")
        same_bits(o.trust_ratios()[p], ra[a[i]], f"{name}: ratio of tensor {i} alone vs in the list")


@pytest.mark.parametrize("name", ["lamb", "lars"])
def test_one_nan_gradient_element_poisons_exactly_its_own_tensor(name):
    ps = make_params("t41")
    bad = 40  # the 41st tensor: the second table, two chunks
    ps[bad].grad[8200] = float("nan")
    opt = make_opt(name, ps)
    opt.step()
    r = opt.trust_ratios()
    for i, p in enumerate(ps):
        if i == bad:
            assert bool(torch.isnan(p).all()), f"{name}: tensor {i} should be NaN everywhere"
            assert bool(torch.isnan(r[p]))
        else:
            assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(r[p])), f"{name}: tensor {i} caught the NaN"


@pytest.mark.parametrize("name", ["lamb", "lars"])
def test_input_guards_hold_nan_and_do_not_reach_a_norm(name):
    """Parameters and gradients between NaN guards, every size of the set, misaligned too: every ratio finite."""
    C = load()
    for mode in ALIGN_MODES:
        sz = L.sizes("set")
        fp, fm, fg, fa, fs = lamb_flat("set", F32, BF16, False, False)
        P = Arena(sz, F32, mis_for(mode, sz, True), nan_guard=True).set(fp)
        G = Arena(sz, BF16, mis_for(mode, sz, False), nan_guard=True).set(fg)
        A = Arena(sz, F32, mis_for(mode, sz, False), nan_guard=True).set(fa)
        S = Arena(sz, F32, mis_for(mode, sz, False), nan_guard=True).set(fs)
        if name == "lamb":
            r = C.fused_lamb(P.views, G.views, A.views, S.views, [], 1e-2, 0.9, 0.999, 1e-6, 0.1, 3, True, True, False, None)
        else:
            r = C.fused_lars(P.views, G.views, A.views, [], 0.1, 0.9, 0.0, 0.01, False, False, False, 0.02, 1e-8, None)
        assert bool(torch.isfinite(r).all()), (name, mode, r)
        assert bool(torch.isfinite(P.interior()).all())
        for X in (P, A) + ((S,) if name == "lamb" else ()):
            X.assert_guards(f"{name} {mode}")
        G.assert_unchanged(f"{name} {mode} grad")


# every place a load path or the fold turns over in a ragged three-chunk tensor, and its last element
ONE_HOT_AT = [0, 7, 8, 2047, 2048, 8191, 8192, 16383, 16384, 3 * 8192, 3 * 8192 + 4]


@pytest.mark.parametrize("name", ["lamb", "lars"])
def test_every_element_reaches_its_norm(name):
    """The fp64 comparison bounds a ratio by the error of a lane-serial fp32 sum (see _lw_refs.C): one
    dropped element among 24581 random ones would pass it. Here a tensor is zero but for one element of
    the parameter (3.0) and one of the gradient (4.0 for LARS, 1000 for LAMB), so both norms are exact in
    any summation order and a dropped element gives ratio 1 or a norm of 0. LARS: lam is
    tc 3 / (4 + wd 3 + eps), formed in fp64 from tc, wd and eps as fp32 kernel arguments (half an ulp
    each) and rounded to fp32 once: 2^-22 relative covers them. LAMB on zero state, step 1:
    m / bc1 = g and sqrt(v) / sqrt(bc2) = |g| up to 3 and 5 fp32 roundings, + eps (1e-9 relative), the
    quotient, the root of u^2 and |w| / |u|: 2^-20 relative covers all of them."""
    C = load()
    n, others = 3 * 8192 + 5, [9, 2049]
    sz = others + [n] + others
    for mode in ("aligned", "misaligned"):
        for k, j in zip(ONE_HOT_AT, reversed(ONE_HOT_AT)):
            w, g = torch.zeros(sum(sz)), torch.zeros(sum(sz))
            off = sum(others)
            w[off + k], g[off + j] = 3.0, 4.0 if name == "lars" else 1000.0
            w[:off], g[:off] = 1.0, 1.0  # the neighbours are ordinary tensors
            w[off + n:], g[off + n:] = 1.0, 1.0
            P = Arena(sz, F32, mis_for(mode, sz), nan_guard=True).set(w)
            G = Arena(sz, F32, mis_for(mode, sz), nan_guard=True).set(g)
            A = Arena(sz, F32, mis_for(mode, sz)).set(torch.zeros(sum(sz)))
            S = Arena(sz, F32, mis_for(mode, sz)).set(torch.zeros(sum(sz)))
            if name == "lars":
                r = C.fused_lars(P.views, G.views, A.views, [], 0.1, 0.9, 0.0, 0.01, False, False, True, 0.02, 1e-8, None)
                want, tol = 0.02 * 3.0 / (4.0 + 0.01 * 3.0 + 1e-8), 2.0 ** -22
            else:
                r = C.fused_lamb(P.views, G.views, A.views, S.views, [], 1e-2, 0.9, 0.999, 1e-6, 0.0, 1, True, True,
                                 False, None)
                want, tol = 3.0, 2.0 ** -20
            got = r[len(others)].item()
            assert abs(got - want) <= tol * want, f"{name} {mode}: one-hot w at {k}, g at {j}: ratio {got!r}, want {want!r}"


def test_layer_adaptation_off_is_bitwise_fused_sgd():
    for pdt, master in ((F32, False), (BF16, True)):
        a, b = make_params("set", pdt, pdt), make_params("set", pdt, pdt)
        kw = dict(lr=0.1, momentum=0.9, weight_decay=0.01, nesterov=True, master_weights=master)
        oa = FusedLARS([{"params": a[:5]}, {"params": a[5:], "layer_adaptation": False}], **kw)
        ob = FusedSGD(b[5:], **kw)
        for gs in (None, gs_tensor(), None):
            oa.step(grad_scale=gs)
            ob.step(grad_scale=gs)
        for x, y in zip(state_bits(oa, a[5:]), state_bits(ob, b[5:])):
            same_bits(x, y, f"layer_adaptation=False vs FusedSGD {pdt}")
        r = oa.trust_ratios()
        assert all(r[p].item() == 1.0 for p in a[5:]) and any(r[p].item() != 1.0 for p in a[:5])
        assert any(not torch.equal(x, y) for x, y in zip(a[:5], b[:5]) if x.numel())


def test_clip_coefficient_composes_as_grad_scale():
    for name in ("lamb", "lars"):
        a, b = make_params("set"), make_params("set")
        _, coef = clip_grad_norm_(a, 1.0, fused_into_optimizer=True)
        assert coef.shape == (1,) and coef.item() < 1.0
        for p in b:
            p.grad.mul_(coef)
        oa, ob = make_opt(name, a), make_opt(name, b)
        oa.step(grad_scale=coef)
        ob.step()
        for i, (x, y) in enumerate(zip(a, b)):  # the product is formed once either way, in another order
            torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-6, msg=f"{name} tensor {i}")


@pytest.mark.parametrize("name", ["lamb", "lars"])
def test_step_does_not_synchronise_with_the_host(name):
    ps = make_params("t41", BF16, BF16)
    opt = make_opt(name, ps, master_weights=True)
    opt.step()  # state creation
    gs = gs_tensor()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step(grad_scale=gs)
        opt.step_params(ps[:3], [p.grad for p in ps[:3]])
        r = opt.trust_ratios()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(r) == len(ps)


def test_step_params_equals_step():
    for name in ("lamb", "lars"):
        a, b = make_params("t41"), make_params("t41")
        oa, ob = make_opt(name, a), make_opt(name, b)
        for _ in range(2):
            oa.step()
            ob.step_params(b[:20], [p.grad for p in b[:20]])
            ob.step_params(b[20:], [p.grad for p in b[20:]])
        for x, y in zip(state_bits(oa, a), state_bits(ob, b)):
            same_bits(x, y, f"{name}: step_params vs step")


HIP_GRAPH_NODE_TYPE_KERNEL = 0  # hipGraphNodeTypeKernel


def test_lars_step_captured_in_a_graph_replays_the_eager_step_and_is_a_serial_chain():
    a, b = make_params("t41", BF16, BF16), make_params("t41", BF16, BF16)
    oa, ob = make_opt("lars", a, master_weights=True), make_opt("lars", b, master_weights=True)
    gs = gs_tensor()
    oa.step(grad_scale=gs)
    ob.step(grad_scale=gs)  # the eager warm-up: state exists, first = False from here on
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    saved = [t.clone() for t in state_bits(oa, a)]
    with torch.cuda.graph(graph):
        oa.step(grad_scale=gs)
    # capture does not run the kernels
    for x, y in zip(state_bits(oa, a), saved):
        same_bits(x, y, "capture changed a tensor")
    # the captured work: 41 tensors = 2 segment tables x (sums of squares, fold, update), one after the other
    types, edges = load().hip_graph_topology(int(graph.raw_cuda_graph()))
    print(f"captured LARS step: node types {types}, edges {edges}")
    assert len(types) == 6 and all(t == HIP_GRAPH_NODE_TYPE_KERNEL for t in types), types
    assert len(edges) == len(types) - 1, edges
    for i in range(len(types)):
        assert sum(1 for f, _ in edges if f == i) <= 1 and sum(1 for _, t in edges if t == i) <= 1, (i, edges)
    graph.replay()
    ob.step(grad_scale=gs)
    torch.cuda.synchronize()
    for x, y in zip(state_bits(oa, a), state_bits(ob, b)):
        same_bits(x, y, "graph replay vs eager step")
