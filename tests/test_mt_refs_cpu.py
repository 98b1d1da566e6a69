"""Anchors tests/_mt_refs.py on the CPU, over the option tables, dtype pairs and inputs the GPU tests
(tests/test_multi_tensor_edges_gpu.py) use: the fp64 references are torch.optim's semantics (1e-12 of
torch.optim.SGD / Adam / AdamW run in fp64, step by step over 3 steps); fp32 torch stays within
C / 4 of them, which re-derives the constants table; the optimizers' CPU fallbacks stay within the
bounds; and ref_scale_copy's cast is bit-equal to an integer round-to-nearest-even.
"""
import itertools

import pytest
import torch

import _mt_refs as M
from distributeddataparallel_amd.optim import FusedAdam, FusedAdamW, FusedSGD

BF16, F16, F32, F64 = M.BF16, M.F16, M.F32, M.F64
ALL_PAIRS = [(p, g, False) for p, g in M.SGD_PAIRS] + [(p, g, True) for p, g in M.MASTER_PAIRS]
GS = torch.tensor([M.GRAD_SCALE])


def _covers_pairs(keys, table, legal=lambda d: True):
    vals = [sorted({r[i] for r in table}, key=float) for i in range(len(keys))]
    need = set()
    for r in itertools.product(*vals):
        if legal(dict(zip(keys, r))):
            need |= {(i, r[i], j, r[j]) for i in range(len(r)) for j in range(i + 1, len(r))}
    have = set()
    for r in table:
        assert legal(dict(zip(keys, r))), r
        have |= {(i, r[i], j, r[j]) for i in range(len(r)) for j in range(i + 1, len(r))}
    return need - have


def test_option_tables_cover_every_pair():
    legal = lambda d: not (d["nesterov"] and (d["momentum"] == 0 or d["dampening"] != 0))  # noqa: E731
    assert not _covers_pairs(M.SGD_KEYS, M.SGD_TABLE, legal)
    assert not _covers_pairs(M.ADAM_KEYS, M.ADAM_TABLE)
    assert {r[4] for r in M.ADAM_TABLE} == {1, 2, 1000}


def test_size_lists_sit_on_the_table_edges():
    assert len(M.sizes("t40")) == M.K_MAX_SEG and len(M.sizes("t41")) == M.K_MAX_SEG + 1
    s = M.sizes("t83")
    assert len(s) == 83 and s[0] == 0 and s[41] == 0 and s[-1] == 0
    assert sum(1 for n in s if n) == 2 * M.K_MAX_SEG and all(n for n in s[1:41] + s[42:82])
    assert set(M.N) <= set(M.sizes("set")) and not any(M.sizes("zeros"))


def _sgd_kw(row):
    o = M.sgd_opts(row)
    gs = GS if o.pop("gs") else None
    return dict(lr=M.SGD_LR, grad_scale=gs, **o)


def _adam_kw(row):
    o = M.adam_opts(row)
    gs = GS if o.pop("gs") else None
    zero = o.pop("zero_state")
    return dict(grad_scale=gs, **M.ADAM_HP, **o), zero


def _rel(a, b, scale):
    """max |a - b| relative to the magnitude of the terms that were added (an exp_avg or a parameter
    near zero is a cancellation: fp64 itself is only this good there)."""
    return ((a.double() - b.double()).abs() / scale.double().clamp_min(1e-300)).max().item() if a.numel() else 0.0


@pytest.mark.parametrize("row", M.SGD_TABLE)
def test_sgd_reference_is_torch_fp64_over_3_steps(row):
    kw = _sgd_kw(row)
    n = 2049
    p, _, g = M.opt_inputs(n, F32, F32, 0, False)
    buf = M.sgd_state(n, 0)
    w = torch.nn.Parameter(p.double().clone())
    tk = {k: v for k, v in kw.items() if k not in ("grad_scale", "first")}
    opt = torch.optim.SGD([w], foreach=False, **tk)
    if kw["momentum"] != 0 and not kw["first"]:
        opt.state[w]["momentum_buffer"] = buf.double().clone()
    cur_p, cur_buf, first = p.double(), buf.double(), kw["first"]
    for k in range(3):
        gk = g.double() * (k + 1) - 0.25 * k
        w.grad = gk * (1.0 if kw["grad_scale"] is None else kw["grad_scale"].double())
        opt.step()
        o = M.ref_sgd_step(cur_p, gk, cur_buf, **{**kw, "first": first})
        assert _rel(o["p"], w.detach(), o["p_scale"]) <= 1e-12
        if kw["momentum"] != 0:
            assert _rel(o["buf"], opt.state[w]["momentum_buffer"], o["buf_scale"]) <= 1e-12
            cur_buf = o["buf"]
        cur_p, first = o["p"], False


@pytest.mark.parametrize("row", M.ADAM_TABLE)
def test_adam_reference_is_torch_fp64_over_3_steps(row):
    kw, zero = _adam_kw(row)
    n = 2049
    p, _, g, m, v = M.adam_inputs(n, F32, F32, 0, False, zero)
    w = torch.nn.Parameter(p.double().clone())
    cls = torch.optim.AdamW if kw["decoupled"] else torch.optim.Adam
    opt = cls([w], lr=kw["lr"], betas=(kw["beta1"], kw["beta2"]), eps=kw["eps"], weight_decay=kw["weight_decay"],
              maximize=kw["maximize"], foreach=False)
    opt.state[w].update(step=torch.tensor(float(kw["step"] - 1)), exp_avg=m.double().clone(),
                        exp_avg_sq=v.double().clone())
    cp, cm, cv = p.double(), m.double(), v.double()
    for k in range(3):
        gk = g.double() * (k + 1) - 0.25 * k
        w.grad = gk * (1.0 if kw["grad_scale"] is None else kw["grad_scale"].double())
        opt.step()
        o = M.ref_adam_step(cp, gk, cm, cv, **{**kw, "step": kw["step"] + k})
        assert _rel(o["p"], w.detach(), o["p_scale"]) <= 1e-12
        assert _rel(o["m"], opt.state[w]["exp_avg"], o["m_scale"]) <= 1e-12
        assert _rel(o["v"], opt.state[w]["exp_avg_sq"], o["v_scale"]) <= 1e-12
        cp, cm, cv = o["p"], o["m"], o["v"]


def _sgd_cases():
    for pdt, gdt, master in ALL_PAIRS:
        for row in M.SGD_TABLE:
            for i, n in enumerate(M.sizes("set")):
                p, mw, g = M.opt_inputs(n, pdt, gdt, i, master)
                yield pdt, master, _sgd_kw(row), p, mw, g, M.sgd_state(n, i)


def _adam_cases():
    for pdt, gdt, master in ALL_PAIRS:
        for row in M.ADAM_TABLE:
            kw, zero = _adam_kw(row)
            for i, n in enumerate(M.sizes("set")):
                yield (pdt, master, kw) + M.adam_inputs(n, pdt, gdt, i, master, zero)


def test_fp32_torch_sgd_within_a_quarter_of_C():
    wp = wb = 0.0
    for pdt, master, kw, p, mw, g, buf in _sgd_cases():
        ref = M.ref_sgd_step(p, g, buf, master=mw, **kw)
        t32 = M.torch32_sgd_step(p, g, buf, master=mw, **kw)
        wp = max(wp, M.worst(t32["p"], ref["p"], ref["p_scale"]))
        if kw["momentum"] != 0:
            wb = max(wb, M.worst(t32["buf"], ref["buf"], ref["buf_scale"]))
    print(f"fp32 torch SGD: p {wp:.3f}, buf {wb:.3f} (x 2^-24 scale)")
    assert wp <= M.C["sgd_p"] / 4 and wb <= M.C["sgd_buf"] / 4


def test_fp32_torch_adam_within_a_quarter_of_C():
    w = {"p": 0.0, "m": 0.0, "v": 0.0}
    for pdt, master, kw, p, mw, g, m, v in _adam_cases():
        ref = M.ref_adam_step(p, g, m, v, master=mw, **kw)
        t32 = M.torch32_adam_step(p, g, m, v, master=mw, **kw)
        for k in w:
            w[k] = max(w[k], M.worst(t32[k], ref[k], ref[k + "_scale"]))
    print("fp32 torch Adam: " + ", ".join(f"{k} {x:.3f}" for k, x in w.items()) + " (x 2^-24 scale)")
    assert w["p"] <= M.C["adam_p"] / 4 and w["m"] <= M.C["adam_m"] / 4 and w["v"] <= M.C["adam_v"] / 4


def _norm_lists():
    for dt in (F32, BF16, F16):  # (fp64 lists are summed in fp64: a bound of their own, one fp32 rounding)
        for kind in M.LISTS:
            yield dt, kind, [M.norm_input(n, dt, i) for i, n in enumerate(M.sizes(kind))]


def test_fp32_torch_l2norm_within_a_quarter_of_C():
    w = 0.0
    for dt, kind, ts in _norm_lists():
        s, sc = M.ref_sumsq(ts)
        norm, nb, _, _ = M.norm_bounds(s, sc, 0.0, 1.0)
        got = torch.linalg.vector_norm(torch.cat([t.float() for t in ts]))
        w = max(w, ((got.double() - norm).abs() / nb.clamp_min(1e-300)).item() if norm > 0 else float(got != 0))
    print(f"fp32 torch vector_norm: {w:.3f} (x 2^-24 scale)")
    assert w <= M.C["l2norm"] / 4


def test_cpu_fallbacks_within_bounds():
    """FusedSGD._cpu_step and the CPU branch of FusedAdamW / FusedAdam, one step from explicit state."""
    for pdt, master, kw, p, mw, g, buf in _sgd_cases():
        ref = M.ref_sgd_step(p, g, buf, master=mw, **kw)
        w = (mw if master else p).clone()
        b = torch.full_like(buf, float("nan")) if kw["first"] else buf.clone()
        group = {k: kw[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize")}
        FusedSGD._cpu_step([w], [g], [b] if kw["momentum"] != 0 else [], group, kw["first"], kw["grad_scale"])
        M.check("cpu sgd p", w, ref["p"], M.elem_bound(ref["p"], w.dtype, M.C["sgd_p"], ref["p_scale"]))
        if kw["momentum"] != 0:
            M.check("cpu sgd buf", b, ref["buf"], M.elem_bound(ref["buf"], F32, M.C["sgd_buf"], ref["buf_scale"]))
    dummy = torch.nn.Parameter(torch.zeros(1))
    opts = {True: FusedAdamW([dummy]), False: FusedAdam([dummy])}
    for pdt, master, kw, p, mw, g, m, v in _adam_cases():
        ref = M.ref_adam_step(p, g, m, v, master=mw, **kw)
        q, mm, vv, ms = p.clone(), m.clone(), v.clone(), ([mw.clone()] if master else [])
        group = dict(betas=(kw["beta1"], kw["beta2"]), lr=kw["lr"], eps=kw["eps"], weight_decay=kw["weight_decay"],
                     maximize=kw["maximize"])
        opts[kw["decoupled"]]._cpu_step([q], [g], [mm], [vv], ms, group, kw["step"], kw["grad_scale"])
        if master:
            M.check("cpu adam master", ms[0], ref["p"], M.elem_bound(ref["p"], F32, M.C["adam_p"], ref["p_scale"]))
            assert torch.equal(q, ms[0].to(pdt))
        else:
            M.check("cpu adam p", q, ref["p"], M.elem_bound(ref["p"], pdt, M.C["adam_p"], ref["p_scale"]))
        M.check("cpu adam m", mm, ref["m"], M.elem_bound(ref["m"], F32, M.C["adam_m"], ref["m_scale"]))
        M.check("cpu adam v", vv, ref["v"], M.elem_bound(ref["v"], F32, M.C["adam_v"], ref["v_scale"]))


@pytest.mark.parametrize("scale", [1.0, 0.5, 1 / 3])
def test_ref_scale_copy_is_integer_rne(scale):
    x = torch.cat([M.copy_specials(BF16), M.copy_specials(F16), M.copy_specials(F32),
                   M.copy_input(4096, F32, BF16, 0), M.subnormal_input(512, 1)])
    prod = x * torch.tensor(scale, dtype=F32)  # the one fp32 multiply
    got = M.ref_scale_copy(x, BF16, scale).view(torch.int16).to(torch.int64) & 0xFFFF
    want = M.bf16_rne_bits(prod)
    nan = torch.isnan(prod)
    assert torch.equal(got[~nan], want[~nan]) and bool(((got[nan] & 0x7FFF) > 0x7F80).all())
    # the scale tensor multiplies sc in fp32 before the product
    st = torch.tensor([0.7])
    sc = torch.tensor(scale, dtype=F32) * st[0]
    got = M.ref_scale_copy(x, BF16, scale, st).view(torch.int16).to(torch.int64) & 0xFFFF
    nan = torch.isnan(x * sc)
    assert torch.equal(got[~nan], M.bf16_rne_bits(x * sc)[~nan])
    if scale == 1.0:  # ties go to the even neighbour, and the planted extremes behave as planted
        t = M.ref_scale_copy(M._f32_from_bits([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF]), BF16, 1.0)
        assert t.view(torch.int16).tolist() == [0x3F80, 0x3F82, 0x3F81, 0x3F80]
        h = M.copy_specials(F16)[-6:]  # +-max, +-the tie that rounds to inf, +-the value just below it
        r = M.ref_scale_copy(h, F16, 1.0).float()
        assert r.tolist() == [65504.0, -65504.0, float("inf"), float("-inf"), 65504.0, -65504.0]
        assert torch.isinf(M.ref_scale_copy(torch.tensor([1e5, -7e4]), F16, 1.0)).all()
        b = M.ref_scale_copy(M.copy_specials(BF16)[-6:], BF16, 1.0).float()
        big = torch.finfo(BF16).max
        assert b.tolist() == [big, -big, float("inf"), float("-inf"), big, -big]


def test_ref_scale_copy_fp64_keeps_fp64_precision():
    x = M.copy_input(64, F64, F64, 0)
    y = M.ref_scale_copy(x, F64, 1 / 3)
    assert y.dtype == F64 and torch.equal(y, x * (1 / 3))
    assert not torch.equal(y, (x.float() * torch.tensor(1 / 3, dtype=F32)).double())
    assert torch.equal(M.ref_scale_copy(x, F32, 1 / 3), (x * (1 / 3)).float())
