"""Anchors tests/_lw_refs.py on the CPU, over the lists, dtype pairs and option tables the GPU tests
(tests/test_layerwise_optim_gpu.py) use: with adaptation off the fp64 references are the Adam(W) / SGD
references of tests/_mt_refs.py (which are torch.optim's semantics); the plain fp32 torch
implementation stays within C / 4 of them, which re-derives the constants table, and stays inside
its own bounds on every single case.
"""
import functools
import itertools

import pytest
import torch

import _lw_refs as L
import _mt_refs as M

GS = torch.tensor([M.GRAD_SCALE])


def _uncovered(keys, table, legal=lambda d: True):
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
    assert not _uncovered(L.LAMB_KEYS, L.LAMB_TABLE)
    assert {r[0] for r in L.LAMB_TABLE} == {0.0, 0.1} and {r[5] for r in L.LAMB_TABLE} == {1, 2, 1000}
    assert any(not L.lamb_opts(r)[0]["adapt"] for r in L.LAMB_TABLE)
    legal = lambda d: not (d["nesterov"] and (d["momentum"] == 0 or d["dampening"] != 0))  # noqa: E731
    assert not _uncovered(L.LARS_KEYS, L.LARS_TABLE, legal)
    # the SGD_TABLE rows crossed with weight_decay and grad_scale
    rest = {r[:3] + r[4:5] + r[6:] for r in M.SGD_TABLE}
    assert {r[:3] + r[4:5] + r[6:] for r in L.LARS_TABLE} == rest and len(L.LARS_TABLE) == 4 * len(rest)
    for kind, i in L.LAMB_EXTRA:
        assert L.lamb_opts(L.LAMB_TABLE[i])[0]["adapt"]


def test_lists_hold_the_zero_tensors_and_the_table_edges():
    s = L.sizes("set")
    zp, zg = L.zero_roles("set")
    assert s[:-2] == M.sizes("set") and s[zp] == L.ZERO_P and s[zg] == L.ZERO_G
    ts = L.lamb_inputs("set", L.BF16, L.F32, True, False)
    assert not ts[zp][0].any() and not ts[zp][1].any() and ts[zp][2].any() and not ts[zg][2].any() and ts[zg][0].any()
    ts = L.lars_inputs("set", L.F32, L.BF16, False)
    assert not ts[zp][0].any() and ts[zp][1] is None and not ts[zg][2].any()
    assert L.sizes("t41") == M.sizes("t41") and L.sizes("t83") == M.sizes("t83")
    assert all(sum(L.sizes(k)) < 300_000 for k in L.LISTS)


def _rel(a, b, scale):
    return ((a.double() - b.double()).abs() / scale.double().clamp_min(1e-300)).max().item() if a.numel() else 0.0


@pytest.mark.parametrize("row", L.LAMB_TABLE)
def test_lamb_reference_without_adaptation_is_the_adamw_reference(row):
    kw, gs, zero = L.lamb_opts(row)
    gst = GS if gs else None
    bc = kw.pop("bias_correction")
    kw.pop("adapt")
    for n in (1, 9, 2049):
        p, _, g, m, v = M.adam_inputs(n, L.F32, L.F32, 0, False, zero)
        o = L.ref_lamb_step(p, g, m, v, grad_scale=gst, bias_correction=True, adapt=False, **kw)
        a = M.ref_adam_step(p, g, m, v, grad_scale=gst, decoupled=True, **kw)
        for k in ("p", "m", "v"):
            assert _rel(o[k], a[k], a[k + "_scale"]) <= 1e-12, (k, n)
        assert o["r"].item() == 1.0 and o["r_scale"].item() == 0.0
        if not bc:  # no bias correction: both corrections are 1, as at a step where beta^t has vanished
            o1 = L.ref_lamb_step(p, g, m, v, grad_scale=gst, bias_correction=False, adapt=False, **kw)
            a1 = M.ref_adam_step(p, g, m, v, grad_scale=gst, decoupled=True, **{**kw, "step": 10 ** 6})
            assert _rel(o1["p"], a1["p"], a1["p_scale"]) <= 1e-12


@pytest.mark.parametrize("row", L.LARS_TABLE)
def test_lars_reference_without_adaptation_is_the_sgd_reference(row):
    kw, gs = L.lars_opts(row)
    gst = GS if gs else None
    sk = {k: v for k, v in kw.items() if k not in ("trust_coefficient", "eps")}
    for n in (1, 9, 2049):
        p, _, g = M.opt_inputs(n, L.F32, L.F32, 0, False)
        buf = M.sgd_state(n, 0)
        o = L.ref_lars_step(p, g, buf, grad_scale=gst, adapt=False, **kw)
        a = M.ref_sgd_step(p, g, buf, grad_scale=gst, **sk)
        for k in a:
            assert torch.equal(o[k], a[k]), (k, n)
        assert o["r"].item() == 1.0 and o["r_scale"].item() == 0.0


def test_references_follow_the_written_formulas():
    """The adaptive part, by hand on a tiny tensor."""
    w, g = torch.tensor([3.0, -4.0]), torch.tensor([1.0, 2.0])
    z = torch.zeros(2)
    o = L.ref_lamb_step(w, g, z, z, lr=0.5, beta1=0.9, beta2=0.99, eps=0.0, weight_decay=0.0, step=1,
                        bias_correction=True, adapt=True, maximize=False)
    # m / bc1 = g, v / bc2 = g^2: u = sign(g), |u| = sqrt(2), |w| = 5
    assert abs(o["r"].item() - 5 / 2 ** 0.5) < 1e-12
    assert torch.allclose(o["p"], w.double() - 0.5 * (5 / 2 ** 0.5) * torch.tensor([1.0, 1.0], dtype=L.F64), atol=1e-12)
    o = L.ref_lars_step(w, g, z, lr=0.5, momentum=0.0, dampening=0.0, weight_decay=0.1, nesterov=False, maximize=True,
                        first=True, trust_coefficient=0.02, eps=1e-8, grad_scale=torch.tensor([-2.0]))
    gn = 2 * 5 ** 0.5
    lam = 0.02 * 5 / (gn + 0.5 + 1e-8)
    assert abs(o["r"].item() - lam) < 1e-15 and abs(o["g_norm"].item() - gn) < 1e-12
    d = lam * (g.double() * 2.0 + 0.1 * w.double())  # g' = g * (-2) * (-1)
    assert torch.allclose(o["p"], w.double() - 0.5 * d, atol=1e-14)
    for zero_w, zero_g in ((True, False), (False, True)):
        o = L.ref_lars_step(z if zero_w else w, z if zero_g else g, z, lr=0.5, momentum=0.0, dampening=0.0,
                            weight_decay=0.1, nesterov=False, maximize=False, first=True, trust_coefficient=0.02, eps=1e-8)
        assert o["r"].item() == 1.0
    o = L.ref_lamb_step(z, g, z, z, lr=0.5, beta1=0.9, beta2=0.99, eps=1e-6, weight_decay=0.1, step=1,
                        bias_correction=True, adapt=True, maximize=False)
    assert o["r"].item() == 1.0 and bool((o["p"] != 0).all())  # a zero-initialised tensor still trains


@functools.lru_cache(maxsize=None)
def _measure(which):
    """Worst error of the fp32 yardstick per output over every GPU case, in units of 2^-24 scale, and
    the worst ratio of its error to its own bound C."""
    worst, inside = {}, 0.0
    lamb = which == "lamb"
    table, extra = (L.LAMB_TABLE, L.LAMB_EXTRA) if lamb else (L.LARS_TABLE, L.LARS_EXTRA)
    for pdt, gdt, master in L.ALL_PAIRS:
        for kind, row in L.cases(table, extra):
            if lamb:
                kw, gs, zero = L.lamb_opts(row)
                tensors, ref_fn, t32_fn = L.lamb_inputs(kind, pdt, gdt, master, zero), L.ref_lamb_step, L.torch32_lamb_step
                outs = (("p", "p"), ("m", "m"), ("v", "v"), ("r", "r"))
            else:
                kw, gs = L.lars_opts(row)
                tensors, ref_fn, t32_fn = L.lars_inputs(kind, pdt, gdt, master), L.ref_lars_step, L.torch32_lars_step
                outs = (("p", "p"), ("r", "r")) + ((("buf", "buf"),) if kw["momentum"] != 0 else ())
            kw["grad_scale"] = GS if gs else None
            for p, mw, *rest in tensors:
                ref = ref_fn(p, *rest, master=mw, **kw)
                got = t32_fn(p, *rest, master=mw, **kw)
                for k, name in outs:
                    e = M.worst(got[k], ref[k], ref[k + "_scale"])
                    worst[name] = max(worst.get(name, 0.0), e)
                    inside = max(inside, e / L.C[f"{which}_{name}"])
    return worst, inside


@pytest.mark.parametrize("which", ["lamb", "lars"])
def test_fp32_yardstick_within_a_quarter_of_C_and_C_is_tight(which):
    worst, inside = _measure(which)
    print(f"fp32 torch {which}: " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()) + " (x 2^-24 scale)")
    for name, x in worst.items():
        c = L.C[f"{which}_{name}"]
        assert x <= c / 4, (name, x)
        assert x > c / 4 - 0.1 - 1e-9, f"{which}_{name}: C is 4 x {c / 4}, the measured maximum is {x:.3f}"
    assert inside <= 0.25
