"""FusedLAMB / FusedLARS without a GPU: the CPU path against the fp64 references of tests/_lw_refs.py
over three consecutive steps, state-dict round trips with bf16 parameters, a ``layer_adaptation=False``
group against FusedSGD, and every error path.
"""
import copy

import pytest
import torch

import _lw_refs as L
import _mt_refs as M
from distributeddataparallel_amd.optim import FusedLAMB, FusedLARS, FusedSGD

BF16, F16, F32 = M.BF16, M.F16, M.F32
SIZES = [1, 9, 2049, 8193, 7]  # the last one starts from an all-zero parameter
GS = torch.tensor([M.GRAD_SCALE])


def _params(pdt, gdt, seed=0):
    ps = []
    for i, n in enumerate(SIZES):
        p, _, _ = M.opt_inputs(n, F32, gdt, seed + i, False)
        if i == len(SIZES) - 1:
            p = torch.zeros_like(p)
        ps.append(torch.nn.Parameter(p.to(pdt)))
    return ps


def _grads(ps, gdt, k):
    for i, p in enumerate(ps):
        p.grad = M.opt_inputs(p.numel(), F32, gdt, 100 * k + i, False)[2]
        if k == 1 and i == 0:
            p.grad.zero_()  # an all-zero gradient on the second step


@pytest.mark.parametrize("pdt,gdt,master", [(F32, F32, False), (BF16, BF16, True), (F16, F16, True), (BF16, BF16, False)])
@pytest.mark.parametrize("opts", [dict(weight_decay=0.1), dict(weight_decay=0.0, always_adapt=True, maximize=True),
                                  dict(weight_decay=0.0, bias_correction=False)])
def test_lamb_cpu_path_three_steps(pdt, gdt, master, opts):
    ps = _params(pdt, gdt)
    opt = FusedLAMB(ps, lr=1e-2, master_weights=master, **opts)
    kw = dict(L.LAMB_HP, weight_decay=opts["weight_decay"], bias_correction=opts.get("bias_correction", True),
              adapt=opts["weight_decay"] != 0 or opts.get("always_adapt", False), maximize=opts.get("maximize", False))
    for k in range(3):
        _grads(ps, gdt, k)
        gs = GS if k == 1 else None
        pre = []
        for p in ps:
            st = opt.state[p]
            z = torch.zeros(p.numel())
            pre.append((p.detach().clone(), st["master"].clone() if "master" in st else None, p.grad.clone(),
                        st.get("exp_avg", z).clone(), st.get("exp_avg_sq", z).clone()))
        opt.step(grad_scale=gs)
        ratios = opt.trust_ratios()
        for i, (p, (p0, mw, g, m, v)) in enumerate(zip(ps, pre)):
            if master and mw is None:
                mw = p0.float()  # the master is created from the parameter on the first step
            ref = L.ref_lamb_step(p0, g, m, v, step=k + 1, grad_scale=gs, master=mw, **kw)
            tag = f"lamb cpu step {k} tensor {i}"
            st = opt.state[p]
            if master:
                L.check(tag + " master", st["master"], ref["p"], L.elem_bound(ref["p"], F32, L.C["lamb_p"], ref["p_scale"]))
                assert torch.equal(p.detach(), st["master"].to(pdt))
            else:
                L.check(tag + " p", p.detach(), ref["p"], L.elem_bound(ref["p"], pdt, L.C["lamb_p"], ref["p_scale"]))
            L.check(tag + " m", st["exp_avg"], ref["m"], L.elem_bound(ref["m"], F32, L.C["lamb_m"], ref["m_scale"]))
            L.check(tag + " v", st["exp_avg_sq"], ref["v"], L.elem_bound(ref["v"], F32, L.C["lamb_v"], ref["v_scale"]))
            L.check(tag + " r", ratios[p], ref["r"], L.C["lamb_r"] * L.EPS32 * ref["r_scale"])
            assert ratios[p].dim() == 0 and ratios[p].dtype == F32
    assert bool(ps[-1].detach().abs().max() > 0)  # the zero-initialised tensor trained


@pytest.mark.parametrize("pdt,gdt,master", [(F32, F32, False), (BF16, BF16, True), (F16, F16, True), (BF16, BF16, False)])
@pytest.mark.parametrize("opts", [dict(momentum=0.9, weight_decay=0.01), dict(momentum=0.9, nesterov=True, maximize=True),
                                  dict(momentum=0.0, weight_decay=0.01), dict(momentum=0.9, dampening=0.1)])
def test_lars_cpu_path_three_steps(pdt, gdt, master, opts):
    ps = _params(pdt, gdt)
    opt = FusedLARS(ps, lr=0.1, trust_coefficient=0.02, master_weights=master, **opts)
    kw = dict(L.LARS_HP, momentum=opts["momentum"], dampening=opts.get("dampening", 0.0),
              weight_decay=opts.get("weight_decay", 0.0), nesterov=opts.get("nesterov", False),
              maximize=opts.get("maximize", False))
    for k in range(3):
        _grads(ps, gdt, k)
        gs = GS if k == 1 else None
        pre = []
        for p in ps:
            st = opt.state[p]
            pre.append((p.detach().clone(), st["master"].clone() if "master" in st else None, p.grad.clone(),
                        st["momentum_buffer"].clone() if "momentum_buffer" in st else torch.zeros(p.numel())))
        opt.step(grad_scale=gs)
        ratios = opt.trust_ratios()
        for i, (p, (p0, mw, g, buf)) in enumerate(zip(ps, pre)):
            if master and mw is None:
                mw = p0.float()
            ref = L.ref_lars_step(p0, g, buf, first=k == 0, grad_scale=gs, master=mw, **kw)
            tag = f"lars cpu step {k} tensor {i}"
            st = opt.state[p]
            if master:
                L.check(tag + " master", st["master"], ref["p"], L.elem_bound(ref["p"], F32, L.C["lars_p"], ref["p_scale"]))
                assert torch.equal(p.detach(), st["master"].to(pdt))
            else:
                L.check(tag + " p", p.detach(), ref["p"], L.elem_bound(ref["p"], pdt, L.C["lars_p"], ref["p_scale"]))
            if kw["momentum"] != 0:
                L.check(tag + " buf", st["momentum_buffer"], ref["buf"],
                        L.elem_bound(ref["buf"], F32, L.C["lars_buf"], ref["buf_scale"]))
            L.check(tag + " r", ratios[p], ref["r"], L.C["lars_r"] * L.EPS32 * ref["r_scale"])
    r = opt.trust_ratios()
    assert r[ps[-1]].item() != 1.0 and bool(ps[-1].detach().abs().max() > 0)  # zero-initialised, trained since


@pytest.mark.parametrize("cls,kw", [(FusedLAMB, dict(lr=1e-2)), (FusedLARS, dict(lr=0.1, momentum=0.9, weight_decay=0.01))])
def test_state_dict_round_trip_keeps_state_dtypes(cls, kw):
    ps, qs = _params(BF16, BF16), _params(BF16, BF16)
    o1, o2 = cls(ps, master_weights=True, **kw), cls(qs, master_weights=True, **kw)
    for k in range(2):
        _grads(ps, BF16, k)
        o1.step()
    sd = copy.deepcopy(o1.state_dict())  # (as a save and a load: state_dict() hands out the live tensors)
    o2.load_state_dict(sd)
    for p, q in zip(ps, qs):
        q.data.copy_(p.data)
        for key, val in o1.state[p].items():
            got = o2.state[q][key]
            if torch.is_tensor(val):
                assert got.dtype == val.dtype == F32 and torch.equal(got, val), key
            else:
                assert got == val
    _grads(ps, BF16, 2)
    _grads(qs, BF16, 2)
    o1.step()
    o2.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q) and torch.equal(o1.state[p]["master"], o2.state[q]["master"])


def test_layer_adaptation_false_group_equals_fused_sgd():
    for pdt, master in ((F32, False), (BF16, True)):
        a, b = _params(pdt, pdt), _params(pdt, pdt)
        kw = dict(lr=0.1, momentum=0.9, weight_decay=0.01, nesterov=True, master_weights=master)
        oa = FusedLARS([{"params": a[:2]}, {"params": a[2:], "layer_adaptation": False}], **kw)
        ob = FusedSGD(b[2:], **kw)
        for k in range(3):
            _grads(a, pdt, k)
            _grads(b, pdt, k)
            gs = GS if k == 1 else None
            oa.step(grad_scale=gs)
            ob.step(grad_scale=gs)
        for x, y in zip(a[2:], b[2:]):
            assert torch.equal(x, y)
            assert torch.equal(oa.state[x]["momentum_buffer"], ob.state[y]["momentum_buffer"])
            assert oa.trust_ratios()[x].item() == 1.0
        assert oa.trust_ratios()[a[1]].item() != 1.0


def test_error_paths():
    p64 = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    p64.grad = torch.ones(4, dtype=torch.float64)
    for opt in (FusedLAMB([p64]), FusedLARS([p64], lr=0.1)):
        with pytest.raises(TypeError, match="fp64"):
            opt.step()
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="Nesterov"):
        FusedLARS([p], lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="Nesterov"):
        FusedLARS([p], lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)
    for opt in (FusedLAMB([p]), FusedLARS([p], lr=0.1)):
        assert hasattr(opt, "step_params")
        assert not hasattr(opt, "step_slices") and not hasattr(opt, "advance")
        assert opt.trust_ratios() == {}


def test_overlapped_tail_schedule_is_refused_with_a_clear_message():
    from distributeddataparallel_amd.parallel.distributed import DistributedDataParallel as DDP

    p = torch.nn.Parameter(torch.zeros(4))

    class Stub:  # register_overlapped_optimizer checks the optimizer before it touches the DDP instance
        pass

    for opt in (FusedLAMB([p]), FusedLARS([p], lr=0.1)):
        with pytest.raises(TypeError) as e:
            DDP.register_overlapped_optimizer(Stub(), opt, schedule="tail")
        msg = str(e.value)
        assert type(opt).__name__ in msg and "schedule='backward'" in msg and "norm" in msg
        with pytest.raises(ValueError, match="unknown overlapped-optimizer schedule"):
            DDP.register_overlapped_optimizer(Stub(), opt, schedule="later")
    with pytest.raises(TypeError, match="step_params"):
        DDP.register_overlapped_optimizer(Stub(), torch.optim.SGD([p], lr=0.1), schedule="backward")


def test_a_refused_step_changes_nothing_and_a_new_group_is_found():
    for make in (lambda ps: FusedLAMB(ps), lambda ps: FusedLARS(ps, lr=0.1)):
        a, b = torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(4, dtype=torch.float64))
        a.grad, b.grad = torch.ones(4), torch.ones(4, dtype=torch.float64)
        opt = make([{"params": [a]}, {"params": [b]}])  # the refused parameter sits in a later group
        with pytest.raises(TypeError, match="fp64"):
            opt.step()
        assert len(opt.state[a]) == 0 and torch.equal(a.detach(), torch.ones(4)) and opt.trust_ratios() == {}
        with pytest.raises(TypeError, match="fp64"):
            opt.step_params([a, b], [a.grad, b.grad])
        assert len(opt.state[a]) == 0
        c = torch.nn.Parameter(torch.ones(3))
        opt.step_params([a], [a.grad])  # builds the parameter -> group cache
        opt.add_param_group({"params": [c]})
        opt.step_params([c], [torch.ones(3)])
        assert not torch.equal(c.detach(), torch.ones(3))
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    opt = FusedLARS([p], lr=0.1, momentum=0.9)
    opt.param_groups[0]["nesterov"], opt.param_groups[0]["dampening"] = True, 0.1
    with pytest.raises(ValueError, match="Nesterov"):
        opt.step()
    assert len(opt.state[p]) == 0
