"""FusedAdamW / FusedAdam with 8-bit (block-scaled e4m3) moments, CPU backend: parity with the
32-bit states on the first step, the state format, slices, checkpoints and convergence."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _adam8_refs import (SLICINGS, check_neighbours, check_scales, check_shapes, dyadic, exact_moments_b05,
                         run_whole_and_sliced)
from distributeddataparallel_amd.optim import FusedAdam, FusedAdamW


def _pair(cls, shape, dtype, **kw):
    torch.manual_seed(0)
    a = nn.Parameter(torch.randn(shape).to(dtype))
    b = nn.Parameter(a.detach().clone())
    master = dtype != torch.float32
    return (a, cls([a], master_weights=master, **kw)), (b, cls([b], master_weights=master, state_bits=8, **kw))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("maximize,scaled", [(False, False), (True, False), (False, True)])
def test_step1_bitwise_parity_with_32bit_states(cls, wd, maximize, scaled, dtype):
    """The states start at zero and the parameters use the fresh fp32 moments, so after one step the
    parameters (and masters) are bitwise those of state_bits=32."""
    (a, oa), (b, ob) = _pair(cls, (5, 77), dtype, lr=1e-2, weight_decay=wd, maximize=maximize)
    g = torch.randn(5, 77).to(dtype)
    a.grad, b.grad = g.clone(), g.clone()
    gs = torch.tensor([0.37]) if scaled else None
    oa.step(grad_scale=gs)
    ob.step(grad_scale=gs)
    assert torch.equal(a, b)
    if dtype != torch.float32:
        assert ob.state[b]["master"].dtype == torch.float32
        assert torch.equal(oa.state[a]["master"], ob.state[b]["master"])


def test_unknown_state_bits_is_refused():
    with pytest.raises(ValueError):
        FusedAdamW([nn.Parameter(torch.zeros(3))], state_bits=4)


@pytest.mark.parametrize("numel,groups", [(1, 1), (127, 1), (128, 1), (129, 2)])
def test_state_shapes(numel, groups):
    p = nn.Parameter(torch.randn(numel))
    opt = FusedAdamW([p], state_bits=8)
    p.grad = torch.randn(numel)
    opt.step()
    st = opt.state[p]
    check_shapes(st, numel)
    assert st["exp_avg_scale"].numel() == groups and st["exp_avg_sq_scale"].numel() == groups
    m, v = opt.decode_states(p)
    assert m.dtype == torch.float32 and m.shape == p.shape and v.shape == p.shape


def test_scales_are_group_max_over_448_and_codes_are_neighbours():
    """betas = (0.5, 0.5) and dyadic gradients make the fp32 trajectory exactly reproducible (see
    _adam8_refs.dyadic): after each of 5 steps every scale is its group's maximum / 448 exactly and
    every code is a neighbour of the exact value, the exact moments following from decode_states of
    the step before."""
    gen = torch.Generator().manual_seed(3)
    p = nn.Parameter(torch.randn(7, 191))  # 1337 elements: 10 whole groups and one of 57
    opt = FusedAdamW([p], lr=1e-3, betas=(0.5, 0.5), state_bits=8, seed=5)
    m_prev, v_prev = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(5):
        g = dyadic(p.shape, gen)
        if step == 2:
            g.view(-1)[128:256] = 0  # a group whose moments only decay
        p.grad = g
        opt.step()
        m, v = exact_moments_b05(m_prev, v_prev, g)
        check_shapes(opt.state[p], p.numel())
        check_scales(opt.state[p], m, v.sqrt(), f"step {step + 1}: ")
        check_neighbours(opt.state[p], m, v.sqrt(), f"step {step + 1}: ")
        m_prev, v_prev = opt.decode_states(p)


def test_neighbour_property_with_default_betas():
    """Random gradients over 6 decades of magnitude within a group, betas (0.9, 0.999): every decoded
    m and s is within one code step of the exact value (fp64, from the previous decoded state)."""
    gen = torch.Generator().manual_seed(4)
    n = 4096 + 77
    p = nn.Parameter(torch.randn(n))
    opt = FusedAdamW([p], lr=1e-3, state_bits=8)
    m_prev, v_prev = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    mag = 10.0 ** (-6 * torch.rand(n, generator=gen))
    for step in range(4):
        g = torch.randn(n, generator=gen) * mag
        p.grad = g
        opt.step()
        m = 0.9 * m_prev + (1 - 0.9) * g.double()
        v = 0.999 * v_prev + (1 - 0.999) * g.double() ** 2
        # (fp32 rounding of the update, 6e-8 relative, is far below the 2^-3 / 2^-9 code steps)
        check_neighbours(opt.state[p], m, v.sqrt(), f"step {step + 1}: ")
        m_prev, v_prev = (t.double() for t in opt.decode_states(p))


def test_all_zero_gradient_gives_zero_scales_and_codes():
    p = nn.Parameter(torch.randn(300))
    opt = FusedAdamW([p], lr=1e-2, state_bits=8)
    for _ in range(3):
        p.grad = torch.zeros(300)
        opt.step()
    st = opt.state[p]
    for name in ("exp_avg", "exp_avg_sq"):
        assert (st[name + "_q"] == 0).all() and (st[name + "_scale"] == 0).all()
    assert torch.isfinite(p).all()
    # one live element in an otherwise dead group: the dead ones stay at code 0, nothing is NaN
    g = torch.zeros(300)
    g[130] = 1e-3
    p.grad = g
    opt.step()
    assert torch.isfinite(p).all() and st["exp_avg_sq_q"][130] == 0x7E and int((st["exp_avg_sq_q"] != 0).sum()) == 1


@pytest.mark.parametrize("pieces", SLICINGS)
def test_slices_match_whole_update(pieces):
    (pw, sw), (ps, ss) = run_whole_and_sliced("cpu", pieces)
    assert torch.equal(pw, ps) and torch.isfinite(ps).all()
    for key in ("exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale"):
        assert torch.equal(sw[key], ss[key]), key
    assert sw["step"] == ss["step"] == 2


def test_slices_out_of_order_raise():
    p = nn.Parameter(torch.randn(1000))
    opt = FusedAdamW([p], state_bits=8)
    g = torch.randn(1000)
    opt.advance([p])
    with pytest.raises(RuntimeError, match="ascending"):
        opt.step_slices([(p, g, 300, 1000)])
    opt.step_slices([(p, g, 0, 300)])
    with pytest.raises(RuntimeError, match="ascending"):
        opt.step_slices([(p, g, 0, 300)])
    opt.step_slices([(p, g, 300, 1000)])


@pytest.mark.parametrize("bits", [8, 32])
def test_checkpoint_round_trip_keeps_dtypes_and_resumes_bitwise(bits):
    """state_dict -> fresh optimizer -> load_state_dict on a bf16 model with fp32 masters: every state
    tensor keeps its dtype (torch's loader would cast them all to bf16), and three more steps are
    bitwise those of the uninterrupted run."""
    torch.manual_seed(2)
    model = nn.Sequential(nn.Linear(24, 50), nn.Linear(50, 3)).to(torch.bfloat16)
    opt = FusedAdamW(model.parameters(), lr=1e-2, master_weights=True, state_bits=bits, seed=9)
    grads = [[torch.randn_like(p) for p in model.parameters()] for _ in range(5)]

    def run(m, o, steps):
        for gs in steps:
            for p, g in zip(m.parameters(), gs):
                p.grad = g.clone()
            o.step()

    run(model, opt, grads[:2])
    sd = copy.deepcopy(opt.state_dict())
    model2 = copy.deepcopy(model)
    opt2 = FusedAdamW(model2.parameters(), lr=1e-2, master_weights=True, state_bits=bits, seed=1234)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["seed"] == 9 and opt2.param_groups[0]["state_bits"] == bits
    want = ({"exp_avg_q": torch.uint8, "exp_avg_sq_q": torch.uint8, "exp_avg_scale": torch.float32,
             "exp_avg_sq_scale": torch.float32} if bits == 8 else
            {"exp_avg": torch.float32, "exp_avg_sq": torch.float32})
    want["master"] = torch.float32
    for p in model2.parameters():
        st = opt2.state[p]
        assert st["step"] == 2
        assert {k: v.dtype for k, v in st.items() if torch.is_tensor(v)} == want
    run(model, opt, grads[2:])
    run(model2, opt2, grads[2:])
    for a, b in zip(model.parameters(), model2.parameters()):
        assert torch.equal(a, b)
        for k, v in opt.state[a].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(opt2.state[b][k])), k


def _train_mlp(order_seed, steps=300, **opt_kw):
    """2-layer MLP (64-128-10) on a fixed synthetic classification set; the final loss on the whole set."""
    data = torch.Generator().manual_seed(100)
    x = torch.randn(512, 64, generator=data)
    y = (x @ torch.randn(64, 10, generator=data) + 0.5 * torch.randn(512, 10, generator=data)).argmax(1)
    torch.manual_seed(7)
    model = nn.Sequential(nn.Linear(64, 128), nn.ReLU(), nn.Linear(128, 10))
    opt = FusedAdamW(model.parameters(), lr=3e-3, betas=(0.9, 0.999), weight_decay=1e-2, **opt_kw)
    order = torch.Generator().manual_seed(order_seed)
    for _ in range(steps):
        idx = torch.randint(0, 512, (64,), generator=order)
        opt.zero_grad()
        F.cross_entropy(model(x[idx]), y[idx]).backward()
        opt.step()
    with torch.no_grad():
        return F.cross_entropy(model(x), y).item()


def test_convergence_is_within_the_fp32_runs_spread():
    """300 steps with beta2 = 0.999. The yardstick is state_bits=32 over 5 data orders: the 8-bit
    run's final training loss may be at most the worst of them plus their spread. Measured here
    (CPU backend): fp32 min 0.0139 / max 0.0146 over the 5 orders, 8-bit 0.0143 (order 0)."""
    fp32 = [_train_mlp(s) for s in range(5)]
    lo, hi = min(fp32), max(fp32)
    q8 = _train_mlp(0, state_bits=8)
    print(f"fp32 final loss min {lo:.4f} max {hi:.4f}; state_bits=8 final loss {q8:.4f}")
    assert q8 <= hi + (hi - lo), (q8, lo, hi)
