"""Stochastically rounded bf16 parameters, CPU backend: the rounding's definition and statistics,
its keying, and FusedAdamW / FusedAdam(param_rounding="stochastic") without master weights."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from _sr_refs import (all_bf16_patterns, bf16_bits, crafted, f32_bits, from_f32_bits, random_f32, ref_round_bits,
                      stream_keys)
from distributeddataparallel_amd.optim import FusedAdam, FusedAdamW, stochastic_round_bf16

KEYS = [(0, 0, 0), (1, 0, 1), (12345, 7, 300), ((1 << 63) - 1, (1 << 32) - 1, (1 << 32) - 1)]  # (seed, ordinal, step)


@pytest.mark.parametrize("seed,ordinal,step", KEYS)
def test_bf16_values_come_back_unchanged(seed, ordinal, step):
    """All 65,536 bf16 patterns widened to fp32: the low half is zero, so no r can carry. +-inf stay
    +-inf, every NaN pattern gives a NaN."""
    x = all_bf16_patterns()
    got = bf16_bits(stochastic_round_bf16(x, seed, ordinal, step))
    pat = np.arange(1 << 16, dtype=np.uint16)
    nan = ((pat & 0x7F80) == 0x7F80) & ((pat & 0x007F) != 0)
    assert np.array_equal(got[~nan], pat[~nan])
    assert (((got[nan] & 0x7F80) == 0x7F80) & ((got[nan] & 0x007F) != 0)).all()
    assert got[0x7F80] == 0x7F80 and got[0xFF80] == 0xFF80


@pytest.mark.parametrize("seed,ordinal,step", KEYS)
def test_nan_inf_and_saturation(seed, ordinal, step):
    x = from_f32_bits([0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF])
    x = x.repeat(4096)  # every element index draws other bits
    y = stochastic_round_bf16(x, seed, ordinal, step)
    got = bf16_bits(y).reshape(4096, 8)
    assert (got[:, 0] == 0x7F7F).all() and (got[:, 1] == 0xFF7F).all()  # finite never becomes inf
    assert (got[:, 2] == 0x7F80).all() and (got[:, 3] == 0xFF80).all()
    assert torch.isnan(y.view(4096, 8)[:, 4:]).all()


def test_matches_the_definition_bit_for_bit():
    """The int64 emulation against the definition in numpy's wrapping uint32 arithmetic: crafted and
    random inputs, element indices on both sides of 2^32."""
    x = torch.cat([crafted(), random_f32(50000, 1)])
    for (seed, ordinal, step), offset in zip(KEYS, (0, 7, (1 << 32) - 1000, (1 << 40) + 3)):
        got = bf16_bits(stochastic_round_bf16(x, seed, ordinal, step, offset))
        assert np.array_equal(got, ref_round_bits(x, seed, ordinal, step, offset)), (seed, ordinal, step, offset)


def test_third_stream_key_differs_from_the_moment_keys():
    for seed, ordinal, step in KEYS:
        km, ks, kp = stream_keys(seed, ordinal, step)
        assert kp != km and kp != ks


def test_result_is_one_of_the_two_neighbours():
    """Random finite fp32 values: truncation, or one bf16 step further from zero."""
    x = random_f32(200000, 2)
    u = f32_bits(x).astype(np.int64)
    got = bf16_bits(stochastic_round_bf16(x, 3, 1, 2)).astype(np.int64)
    trunc = u >> 16
    assert np.isin(got - trunc, (0, 1)).all()
    inexact = (u & 0xFFFF) != 0
    assert (got[~inexact] == trunc[~inexact]).all()
    assert 0.3 < (got[inexact] != trunc[inexact]).mean() < 0.7  # both neighbours occur


@pytest.mark.parametrize("low", [0x1000, 0x8000, 0xF000])
@pytest.mark.parametrize("sign", [0, 0x80000000])
def test_round_up_frequency(low, sign):
    """One value with low half L over 65,536 element indices: the share rounded away from zero is
    within 6 sigma of q = L / 65536, sigma = sqrt(q (1 - q) / 65536)."""
    n = 65536
    bits = sign | 0x3F8A0000 | low
    x = from_f32_bits(np.full(n, bits, dtype=np.uint32))
    got = bf16_bits(stochastic_round_bf16(x, 9, 2, 5)).astype(np.int64)
    assert np.isin(got, (bits >> 16, (bits >> 16) + 1)).all()
    share = float((got == (bits >> 16) + 1).mean())
    q = low / 65536
    sigma = math.sqrt(q * (1 - q) / n)
    print(f"L = {low:#06x}: share rounded away from zero {share:.5f}, q {q:.5f}, ({share - q:+.2e}) / sigma = "
          f"{(share - q) / sigma:+.2f}")
    assert abs(share - q) <= 6 * sigma


def test_keying():
    """The bits change with each of seed, ordinal, step and offset; a slice rounded with its offset is
    that slice of the whole; shape and dense strides do not matter, only memory order."""
    x = random_f32(20000, 3)
    base = stochastic_round_bf16(x, 5, 1, 2, 0)
    assert torch.equal(base, stochastic_round_bf16(x, 5, 1, 2, 0))
    for other in ((6, 1, 2, 0), (5, 2, 2, 0), (5, 1, 3, 0), (5, 1, 2, 1)):
        assert not torch.equal(base, stochastic_round_bf16(x, *other)), other
    for a, b in ((0, 1), (1, 20000), (127, 8193), (19999, 20000)):
        assert torch.equal(stochastic_round_bf16(x[a:b], 5, 1, 2, offset=a), base[a:b]), (a, b)
    assert torch.equal(stochastic_round_bf16(x.view(100, 200), 5, 1, 2), base.view(100, 200))
    t = x.view(100, 200).t()  # dense, permuted: flat memory order is x's
    y = stochastic_round_bf16(t, 5, 1, 2)
    assert y.shape == t.shape and y.stride() == t.stride() and torch.equal(y.t().reshape(-1), base)
    assert stochastic_round_bf16(torch.empty(0), 1).numel() == 0
    with pytest.raises(TypeError):
        stochastic_round_bf16(x.double(), 1)
    with pytest.raises(ValueError):
        stochastic_round_bf16(x.view(100, 200)[:, ::2], 1)


# ---- the optimizers ---------------------------------------------------------------------------------

def test_value_errors():
    bf = lambda: nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))  # noqa: E731
    for cls in (FusedAdamW, FusedAdam):
        with pytest.raises(ValueError, match="master"):
            cls([bf()], master_weights=True, param_rounding="stochastic")
        with pytest.raises(ValueError, match="param_rounding"):
            cls([bf()], param_rounding="up")
        with pytest.raises(ValueError, match="bf16"):
            cls([nn.Parameter(torch.zeros(3, dtype=torch.float16))], param_rounding="stochastic")
    assert FusedAdamW([bf()]).defaults["param_rounding"] == "nearest"


def _model(seed=0):
    """bf16 and fp32 parameters in one optimizer; one bf16 parameter is dense but not contiguous."""
    gen = torch.Generator().manual_seed(seed)
    ps = [nn.Parameter(torch.randn(n, generator=gen).to(torch.bfloat16)) for n in (1, 129, 1000)]
    ps.append(nn.Parameter(torch.randn(40, 30, generator=gen).to(torch.bfloat16).t()))
    ps.append(nn.Parameter(torch.randn(300, generator=gen)))
    return ps


def _grads(ps, k):
    gen = torch.Generator().manual_seed(100 + k)
    for p in ps:
        p.grad = torch.empty_like(p).copy_(torch.randn(p.shape, generator=gen))  # (the parameter's strides)


@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam])
@pytest.mark.parametrize("bits", [32, 8])
def test_step_is_the_fp32_update_rounded_with_the_ops_bits(cls, bits):
    """Step 1 from zero moments: bf16 parameters are stochastic_round_bf16 of the fp32 value that a
    master-weight run computes (same fp32 arithmetic), keyed by (seed, ordinal, 1, index); the fp32
    parameter equals the nearest run's; no master state exists."""
    kw = dict(lr=1e-2, weight_decay=0.1, state_bits=bits, seed=21)
    pa, pb = _model(), _model()
    oa, ob = cls(pa, master_weights=True, **kw), cls(pb, param_rounding="stochastic", **kw)
    _grads(pa, 0)
    _grads(pb, 0)
    oa.step()
    ob.step()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert "master" not in ob.state[b]
        if a.dtype == torch.float32:
            assert torch.equal(a, b)
        else:
            want = stochastic_round_bf16(oa.state[a]["master"], 21, i, 1)
            assert torch.equal(b, want), i
            assert b.numel() < 100 or not torch.equal(a, b)
    assert ob.state_dict()["param_groups"][0]["param_rounding"] == "stochastic"


def test_small_updates_are_applied_in_expectation():
    """4096 bf16 parameters at 1.0, gradient 1.0, lr 2^-12 (1/16 of the bf16 step below 1.0), 64 steps:
    nearest rounding leaves every parameter at 1.0; stochastic rounding follows the master run's mean
    within 6 sigma (each step is a Bernoulli(1/16) move of 2^-8; sigma of the mean over 4096 elements
    = 2^-8 sqrt(64 * 15 / 256 / 4096))."""
    res = {}
    for name, kw in (("master", dict(master_weights=True)), ("nearest", {}), ("sr", dict(param_rounding="stochastic"))):
        p = nn.Parameter(torch.ones(4096, dtype=torch.bfloat16))
        opt = FusedAdamW([p], lr=2.0 ** -12, weight_decay=0.0, eps=1e-8, seed=3, **kw)
        for _ in range(64):
            p.grad = torch.ones_like(p)
            opt.step()
        res[name] = p.detach().double()
    assert (res["nearest"] == 1.0).all()
    sigma = 2.0 ** -8 * math.sqrt(64 * 15 / 256 / 4096)
    print(f"means: master {res['master'].mean():.6f}, stochastic {res['sr'].mean():.6f}, 6 sigma {6 * sigma:.2e}")
    assert abs(res["sr"].mean() - res["master"].mean()) <= 6 * sigma


@pytest.mark.parametrize("bits", [32, 8])
def test_state_dict_round_trip_continues_bitwise(bits):
    """bits = 32: 3 steps, save, load into a fresh optimizer over copies of the parameters, 3 more
    steps: bitwise the uninterrupted 6 steps. (bits = 8 draws the CPU path's moment bits from a
    generator seeded by the same tuple, so it holds there too.)"""
    kw = dict(lr=1e-2, weight_decay=0.1, state_bits=bits, seed=8, param_rounding="stochastic")
    pa = _model()
    oa = FusedAdamW(pa, **kw)
    for k in range(3):
        _grads(pa, k)
        oa.step()
    pb = [nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in pa]
    ob = FusedAdamW(pb, lr=1e-2, weight_decay=0.1, state_bits=bits, seed=99, param_rounding="stochastic")
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert ob.param_groups[0]["seed"] == 8 and ob.param_groups[0]["param_rounding"] == "stochastic"
    for k in range(3, 6):
        for ps, o in ((pa, oa), (pb, ob)):
            _grads(ps, k)
            o.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        assert "master" not in ob.state[b] and ob.state[b]["step"] == 6


def test_master_checkpoint_loads_into_a_stochastic_optimizer_and_not_back():
    pa = _model()
    oa = FusedAdamW(pa, lr=1e-2, master_weights=True, seed=4)
    for k in range(2):
        _grads(pa, k)
        oa.step()
    sd = copy.deepcopy(oa.state_dict())
    pb = [nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in pa]
    ob = FusedAdamW(pb, lr=1e-2, seed=4, param_rounding="stochastic")
    ob.load_state_dict(sd)
    grp = ob.param_groups[0]
    assert grp["param_rounding"] == "stochastic" and grp["master_weights"] is False
    changed = 0
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert "master" not in ob.state[b]
        if a.dtype == torch.bfloat16:
            assert torch.equal(b, stochastic_round_bf16(oa.state[a]["master"], 4, i, 2))
            changed += int(not torch.equal(a, b))
        else:
            assert torch.equal(a, b)
        assert torch.equal(ob.state[b]["exp_avg"], oa.state[a]["exp_avg"])
    assert changed >= 2  # (the nearest-rounded parameters were replaced)
    _grads(pb, 2)
    ob.step()  # and it steps: no master comes back
    assert all("master" not in ob.state[b] for b in pb)
    pc = [nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in pa]
    oc = FusedAdamW(pc, lr=1e-2, master_weights=True, seed=4)
    with pytest.raises(ValueError, match="param_rounding='stochastic'"):
        oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert len(oc.state) == 0


@pytest.mark.parametrize("pieces", [[(0, 300), (300, 1000)], [(0, 1), (1, 129), (129, 777), (777, 1000)]])
def test_slices_match_whole_update(pieces):
    """state_bits = 32: any ascending contiguous slicing gives the whole-parameter bits (the hash is
    keyed by the element's index within the parameter)."""
    torch.manual_seed(1)
    init, grads = torch.randn(1000).to(torch.bfloat16), [torch.randn(1000).to(torch.bfloat16) for _ in range(2)]
    out = []
    for sliced in (False, True):
        p = nn.Parameter(init.clone())
        opt = FusedAdamW([nn.Parameter(torch.zeros(3)), p], lr=1e-2, weight_decay=0.1, seed=11,
                         param_rounding="stochastic")
        for g in grads:
            if sliced:
                opt.advance([p])
                for lo, hi in pieces:
                    opt.step_slices([(p, g, lo, hi)])
            else:
                p.grad = g
                opt.step()
        out.append(p)
    assert torch.equal(out[0], out[1])
