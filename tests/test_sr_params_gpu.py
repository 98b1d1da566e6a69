"""Stochastically rounded bf16 parameters on the MI355X: the rounding kernel against the CPU oracle,
and FusedAdamW / FusedAdam(param_rounding="stochastic") with 32-bit and 8-bit states: stagnation
removed, independence of launches, alignment and slices, one random stream for both kernels,
seeds and graph capture."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from _adam8_refs import SLICINGS
from _sr_refs import bf16_bits, crafted, random_f32, ref_round_bits
from distributeddataparallel_amd.optim import FusedAdam, FusedAdamW, stochastic_round_bf16
from test_adam8_gpu import NUMELS, _params, _set_grads

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
KEYS = [(0, 0, 0, 0), (12345, 7, 300, 129), ((1 << 63) - 1, (1 << 32) - 1, (1 << 32) - 1, (1 << 32) - 4099)]


def _sr_kw(bits, **kw):
    return dict(lr=1e-2, weight_decay=0.1, state_bits=bits, param_rounding="stochastic", **kw)


# ---- the rounding kernel ------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,ordinal,step,offset", KEYS)
def test_kernel_matches_oracle_on_crafted_inputs(seed, ordinal, step, offset):
    """Every bf16 pattern, NaNs, infinities, the largest finite values, fp32 neighbours of bf16 values:
    bitwise the CPU path, which is bitwise the definition (numpy reference)."""
    x = crafted()
    want = stochastic_round_bf16(x, seed, ordinal, step, offset)
    assert np.array_equal(bf16_bits(want), ref_round_bits(x, seed, ordinal, step, offset))
    got = stochastic_round_bf16(x.cuda(), seed, ordinal, step, offset)
    assert got.dtype == BF16 and got.is_cuda
    assert np.array_equal(bf16_bits(got), bf16_bits(want))
    assert bf16_bits(got)[0x7F80] == 0x7F80 and bf16_bits(got)[0xFF80] == 0xFF80
    assert bf16_bits(got)[1 << 16] == 0x7F7F and bf16_bits(got)[(1 << 16) + 1] == 0xFF7F


@pytest.mark.parametrize("numel", [1, 7, 8191, 8192, 8193, 3 * 8192 + 130])
def test_kernel_matches_oracle_on_random_data(numel):
    """Chunk tails and whole chunks (a block owns 8192 elements), aligned and starting 4 bytes into
    the buffer (not 16-B aligned: the scalar path), offsets that carry element indices past 2^32."""
    x = random_f32(numel + 1, numel)
    xg = x.cuda()
    for seed, ordinal, step, offset in KEYS:
        for lead in (0, 1):
            src = xg[lead:lead + numel]
            assert (src.data_ptr() % 16 != 0) == bool(lead)
            got = stochastic_round_bf16(src, seed, ordinal, step, offset)
            want = stochastic_round_bf16(x[lead:lead + numel], seed, ordinal, step, offset)
            assert torch.equal(got.cpu(), want), (numel, lead, seed)
    whole = stochastic_round_bf16(xg[:numel], 5, 1, 2)
    a = numel // 3
    assert torch.equal(stochastic_round_bf16(xg[a:numel], 5, 1, 2, offset=a), whole[a:])


# ---- the optimizers -------------------------------------------------------------------------------------

def test_stagnation_is_removed():
    """65,536 bf16 parameters at 1.0, gradient 1.0, lr 2^-12: every step asks for 1/16 of the bf16
    step below 1.0 (2^-8). Round-to-nearest without a master never moves. With stochastic rounding
    each step moves each element down one bf16 step with probability 1/16: after 256 steps the
    number of moves is Binomial(256, 1/16) (mean 16, variance 15), so the mean parameter is within
    6 sigma = 6 sqrt(15) 2^-8 / 256 of the master-weight run's, and the variance of the moves over
    the elements is within [0.8, 1.25] x 15 (a key that ignores the step or the element index gives
    thousands or zero)."""
    n, steps = 65536, 256
    res = {}
    for name, kw in (("master", dict(master_weights=True)), ("nearest", {}), ("sr", dict(param_rounding="stochastic"))):
        p = nn.Parameter(torch.ones(n, device="cuda", dtype=BF16))
        opt = FusedAdamW([p], lr=2.0 ** -12, weight_decay=0.0, eps=1e-8, **kw)
        p.grad = torch.ones(n, device="cuda", dtype=BF16)
        for _ in range(steps):
            opt.step()
        res[name] = p.detach().double().cpu()
        assert ("master" in opt.state[p]) == (name == "master")
    assert (res["nearest"] == 1.0).all()
    moves = (1.0 - res["sr"]) * 256
    assert torch.equal(moves, moves.round()) and moves.min() >= 0
    ref_mean, mean, var = res["master"].mean().item(), res["sr"].mean().item(), moves.var().item()
    bound = 6 * math.sqrt(15) * 2.0 ** -8 / 256
    print(f"mean: master {ref_mean:.6f}, stochastic {mean:.6f} (diff {mean - ref_mean:+.2e}, bound {bound:.2e}); "
          f"moves: mean {moves.mean().item():.3f}, variance {var:.3f} (15 expected)")
    assert abs(mean - ref_mean) <= bound
    assert 0.8 * 15 <= var <= 1.25 * 15


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("bits", [32, 8])
@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam])
def test_step1_is_the_master_update_rounded_with_the_ops_bits(cls, bits, misaligned):
    """From zero moments the master-weight kernel and the stochastic one compute the same fp32 value
    (the same update from the same bf16 parameter): every parameter is stochastic_round_bf16 of the
    master run's master, keyed by (seed, its ordinal, step 1, element index)."""
    pa, pb = _params(BF16, misaligned), _params(BF16, misaligned)
    oa = cls(pa, lr=1e-2, weight_decay=0.1, state_bits=bits, master_weights=True)
    ob = cls(pb, **_sr_kw(bits, seed=17))
    _set_grads(pa, 0)
    _set_grads(pb, 0)
    gs = torch.tensor([0.5], device="cuda")
    oa.step(grad_scale=gs)
    ob.step(grad_scale=gs)
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert "master" not in ob.state[b]
        assert torch.equal(b, stochastic_round_bf16(oa.state[a]["master"], 17, i, 1)), (i, a.numel())


def _three_steps(opt, ps, how):
    for step in range(3):
        _set_grads(ps, step)
        if how == "step":
            opt.step()
        elif how == "buckets":  # other launches, another order
            for chunk in (ps[30:], ps[5:30], ps[:5]):
                opt.step_params(chunk, [q.grad for q in chunk])
        else:  # every parameter in a launch of its own, last first
            for q in reversed(ps):
                opt.step_params([q], [q.grad])
        if step == 0 and "exp_avg_q" in opt.state[ps[0]]:
            assert all(opt.state[q]["exp_avg_sq_q"].any() for q in ps)


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("bits", [32, 8])
def test_results_do_not_depend_on_the_launch(bits, misaligned):
    """45 parameters (the segment table turns over at 40), three steps: one step() over one group, the
    same parameters split over three param groups (same ordinals, other launches), bucket by bucket
    in another order, and each parameter in a launch of its own give bitwise equal parameters. With
    the misaligned member its launch goes scalar, the single launches of the others stay vector."""
    runs = []
    for how in ("step", "groups", "buckets", "single"):
        ps = _params(BF16, misaligned)
        groups = [{"params": ps[:5]}, {"params": ps[5:30]}, {"params": ps[30:]}] if how == "groups" else ps
        opt = FusedAdamW(groups, **_sr_kw(bits, seed=7))
        _three_steps(opt, ps, "step" if how == "groups" else how)
        assert all("master" not in opt.state[q] and opt.state[q]["step"] == 3 for q in ps)
        runs.append(ps)
    for other in runs[1:]:
        for i, (a, b) in enumerate(zip(runs[0], other)):
            assert torch.equal(a, b), (i, a.numel())


@pytest.mark.parametrize("bits", [32, 8])
def test_vector_and_scalar_paths_agree(bits):
    n = 3 * 8192 + 130
    init = torch.randn(n + 1).to("cuda", BF16)
    pa, pb = nn.Parameter(init[1:].clone()), nn.Parameter(init.clone()[1:])
    assert pa.data_ptr() % 16 == 0 and pb.data_ptr() % 16 != 0
    oa, ob = FusedAdamW([pa], **_sr_kw(bits, seed=3)), FusedAdamW([pb], **_sr_kw(bits, seed=3))
    for step in range(3):
        _set_grads([pa], step)
        _set_grads([pb], step)
        oa.step()
        ob.step()
    assert torch.equal(pa, pb)


BIG = 3 * 8192 + 130
BIG_SLICING = [(0, 8191), (8191, 2 * 8192 + 1), (2 * 8192 + 1, BIG)]  # cuts off the multiples of 8 and of 128


@pytest.mark.parametrize("numel,pieces", [(1000, SLICINGS[0]), (1000, SLICINGS[1]), (BIG, BIG_SLICING)])
@pytest.mark.parametrize("bits", [32, 8])
def test_slices_match_whole_update(bits, numel, pieces):
    """advance + step_slices piece by piece against step(): bitwise equal parameters after two steps.
    Only what has arrived of the gradient is valid when a piece is stepped (NaN beyond it)."""
    torch.manual_seed(1)
    init = torch.randn(numel).to(BF16)
    grads = [torch.randn(numel).to(BF16) for _ in range(2)]
    out = []
    for sliced in (False, True):
        p = nn.Parameter(init.clone().cuda())
        opt = FusedAdamW([nn.Parameter(torch.zeros(3, device="cuda")), p], **_sr_kw(bits, seed=11))
        for g in grads:
            g = g.cuda()
            if not sliced:
                p.grad = g
                opt.step()
                continue
            opt.advance([p])
            for lo, hi in pieces:
                have = torch.full_like(g, float("nan"))
                have[:hi] = g[:hi]
                opt.step_slices([(p, have, lo, hi)])
        assert opt.state[p]["step"] == 2 and "master" not in opt.state[p]
        out.append(p)
    assert torch.isfinite(out[1]).all() and torch.equal(out[0], out[1])
    assert not torch.equal(out[0].cpu(), init)


@pytest.mark.parametrize("misaligned", [False, True])
def test_both_kernels_share_the_stream(misaligned):
    """Step 1 from zero moments: adam8_kernel and the 32-bit kernel see the same fp32 value, the same
    key and the fresh fp32 moments, so the parameters agree bitwise."""
    pa, pb = _params(BF16, misaligned), _params(BF16, misaligned)
    oa, ob = FusedAdamW(pa, **_sr_kw(32, seed=5)), FusedAdamW(pb, **_sr_kw(8, seed=5))
    _set_grads(pa, 0)
    _set_grads(pb, 0)
    oa.step()
    ob.step()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), (i, a.numel())


@pytest.mark.parametrize("bits", [32, 8])
def test_seeds(bits):
    """Same seed: bitwise equal after 3 steps. Another seed: every parameter of 128 or more elements
    differs somewhere. An fp32 parameter in the same optimizer consumes no random bits of its own."""
    runs = []
    for seed in (7, 7, 8):
        ps = _params(BF16, False) + [nn.Parameter(torch.randn(5000, generator=torch.Generator().manual_seed(1)).cuda())]
        opt = FusedAdamW(ps, **_sr_kw(bits, seed=seed))
        for step in range(3):
            _set_grads(ps, step)
            opt.step()
        runs.append(ps)
    for a, b, c in zip(*runs):
        assert torch.equal(a, b)
        if a.dtype == torch.float32:  # (with 8-bit states its moments are rounded with the seed's bits)
            assert bits == 8 or torch.equal(a, c)
        elif a.numel() >= 128:
            assert not torch.equal(a, c), a.numel()
    assert sum(a.numel() >= 128 for a in runs[0]) > len(NUMELS)


def test_fp32_parameters_match_the_nearest_optimizer():
    pa, pb = _params(torch.float32, False), _params(torch.float32, False)
    oa, ob = FusedAdamW(pa, lr=1e-2, weight_decay=0.1), FusedAdamW(pb, **_sr_kw(32))
    for step in range(2):
        _set_grads(pa, step)
        _set_grads(pb, step)
        oa.step()
        ob.step()
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))


@pytest.mark.parametrize("bits", [32, 8])
def test_capture_is_refused_before_anything_is_launched(bits):
    p = nn.Parameter(torch.randn(1000, device="cuda").to(BF16))
    p.grad = torch.randn(1000, device="cuda").to(BF16)
    opt = FusedAdamW([p], **_sr_kw(bits))
    before = p.detach().clone()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            opt.step()
    torch.cuda.synchronize()
    assert len(opt.state[p]) == 0 and torch.equal(p, before)
    opt.step()  # outside a capture the same optimizer steps
    assert opt.state[p]["step"] == 1 and not torch.equal(p, before)
