"""FusedAdamW(state_bits=8) on the MI355X: the adam8 HIP kernel (block-scaled e4m3 moments with
stochastic rounding) against the 32-bit kernel, the state format, the rounding's statistics,
determinism, slices, the overlapped optimizer, graph capture and the CPU path."""
import math
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _adam8_refs import (SLICINGS, check_neighbours, check_scales, check_shapes, decode, dyadic, e4m3_values,
                         exact_moments_b05, run_whole_and_sliced)
from distributeddataparallel_amd.optim import FusedAdam, FusedAdamW

pytestmark = pytest.mark.gpu

STATE_KEYS = ("exp_avg_q", "exp_avg_scale", "exp_avg_sq_q", "exp_avg_sq_scale")
# group tail, chunk tail (a block owns 8192 elements), whole chunks
NUMELS = [1, 7, 127, 128, 129, 8191, 8192, 8193, 3 * 8192 + 130]


def _params(dtype, misaligned, seed=0):
    """45 parameters (the segment table turns over at 40): NUMELS, small ones, and with `misaligned`
    one that starts 1 element into its buffer (not 16-B aligned: the whole launch goes scalar)."""
    gen = torch.Generator().manual_seed(seed)
    numels = NUMELS + [33 + 5 * i for i in range(45 - len(NUMELS) - 1)]
    ps = [nn.Parameter(torch.randn(n, generator=gen).to("cuda", dtype)) for n in numels]
    buf = torch.randn(2 * 8192 + 71, generator=gen).to("cuda", dtype)
    ps.append(nn.Parameter(buf[1:] if misaligned else buf[:-1].clone()))
    assert len(ps) == 45 and (ps[-1].data_ptr() % 16 != 0) == misaligned
    return ps


def _set_grads(ps, seed, dtype=None):
    gen = torch.Generator().manual_seed(1000 + seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen).to("cuda", dtype or p.dtype)


def _assert_states_equal(oa, pa, ob, pb):
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        for k in STATE_KEYS:
            assert torch.equal(oa.state[a][k], ob.state[b][k]), k
        if "master" in oa.state[a]:
            assert torch.equal(oa.state[a]["master"], ob.state[b]["master"])


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam])
def test_step1_bitwise_parity_with_32bit_kernel(cls, dtype, misaligned):
    """The states start at zero and the update uses the fresh fp32 moments: after one step parameters
    and masters are bitwise those of adam_kernel (bf16 params + fp32 masters + bf16 grads, and fp32)."""
    kw = dict(lr=1e-2, weight_decay=0.1, master_weights=dtype == torch.bfloat16)
    pa, pb = _params(dtype, misaligned), _params(dtype, misaligned)
    oa, ob = cls(pa, **kw), cls(pb, state_bits=8, **kw)
    _set_grads(pa, 0)
    _set_grads(pb, 0)
    gs = torch.tensor([0.5], device="cuda")
    oa.step(grad_scale=gs)
    ob.step(grad_scale=gs)
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), (i, a.numel())
        if dtype == torch.bfloat16:
            assert torch.equal(oa.state[a]["master"], ob.state[b]["master"]), (i, a.numel())
        check_shapes(ob.state[b], b.numel())
        assert ob.state[b]["exp_avg_sq_q"].any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_vector_and_scalar_paths_agree(dtype):
    """The same values in an aligned and in a misaligned tensor (same seed, ordinal and step) give
    identical codes, scales and parameters: only the loads and stores differ between the paths."""
    n = 3 * 8192 + 130
    init = torch.randn(n + 1).to("cuda", dtype)
    pa, pb = nn.Parameter(init[1:].clone()), nn.Parameter(init.clone()[1:])
    assert pa.data_ptr() % 16 == 0 and pb.data_ptr() % 16 != 0
    kw = dict(lr=1e-2, weight_decay=0.1, master_weights=dtype == torch.bfloat16, state_bits=8, seed=3)
    oa, ob = FusedAdamW([pa], **kw), FusedAdamW([pb], **kw)
    for step in range(3):
        _set_grads([pa], step)
        _set_grads([pb], step)
        oa.step()
        ob.step()
    _assert_states_equal(oa, [pa], ob, [pb])
    assert oa.state[pa]["exp_avg_q"].any()


@pytest.mark.parametrize("misaligned", [False, True])
def test_scales_are_group_max_over_448_and_codes_are_neighbours(misaligned):
    """betas = (0.5, 0.5) and dyadic gradients make the fp32 trajectory exactly reproducible (see
    _adam8_refs.dyadic): after each of 5 steps every scale is its group's maximum / 448 exactly and
    every code is a neighbour of the exact value, the exact moments following from decode_states of
    the step before."""
    gen = torch.Generator().manual_seed(3)
    n = 8192 + 1337
    buf = torch.randn(n + 1, device="cuda")
    p = nn.Parameter(buf[1:] if misaligned else buf[1:].clone())
    opt = FusedAdamW([p], lr=1e-3, betas=(0.5, 0.5), state_bits=8, seed=5)
    m_prev, v_prev = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(5):
        g = dyadic(p.shape, gen, "cuda")
        if step == 2:
            g[128:256] = 0  # a group whose moments only decay
        p.grad = g
        opt.step()
        m, v = exact_moments_b05(m_prev, v_prev, g)
        check_shapes(opt.state[p], n)
        check_scales(opt.state[p], m, v.sqrt(), f"step {step + 1}: ")
        check_neighbours(opt.state[p], m, v.sqrt(), f"step {step + 1}: ")
        m_prev, v_prev = opt.decode_states(p)


def _neighbour_run(device, steps, lr=1e-3, decades=0):
    """Default betas, gradients over `decades` decades of magnitude within a group: after every step the
    states are neighbours of the exact moments (fp64, from the previous decoded state). Returns the
    parameter after each step."""
    gen = torch.Generator().manual_seed(4)
    n = 8192 + 4096 + 77
    p = nn.Parameter(torch.randn(n, generator=gen).to(device))
    opt = FusedAdamW([p], lr=lr, weight_decay=0.0, state_bits=8)
    m_prev = torch.zeros(n, dtype=torch.float64, device=device)
    v_prev = torch.zeros(n, dtype=torch.float64, device=device)
    mag = 10.0 ** (-decades * torch.rand(n, generator=gen))
    out = []
    for step in range(steps):
        g = (torch.randn(n, generator=gen) * mag).to(device)
        p.grad = g
        opt.step()
        m = 0.9 * m_prev + (1 - 0.9) * g.double()
        v = 0.999 * v_prev + (1 - 0.999) * g.double() ** 2
        # (fp32 rounding of the update, 6e-8 relative, is far below the 2^-3 / 2^-9 code steps)
        check_neighbours(opt.state[p], m, v.sqrt(), f"{device} step {step + 1}: ")
        m_prev, v_prev = (t.double() for t in opt.decode_states(p))
        out.append(p.detach().clone().cpu())
    return out


def test_neighbour_property_over_six_decades():
    """Elements 10^6 below their group's maximum sit in the subnormal codes or at the smallest code
    (a live s is clamped up to it): still one code step from exact, and never s = 0."""
    _neighbour_run("cuda", 4, decades=6)


def test_gpu_and_cpu_paths_agree_within_the_format_error():
    """Same inputs (unit-variance gradients), 10 steps on each path. The random streams differ by
    design, so nothing is compared bit for bit: each path's states are neighbours of the exact
    moments, and the parameters differ by at most lr (2^-3 + 2^-3) per step (one code step of relative
    error in m and one in s; every element's moments stay in the normal codes after the first step)."""
    lr, steps = 1e-3, 10
    gpu, cpu = _neighbour_run("cuda", steps, lr), _neighbour_run("cpu", steps, lr)
    for k, (a, b) in enumerate(zip(gpu, cpu)):
        d = (a - b).abs().max().item()
        print(f"step {k + 1}: max |p_gpu - p_cpu| = {d:.3e} (bound {(k + 1) * lr * 0.25:.3e})")
        assert d <= (k + 1) * lr * 0.25, (k, d)


def test_stochastic_rounding_is_unbiased():
    """In every group one element has gradient 1.0 and the rest 0.3: after step 1 the exact m of the
    others is 134.4 / 448 of the group's maximum, strictly between the codes 128 and 144. Their mean
    decoded m is within 5 sigma of exact, and both neighbouring codes occur."""
    n = 65536
    g = torch.full((n,), 0.3, device="cuda")
    g[::128] = 1.0
    p = nn.Parameter(torch.zeros(n, device="cuda"))
    opt = FusedAdamW([p], lr=0.0, weight_decay=0.0, state_bits=8, seed=1)
    p.grad = g
    opt.step()
    st = opt.state[p]
    one_minus_b1 = torch.tensor(1.0 - 0.9, dtype=torch.float32)  # formed in fp64 on the host, then rounded
    m_exact = (one_minus_b1 * g.cpu())  # fmaf(b1, 0, (1 - b1) g), fp32
    scale = m_exact[0] / 448.0
    assert torch.equal(st["exp_avg_scale"].cpu(), scale.expand(n // 128))
    small = torch.ones(n, dtype=torch.bool)
    small[::128] = False
    exact = float(m_exact[1].double())
    q = exact / float(scale.double())
    grid = e4m3_values()[:127].double()
    lo_code = int((grid <= q).nonzero().max())
    lo, hi = float(grid[lo_code]) * float(scale), float(grid[lo_code + 1]) * float(scale)
    assert lo < exact < hi and (lo_code, lo_code + 1) == (0x70, 0x71)  # 128 and 144
    codes = st["exp_avg_q"].cpu()[small]
    counts = {c: int((codes == c).sum()) for c in codes.unique().tolist()}
    assert set(counts) == {lo_code, lo_code + 1}, counts
    N = int(small.sum())
    prob = (exact - lo) / (hi - lo)
    sigma = (hi - lo) * math.sqrt(prob * (1 - prob) / N)
    mean = decode(st["exp_avg_q"], st["exp_avg_scale"]).cpu()[small].double().mean().item()
    print(f"p(up) {prob:.4f}, observed {counts[lo_code + 1] / N:.4f}; (mean - exact) / sigma = {(mean - exact) / sigma:.2f}")
    assert abs(mean - exact) <= 5 * sigma, (mean, exact, sigma)
    assert (codes == 0x7E).sum() == 0 and (st["exp_avg_q"].cpu()[~small] == 0x7E).all()


def test_second_moment_decays():
    """One step with g = 1, then 200 steps with g = 0 at beta2 = 0.999 (lr = 0): exact s falls to
    0.999^100 = 0.9048 of its start. Round-to-nearest would leave every code where it is (a code step
    is 6.25 %, one step's decay 0.05 %); with g = 0 the recursion is linear in s, so stochastic
    rounding keeps the mean exact, and over 65,536 elements the mean's sigma is about 0.06 % of s."""
    n = 65536
    p = nn.Parameter(torch.zeros(n, device="cuda"))
    opt = FusedAdamW([p], lr=0.0, betas=(0.9, 0.999), weight_decay=0.0, state_bits=8, seed=2)
    p.grad = torch.ones(n, device="cuda")
    opt.step()
    s0 = opt.decode_states(p)[1].sqrt().double().mean().item()
    assert abs(s0 - math.sqrt(1e-3)) < 1e-6
    p.grad = torch.zeros(n, device="cuda")
    for _ in range(200):
        opt.step()
    ratio = opt.decode_states(p)[1].sqrt().double().mean().item() / s0
    print(f"mean s after 200 zero-gradient steps / start = {ratio:.5f} (exact {0.999 ** 100:.5f})")
    assert abs(ratio - 0.9048) <= 0.01, ratio


def test_determinism_seed_and_launch_grouping():
    """Same seed: bitwise equal states after 5 steps. Another seed: other codes, the same parameters
    at step 1. One step() over all parameters and step_params bucket by bucket, in another order,
    give bitwise equal results (the random bits hang on the parameter's ordinal, not on the launch)."""
    kw = dict(lr=1e-2, weight_decay=0.1, master_weights=True, state_bits=8)
    runs = []
    for seed, bucketed in ((7, False), (7, False), (8, False), (7, True)):
        ps = _params(torch.bfloat16, False)
        opt = FusedAdamW(ps, seed=seed, **kw)
        first = None
        for step in range(5):
            _set_grads(ps, step)
            if bucketed:
                order = [ps[30:], ps[5:30], ps[:5]]
                for chunk in order:
                    opt.step_params(chunk, [q.grad for q in chunk])
            else:
                opt.step()
            if step == 0:
                first = [q.detach().clone() for q in ps]
        runs.append((opt, ps, first))
    (o0, p0, f0), (o1, p1, _), (o2, p2, f2), (o3, p3, _) = runs
    _assert_states_equal(o0, p0, o1, p1)
    _assert_states_equal(o0, p0, o3, p3)
    assert all(torch.equal(a, b) for a, b in zip(f0, f2))
    big = NUMELS.index(3 * 8192 + 130)
    assert not torch.equal(o0.state[p0[big]]["exp_avg_q"], o2.state[p2[big]]["exp_avg_q"])
    assert not torch.equal(o0.state[p0[big]]["exp_avg_sq_q"], o2.state[p2[big]]["exp_avg_sq_q"])


@pytest.mark.parametrize("pieces", SLICINGS)
def test_slices_match_whole_update(pieces):
    (pw, sw), (ps, ss) = run_whole_and_sliced("cuda", pieces)
    assert torch.equal(pw, ps) and torch.isfinite(ps).all()
    for key in STATE_KEYS:
        assert torch.equal(sw[key], ss[key]), key
    assert sw["step"] == ss["step"] == 2


def test_capture_is_refused_before_anything_is_launched():
    p = nn.Parameter(torch.randn(1000, device="cuda"))
    p.grad = torch.randn(1000, device="cuda")
    opt = FusedAdamW([p], state_bits=8)
    before = p.detach().clone()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            opt.step()
    torch.cuda.synchronize()
    assert len(opt.state[p]) == 0 and torch.equal(p, before)
    opt.step()  # outside a capture the same optimizer steps
    assert opt.state[p]["step"] == 1 and not torch.equal(p, before)


@pytest.fixture(scope="module")
def pg():
    from distributeddataparallel_amd import distributed as dist
    from distributeddataparallel_amd.utils.spawn import free_port

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(free_port())
    g = dist.init_process_group("rccl", rank=0, world_size=1, device_id=0)
    yield g
    dist.destroy_process_group()


def test_overlapped_optimizer_matches_step_after_backward(pg, monkeypatch):
    """register_overlapped_optimizer with 8-bit states: the ~300 k-element tail bucket is all-reduced
    in 64 KiB chunks whose boundaries cut parameters at non-multiples of 128 (a bucket slot is only
    16-element aligned), each group is updated by the piece that brings its last element, and three
    steps are bitwise those of the same model stepped by opt.step() after backward."""
    import distributeddataparallel_amd as xddp

    def make():
        torch.manual_seed(0)
        return nn.Sequential(nn.Linear(300, 500), nn.ReLU(), nn.Linear(500, 301), nn.ReLU(),
                             nn.Linear(301, 10)).cuda().to(torch.bfloat16)

    monkeypatch.setenv("XDDP_TAIL_CHUNK_MB", str(1 / 16))
    m1, m2 = make(), make()
    d1 = xddp.DDP(m1, device_ids=[0], gradient_as_bucket_view=True)
    d2 = xddp.DDP(m2, device_ids=[0], gradient_as_bucket_view=True)
    kw = dict(lr=1e-3, weight_decay=0.1, master_weights=True, state_bits=8, seed=4)
    o1, o2 = FusedAdamW(m1.parameters(), **kw), FusedAdamW(m2.parameters(), **kw)
    calls = []
    orig = o1.step_slices
    o1.step_slices = lambda pieces: (calls.append([(p.numel(), lo, hi) for p, _, lo, hi in pieces]), orig(pieces))[1]
    d1.register_overlapped_optimizer(o1)
    g = torch.Generator(device="cuda").manual_seed(1)
    for it in range(3):
        x = torch.randn(8, 300, device="cuda", generator=g).to(torch.bfloat16)
        y = torch.randint(0, 10, (8,), device="cuda", generator=g)
        for d, o, overlapped in ((d1, o1, True), (d2, o2, False)):
            o.zero_grad(set_to_none=True)
            F.cross_entropy(d(x).float(), y).backward()
            if not overlapped:
                o.step()
        torch.cuda.synchronize()
        sliced = [c for c in calls if any(lo != 0 or hi != n for n, lo, hi in c)]
        if it == 2:  # (the buckets are rebuilt after the first iteration)
            assert len(sliced) >= 3, calls
            assert any(lo % 128 or (hi % 128 and hi != n) for c in sliced for n, lo, hi in c), calls
        calls.clear()
    for a, b in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, b)
        for k in STATE_KEYS + ("master",):
            assert torch.equal(o1.state[a][k], o2.state[b][k]), k
