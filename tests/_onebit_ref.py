"""Inputs, a plain-torch statement of the 1-bit wire's rules and the checks shared by the onebit
tests (the HIP kernels and the CPU path of ops.onebit are held to the same ones). Bits and
residuals are compared bitwise in fp32; the scale against an fp64 sum."""
import numpy as np
import torch

import _q8_ref
from distributeddataparallel_amd.ops import onebit

FLT_MAX = torch.finfo(torch.float32).max


def make_input(n, dtype, block, seed):
    """_q8_ref.make_input (Gaussian blocks over the dtype's range, block 1 constant, 2 one-signed,
    4 with a NaN, 6 with +inf) plus, where they fit, an all-zero block 3 and exact +0 / -0 in block 0."""
    x = _q8_ref.make_input(n, dtype, block, seed)
    x[3 * block:4 * block] = 0.0
    x[2:3] = 0.0
    x[5:6] = -0.0
    return x


def make_err(x, block, seed):
    """An fp32 residual of the magnitude of ``x``; zero on blocks 0 and 3 (so v keeps the exact zeros)."""
    g = torch.Generator().manual_seed(seed + 1000)
    e = torch.randn(x.numel(), generator=g) * x.float().abs().nan_to_num(1.0, posinf=1.0)
    e[:block] = 0.0
    e[3 * block:4 * block] = 0.0
    return e


def unpack(payload, block, segments):
    """sign bytes [S * cb, block / 8] uint8 and scales [S * cb] fp32, in block order, on the CPU."""
    seg = payload.cpu().view(segments, -1)
    cb = seg.size(1) // (block // 8 + 4)
    return (seg[:, :cb * block // 8].reshape(-1, block // 8),
            seg[:, cb * block // 8:].contiguous().view(torch.float32).reshape(-1).clone())


def signs(packed, block):
    return torch.from_numpy(np.unpackbits(packed.numpy(), axis=1, bitorder="little")).bool().view(-1, block)


def decoded(packed, scale, block):
    """d [blocks, block] fp32: -scale where the bit is set, +scale elsewhere."""
    return torch.where(signs(packed, block), -scale[:, None], scale[:, None])


def rows(t, total, block):
    v = torch.zeros(total * block, dtype=torch.float32)
    v[:t.numel()] = t.float().cpu()
    return v.view(total, block)


def check_compressed(v, numel, packed, scale, err_before, err_after):
    """``v`` [blocks, block] fp32 (= x + e, zeros from element ``numel`` on) against the payload
    rows and the residual rows before and after the call."""
    total, block = v.shape
    real = (torch.arange(total * block) < numel).view(total, block)
    count = real.sum(1)
    exact = v.double().abs().sum(1)
    live = count > 0
    ok = live & torch.isfinite(v).all(1) & (exact <= FLT_MAX)
    want = np.packbits(((v < 0) & ok[:, None]).numpy(), axis=1, bitorder="little")
    assert torch.equal(packed, torch.from_numpy(want)), "sign bytes differ (padding must be zero)"
    assert torch.isnan(scale[live & ~ok]).all(), "a block with a NaN / inf must store scale = NaN"
    assert not torch.isnan(scale[ok]).any(), "a NaN leaked into a neighbouring block"
    assert (scale[~live] == 0).all(), "padding blocks must have scale 0"
    mean = exact[ok] / count[ok]
    ratio = (scale[ok].double() - mean).abs() / ((count[ok] + 1) * 2.0 ** -24 * mean).clamp_min(1e-300)
    print(f"worst scale error / bound: {ratio.max().item() if ratio.numel() else 0:.4f}")
    assert (ratio <= 1).all()
    zero = ok & (exact == 0)
    assert (scale[zero] == 0).all() and (err_after[zero] == 0).all(), "an all-zero block must stay zero"
    new = torch.where(ok[:, None] & real, v - decoded(packed, scale, block), err_before)
    assert torch.equal(err_after.view(torch.int32), new.view(torch.int32)), \
        "err must be fp32(v - d) on compressed blocks and unchanged on skipped blocks and padding"


def run_compress(device, dtype, n, block, segments, offset=0):
    full = make_input(n + offset, dtype, block, seed=n)
    x, xd = full[offset:], full.to(device)[offset:]  # offset 1: a view one element into its storage
    e0 = make_err(x, block, seed=n)
    err = torch.zeros(n + offset, device=device)[offset:].copy_(e0)
    payload = onebit.compress(xd, err, block, segments)
    assert payload.numel() == onebit.payload_bytes(n, block, segments)
    packed, scale = unpack(payload, block, segments)
    total = packed.size(0)
    check_compressed(rows(x.float() + e0, total, block), n, packed, scale, rows(e0, total, block),
                     rows(err, total, block))
    return payload


def rank_payloads(device, n, block, world):
    """``world`` ranks' one-segment payloads of buckets of ``n`` elements, back to back."""
    parts = []
    for r in range(world):
        x = make_input(n, torch.float32, block, seed=r)
        parts.append(onebit.compress(x.to(device), make_err(x, block, r).to(device), block, 1))
    return torch.cat(parts)


def mean_of(payload, block, world):
    """[blocks * block] fp32: ((d_0 + d_1) + ...) / W in segment order, one division."""
    packed, scale = unpack(payload, block, world)
    d = decoded(packed, scale, block).view(world, -1)
    acc = d[0]
    for r in range(1, world):
        acc = acc + d[r]
    return acc / float(world) if world > 1 else acc


def run_decode_mean(device, world, mode, out_dtype, n, block=512):
    if mode == "mean":
        payload = rank_payloads(device, n, block, world)
        ref = mean_of(payload, block, world)
    else:
        x = make_input(n, torch.float32, block, seed=9)
        payload = onebit.compress(x.to(device), make_err(x, block, 9).to(device), block, world)
        ref = decoded(*unpack(payload, block, world), block).view(-1)
    out = torch.full((n,), 7.0, dtype=out_dtype, device=device)
    onebit.decode_mean(payload, out, block, world, mode)
    got, ref = out.cpu(), ref[:n].to(out_dtype)
    bad = torch.isnan(ref)
    assert bad.any() and not bad.all()
    assert torch.equal(torch.isnan(got), bad), "NaN blocks, and only they, must decode to NaN"
    ints = torch.int32 if out_dtype == torch.float32 else torch.int16
    assert torch.equal(got[~bad].view(ints), ref[~bad].view(ints))


def run_reduce_recompress(device, world, block=512, cb=9):
    """Chunk of 9 blocks: 7 whole, a short one and a padding block (whose incoming bytes are real
    data that the kernel must ignore); block 4 is NaN on every rank."""
    numel = 7 * block + 17
    payload = rank_payloads(device, cb * block, block, world)
    e0 = make_err(make_input(cb * block, torch.float32, block, seed=77), block, 77)
    e0[7 * block:] = 1.5  # the tail's and the padding's residual: must survive where it is padding
    err = e0.clone().to(device)
    out = onebit.reduce_recompress(payload, err, block, world, numel)
    real = torch.arange(cb * block) < numel
    v = torch.where(real, mean_of(payload, block, world) + e0, torch.zeros(()))
    check_compressed(v.view(cb, block), numel, *unpack(out, block, 1), e0.view(cb, block), err.cpu().view(cb, block))


def run_error_feedback(device, block=512, rounds=8):
    """sum_t d_t + e_T = T g up to two fp32 roundings a round: |.| <= T 2^-22 max_t |v_t|."""
    n = 4 * block + 8
    g = make_input(n, torch.float32, block, seed=5).nan_to_num(1.0)
    gd, err, out = g.to(device), torch.zeros(n, device=device), torch.empty(n, device=device)
    total, vmax = torch.zeros(n, dtype=torch.float64), torch.zeros(n)
    for _ in range(rounds):
        vmax = torch.maximum(vmax, (g + err.cpu()).abs())
        onebit.decode_mean(onebit.compress(gd, err, block, 1), out, block, 1, "mean")
        total += out.cpu().double()
    miss = (total + err.cpu().double() - rounds * g.double()).abs()
    bound = rounds * 2.0 ** -22 * vmax.double()
    print(f"worst telescoping error / bound: {(miss / bound.clamp_min(1e-300)).max().item():.4f}")
    assert (miss <= bound).all()
    assert (err != 0).any()


def hook_worker(rank, world, device, algorithm, dtype, rounds=4):
    """Two ranks, a small MLP under DDP with the onebit hook and the same shard every iteration
    (module docstring of test_onebit_hook_gpu.py for the bounds)."""
    import torch.nn as nn
    import torch.nn.functional as F

    import distributeddataparallel_amd as xddp
    from distributeddataparallel_amd import distributed as dist
    from distributeddataparallel_amd.parallel.comm_hooks import OneBitState, onebit_allreduce_hook

    if device == "cuda":
        torch.cuda.set_device(0)

    def mlp():
        torch.manual_seed(0)
        return nn.Sequential(nn.Linear(37, 129), nn.ReLU(), nn.Linear(129, 65), nn.ReLU(),
                             nn.Linear(65, 10)).to(device, dtype)

    def flat_grad(m):
        return torch.cat([p.grad.detach().view(-1) for p in m.parameters()]).double().cpu()

    model, ref = mlp(), mlp()
    ddp = xddp.DDP(model, device_ids=[0] if device == "cuda" else None)
    state, buckets = OneBitState(block=512, algorithm=algorithm, start_iter=1), set()
    ddp.register_comm_hook(state, lambda s, b: (buckets.add(b.index()), onebit_allreduce_hook(s, b))[1])
    g = torch.Generator().manual_seed(3)
    x = torch.randn(world * 8, 37, generator=g).to(device, dtype)
    y = torch.randint(0, 10, (world * 8,), generator=g).to(device)
    shards = []
    for r in range(world):
        ref.zero_grad()
        F.cross_entropy(ref(x[r * 8:(r + 1) * 8]).float(), y[r * 8:(r + 1) * 8]).backward()
        shards.append(flat_grad(ref))
    exact = torch.stack(shards).mean(0)
    outs = []
    for it in range(rounds + 1):
        model.zero_grad()
        F.cross_entropy(ddp(x[rank * 8:(rank + 1) * 8]).float(), y[rank * 8:(rank + 1) * 8]).backward()
        got = flat_grad(model)
        if it == 0:  # warm-up: the plain averaging all-reduce
            assert ((got - exact).abs() <= _q8_ref.ulp(exact, dtype)).all(), f"rank {rank}: warm-up is not the mean"
            continue
        outs.append(got)
        both = torch.empty(world * got.numel(), device=device)
        dist.all_gather_into_tensor(both, got.float().to(device))
        assert torch.equal(both.view(world, -1)[0], both.view(world, -1)[1]), f"it {it}: gradients differ across ranks"
    assert state.iter == rounds + 1
    ew = max(state.worker_error(i).abs().max().item() for i in buckets)
    es = max(state.server_error(i).abs().max().item() for i in buckets) if algorithm == "twoshot" else 0.0
    stats = torch.tensor([ew, es], device=device)
    every = torch.empty(world * 2, device=device)
    dist.all_gather_into_tensor(every, stats)
    every = every.view(world, 2).double().cpu()
    ew_mean, ew_max, es_max = every[:, 0].mean().item(), every[:, 0].max().item(), every[:, 1].max().item()
    assert ew_max > 0 and (es_max > 0) == (algorithm == "twoshot"), "the residuals are not in use"
    outs = torch.stack(outs)
    vmax = max(s.abs().max().item() for s in shards) + ew_max + outs.abs().max().item() + es_max
    bound = ((ew_mean + es_max) / rounds + _q8_ref.ulp(outs.abs().amax(0).clamp_min(1e-300), dtype)
             + rounds * 2.0 ** -22 * vmax)
    miss = (outs.mean(0) - exact).abs()
    first, mean = (outs[0] - exact).norm().item(), (outs.mean(0) - exact).norm().item()
    print(f"rank {rank} {algorithm} {dtype}: worst error / bound {(miss / bound).max().item():.4f}; "
          f"l2 error of out_1 {first:.4e}, of the mean of {rounds} {mean:.4e}; |exact| {exact.norm().item():.4e}")
    assert (miss <= bound).all()
    assert mean < first, "error feedback must bring the running mean closer than one compressed step"
