"""Inputs, an fp64 reading of the q8 payload and the bounds shared by the q8 tests (GPU kernels and
CPU fallbacks are held to the same ones)."""
import torch

from distributeddataparallel_amd.ops import q8


def make_input(n, dtype, block, seed):
    """Gaussian blocks whose magnitudes span the dtype's range (|x| >= 1e-30), and where they fit:
    block 1 constant, block 2 one-signed far from 0, block 4 with a NaN, block 6 with +inf."""
    g = torch.Generator().manual_seed(seed)
    nb = -(-n // block)
    lo, hi = (-4, 3) if dtype == torch.float16 else (-6, 6)
    x = torch.randn(nb, block, generator=g) * torch.logspace(lo, hi, nb)[torch.randperm(nb, generator=g), None]
    x = torch.where(x < 0, -1.0, 1.0) * x.abs().clamp_min(1e-30)
    if nb > 1:
        x[1] = 3.25
    if nb > 2:
        x[2] = 1000 + 1e-3 * torch.rand(block, generator=g)
    if nb > 4:
        x[4, 3] = float("nan")
    if nb > 6:
        x[6, 5] = float("inf")
    return x.view(-1)[:n].to(dtype)


def unpack(payload, block, segments):
    """codes [S * cb, block] uint8, lo and scale [S * cb] fp32, in block order, on the CPU."""
    seg = payload.cpu().view(segments, -1)
    cb = seg.size(1) // (block + 8)
    p = seg[:, cb * block:].contiguous().view(torch.float32).view(-1, 2)
    return seg[:, :cb * block].reshape(-1, block), p[:, 0].clone(), p[:, 1].clone()


def decode(codes, lo, scale):
    return codes.double() * scale.double()[:, None] + lo.double()[:, None]


def ulp(v, dtype):
    """One unit in the last place of ``dtype`` at fp64 ``v``."""
    bits = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}[dtype]
    return torch.ldexp(torch.ones_like(v), torch.frexp(v)[1] - bits)


def check_quantized(v, n, codes, lo, scale, exact_params):
    """``v`` [blocks, block] fp64 (zeros past element n) against its quantized form."""
    total, block = v.shape
    nb = -(-n // block)
    real = (torch.arange(total * block) < n).view(total, block)
    v32 = v.float()
    mn = torch.where(real, v32, float("inf")).amin(1)
    rng = torch.where(real, v32, -float("inf")).amax(1) - mn
    live = torch.arange(total) < nb
    ok = live & torch.isfinite(torch.where(real, v, 0.0)).all(1) & torch.isfinite(rng)
    assert torch.isnan(scale[live & ~ok]).all(), "a block with a NaN / inf must store scale = NaN"
    assert not torch.isnan(scale[ok]).any(), "a NaN leaked into a neighbouring block"
    assert (codes[~real] == 0).all() and (lo[~live] == 0).all() and (scale[~live] == 0).all(), "padding is not zero"
    if exact_params:
        assert torch.equal(lo[ok].view(torch.int32), mn[ok].view(torch.int32)), "lo is not the block minimum"
        assert torch.equal(scale[ok].view(torch.int32), (rng / 255.0)[ok].view(torch.int32)), "scale != (hi - lo) / 255"
    bound = 0.5 * scale.double() * (1 + 1e-4) + 4 * 2.0 ** -23 * torch.where(real, v.abs(), 0.0).amax(1)
    ratio = ((decode(codes, lo, scale) - v).abs() / bound[:, None])[ok][real[ok]]
    print(f"worst decode error / bound: {ratio.max().item():.4f}")
    assert (ratio <= 1).all()
    if exact_params:
        const = ok & (rng == 0)
        assert torch.equal(decode(codes, lo, scale)[const][real[const]], v[const][real[const]]), \
            "a constant block must decode exactly"


def blocks_of(x, total, block):
    v = torch.zeros(total * block, dtype=torch.float64)
    v[:x.numel()] = x.double().cpu()
    return v.view(total, block)


def run_quantize(device, dtype, n, block, segments, offset=0):
    x = make_input(n + offset, dtype, block, seed=n).to(device)[offset:]
    payload = q8.quantize(x, block, segments)
    assert payload.numel() == q8.payload_bytes(n, block, segments)
    codes, lo, scale = unpack(payload, block, segments)
    check_quantized(blocks_of(x, codes.size(0), block), n, codes, lo, scale, exact_params=True)


def _mean_payload(device, n, block, world):
    """``world`` ranks' one-segment payloads of the same bucket, back to back, and their fp64 mean."""
    parts = [q8.quantize(make_input(n, torch.float32, block, seed=r).to(device), block, 1) for r in range(world)]
    dec = torch.stack([decode(*unpack(p, block, 1)) for p in parts])
    mag = torch.stack([unpack(p, block, 1)[1].abs().double() + 255 * unpack(p, block, 1)[2].abs().double()
                       for p in parts]).mean(0)
    return torch.cat(parts), dec.mean(0), mag


def run_dequantize_mean(device, world, mode, out_dtype, n, block=512):
    if mode == "mean":
        payload, ref, mag = _mean_payload(device, n, block, world)
    else:
        payload = q8.quantize(make_input(n, torch.float32, block, seed=9).to(device), block, world)
        codes, lo, scale = unpack(payload, block, world)
        ref, mag = decode(codes, lo, scale), lo.abs().double() + 255 * scale.abs().double()
    out = torch.full((n,), 7.0, dtype=out_dtype, device=device)
    q8.dequantize_mean(payload, out, block, world, mode)
    got, ref = out.cpu().double(), ref.view(-1)[:n]
    if out_dtype == torch.float32:
        tol = (2.0 ** -22 * mag)[:, None].expand(-1, block).reshape(-1)[:n]
    else:  # one ulp around the correctly rounded value
        ref = ref.to(out_dtype).double()
        tol = ulp(ref, out_dtype)
    bad = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), bad), "NaN blocks, and only they, must decode to NaN"
    ratio = ((got - ref).abs() / tol)[~bad]
    print(f"worst error / bound: {ratio.max().item():.4f}")
    assert (ratio <= 1).all()


def run_reduce_requantize(device, world, n, block=512):
    payload, mean, _ = _mean_payload(device, n, block, world)
    out = q8.reduce_requantize(payload, block, world)
    assert out.numel() * world == payload.numel()
    check_quantized(mean, mean.numel(), *unpack(out, block, 1), exact_params=False)


def hook_worker(rank, world, device, algorithm, dtype):
    """Two ranks, a small MLP under DDP with the q8 hook: every gradient within the format's bound
    of the exact mean over the shards, and bitwise equal on both ranks."""
    import torch.nn as nn
    import torch.nn.functional as F

    import distributeddataparallel_amd as xddp
    from distributeddataparallel_amd import distributed as dist
    from distributeddataparallel_amd.parallel.comm_hooks import Q8State, q8_allreduce_hook

    if device == "cuda":
        torch.cuda.set_device(0)

    def mlp():
        torch.manual_seed(0)
        return nn.Sequential(nn.Linear(37, 129), nn.ReLU(), nn.Linear(129, 65), nn.ReLU(),
                             nn.Linear(65, 10)).to(device, dtype)

    model, ref = mlp(), mlp()
    ddp = xddp.DDP(model, device_ids=[0] if device == "cuda" else None)
    ddp.register_comm_hook(Q8State(block=128, algorithm=algorithm), q8_allreduce_hook)
    g = torch.Generator().manual_seed(3)
    for it in range(2):  # the second backward runs on the rebuilt buckets and the cached payloads
        x = torch.randn(world * 8, 37, generator=g).to(device, dtype)
        y = torch.randint(0, 10, (world * 8,), generator=g).to(device)
        model.zero_grad()
        F.cross_entropy(ddp(x[rank * 8:(rank + 1) * 8]).float(), y[rank * 8:(rank + 1) * 8]).backward()
        shards = []
        for r in range(world):
            ref.zero_grad()
            F.cross_entropy(ref(x[r * 8:(r + 1) * 8]).float(), y[r * 8:(r + 1) * 8]).backward()
            shards.append([p.grad.detach().double().cpu() for p in ref.parameters()])
        spread = max((torch.cat([t.view(-1) for t in s]).max() - torch.cat([t.view(-1) for t in s]).min()).item()
                     for s in shards)
        for i, (name, p) in enumerate(model.named_parameters()):
            exact = torch.stack([s[i] for s in shards]).mean(0)
            err = (p.grad.double().cpu() - exact).abs()
            bound = spread / 255 * (1 + 1e-3) + ulp(exact, dtype)
            assert (err <= bound).all(), f"rank {rank} it {it} {name}: {(err / bound).max().item():.3f} x bound"
        flat = torch.cat([p.grad.detach().float().view(-1) for p in model.parameters()])
        both = torch.empty(world * flat.numel(), device=device)
        dist.all_gather_into_tensor(both, flat)
        assert torch.equal(both.view(world, -1)[0], both.view(world, -1)[1]), "gradients differ across ranks"
