"""Inputs, a plain-torch statement of the top-k wire's rules and the checks shared by the topk tests
(the HIP kernels and the CPU path of ops.topk are held to the same ones). Everything on this wire
is exact, so offsets, values, residuals and decoded buckets are compared bitwise."""
import torch

import _q8_ref
from distributeddataparallel_amd.ops import topk

CASES = [(1024, 8), (2048, 32), (4096, 64)]  # (block, k)
EMPTY = 0xFFFF


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def make_input(n, dtype, block, k, variant, seed=0):
    """Small Gaussian blocks (|x| < 0.9) and, where they fit, per variant:
    0: block 0 has k / 2 elements of |x| >= 4 and exactly k + 3 of |x| = 1 with mixed signs, block 1
       is one repeated value, block 2 holds a NaN;
    1: block 0 is all zero with a -0 in it, block 1 holds +inf."""
    g = torch.Generator().manual_seed(seed)
    nb = max(-(-n // block), 3)
    x = (torch.randn(nb, block, generator=g) * 0.1).clamp(-0.9, 0.9)
    if variant == 0:
        at = torch.randperm(block, generator=g)
        x[0, at[:k // 2]] = 4.0 + 0.5 * torch.arange(k // 2)
        x[0, at[k // 2:k // 2 + k + 3]] = torch.where(torch.arange(k + 3) % 3 == 0, -1.0, 1.0)
        x[1] = 3.25
        x[2, 3] = float("nan")
    else:
        x[0] = 0.0
        x[0, 5] = -0.0
        x[1, 7] = float("inf")
    return x.view(-1)[:n].to(dtype)


def make_err(n, block, seed=0):
    """A non-zero fp32 residual; zero on blocks 0 and 1, whose ties and zeros v must keep."""
    e = torch.randn(n, generator=torch.Generator().manual_seed(seed + 1000)) * 0.05
    e[:2 * block] = 0.0
    return e


def select(v, c, k):
    """The rules for one block: ``v`` [block] fp32 with ``c`` real elements -> offsets [k] int32,
    values [k] fp32, the new residual [block] and whether the block was skipped."""
    off, val = torch.full((k,), EMPTY, dtype=torch.int32), torch.zeros(k)
    if not torch.isfinite(v[:c]).all():
        return off, torch.full((k,), float("nan")), v, True
    key = v[:c].abs().view(torch.int32)  # monotone in |v|; a stable sort gives ties to the lower index
    top = torch.sort(key, descending=True, stable=True).indices[:k].sort().values
    off[:top.numel()], val[:top.numel()] = top.to(torch.int32), v[top]
    new = v.clone()
    new[top] = 0.0
    return off, val, new, False


def unpack(payload, k, segments):
    """offsets [S * cb, k] int32 and values [S * cb, k] fp32, in block order, on the CPU."""
    seg = payload.cpu().view(segments, -1)
    cbk = seg.size(1) // 6
    val = seg[:, :cbk * 4].contiguous().view(torch.float32).reshape(-1, k)
    return seg[:, cbk * 4:].contiguous().view(torch.int16).reshape(-1, k).to(torch.int32) & 0xFFFF, val.clone()


def dense(off, val, block):
    """d [blocks, block] fp32: a block's slots at their offsets, +0 elsewhere, NaN on skipped blocks."""
    d = torch.zeros(off.size(0), block)
    for row, (o, x) in enumerate(zip(off, val)):
        d[row, o[o != EMPTY].long()] = x[o != EMPTY]
        if o[0] == EMPTY and torch.isnan(x[0]):
            d[row] = float("nan")
    return d


def mean_of(payload, block, k, world):
    """[blocks * block] fp32: ((d_0 + d_1) + ...) / W in segment order, one division."""
    d = dense(*unpack(payload, k, world), block).view(world, -1)
    acc = d[0]
    for r in range(1, world):
        acc = acc + d[r]
    return acc / float(world) if world > 1 else acc


def rows(t, total, block):
    v = torch.zeros(total * block, dtype=torch.float32)
    v[:t.numel()] = t.float().cpu()
    return v.view(total, block)


def check_selected(v, numel, k, off, val, err_before, err_after):
    """``v`` [blocks, block] fp32 (zeros from element ``numel`` on) against the payload rows and the
    residual rows before and after the call. Returns the rows that were skipped."""
    total, block = v.shape
    skipped = []
    for b in range(total):
        c = min(max(numel - b * block, 0), block)
        o, x, new, bad = select(v[b], c, k)
        assert torch.equal(off[b], o), f"block {b}: offsets {off[b].tolist()} != {o.tolist()}"
        assert torch.equal(bits(val[b]), bits(x)), f"block {b}: values differ"
        want = err_before[b] if bad else torch.where(torch.arange(block) < c, new, err_before[b])
        assert torch.equal(bits(err_after[b]), bits(want)), \
            f"block {b}: err must be 0 / v on a selected block and unchanged on skipped blocks and padding"
        skipped.append(bad)
    return torch.tensor(skipped)


def run_compress(device, dtype, block, k, n, segments, offset=0, variant=0):
    full = make_input(n + offset, dtype, block, k, variant, seed=n)
    x, xd = full[offset:], full.to(device)[offset:]  # offset 1: a view one element into its storage
    e0 = make_err(n, block, seed=n)
    err = torch.zeros(n + offset, device=device)[offset:].copy_(e0)
    payload = topk.compress(xd, err, block, k, segments)
    assert payload.numel() == topk.payload_bytes(n, block, k, segments)
    off, val = unpack(payload, k, segments)
    total, v = off.size(0), x.float() + e0
    bad = check_selected(rows(v, total, block), n, k, off, val, rows(e0, total, block), rows(err, total, block))
    if variant == 0 and n >= 2 * block:
        assert off[1].tolist() == list(range(k)), "a block of one repeated value keeps its first k elements"
    if device != "cpu":
        cpu = topk.compress(x.clone(), e0.clone(), block, k, segments)
        assert torch.equal(payload.cpu(), cpu), "the kernel's payload differs from the CPU path's"
    if dtype == torch.float32:  # nothing is rounded: decoded + e_new is v, except that -0 comes back as +0
        out = torch.full((n,), 7.0, device=device)
        topk.decode_mean(payload, out, block, k, segments, "concat")
        fine = ~bad[:, None].expand(-1, block).reshape(-1)[:n]
        assert torch.equal(bits((out.cpu() + err.cpu())[fine]), bits((v + 0.0)[fine]))
    return payload


def rank_inputs(n, block, k, world):
    """``world`` ranks' fp32 buckets: rank 0 is variant 0 (NaN in block 2), the others are it with the
    NaN replaced and every element scaled by its own 1 + 0.5 N(0, 1), so selections partly overlap."""
    base = make_input(n, torch.float32, block, k, 0, seed=n)
    noise = [1 + 0.5 * torch.randn(n, generator=torch.Generator().manual_seed(r)) for r in range(world)]
    return [base] + [base.nan_to_num(0.3) * noise[r] for r in range(1, world)]


def rank_payloads(device, n, block, k, world):
    """The ranks' one-segment payloads, back to back."""
    return torch.cat([topk.compress(x.to(device), make_err(n, block, r).to(device), block, k, 1)
                      for r, x in enumerate(rank_inputs(n, block, k, world))])


def run_decode_mean(device, world, mode, out_dtype, block, k):
    n = 3 * block + 17
    if mode == "mean":
        payload = rank_payloads(device, n, block, k, world)
        ref = mean_of(payload, block, k, world)
        if world > 1:
            hits = (dense(*unpack(payload, k, world), block).view(world, -1).nan_to_num(0.0) != 0).sum(0)
            assert (hits == 1).any() and (hits > 1).any(), "the ranks' selections must partly overlap"
    else:
        x = make_input(n, torch.float32, block, k, 0, seed=9)
        payload = topk.compress(x.to(device), make_err(n, block, 9).to(device), block, k, world)
        ref = dense(*unpack(payload, k, world), block).view(-1)
    out = torch.full((n,), 7.0, dtype=out_dtype, device=device)
    topk.decode_mean(payload, out, block, k, world, mode)
    got, ref = out.cpu(), ref[:n].to(out_dtype)
    bad = torch.isnan(ref)
    assert torch.equal(bad, (torch.arange(n) // block) == 2), "block 2, and only it, is NaN on rank 0"
    assert torch.equal(torch.isnan(got), bad), "NaN blocks, and only they, must decode to NaN"
    assert torch.equal(bits(got[~bad]), bits(ref[~bad])), "unselected elements are exactly 0, the others the mean"


def run_reduce_reselect(device, world, block, k, cb=9):
    """Chunk of 9 blocks: 7 whole, a short one and a padding block (whose incoming bytes are real
    data that the kernel must ignore); block 2 is NaN on rank 0."""
    numel = 7 * block + 17
    payload = rank_payloads(device, cb * block, block, k, world)
    e0 = torch.randn(cb * block, generator=torch.Generator().manual_seed(77)) * 0.05
    e0[7 * block:] = 1.5  # the tail's and the padding's residual: must survive where it is padding
    err = e0.clone().to(device)
    out = topk.reduce_reselect(payload, err, block, k, world, numel)
    real = torch.arange(cb * block) < numel
    u = torch.where(real, mean_of(payload, block, k, world) + e0, torch.zeros(()))
    bad = check_selected(u.view(cb, block), numel, k, *unpack(out, k, 1), e0.view(cb, block),
                         err.cpu().view(cb, block))
    assert bad.tolist() == [b == 2 for b in range(cb)]


def hook_worker(rank, world, device, algorithm, dtype, rounds=4):
    """Two ranks, a small MLP under DDP with the topk hook and the same shard every iteration
    (module docstring of test_topk_hook_gpu.py for the bounds)."""
    import torch.nn as nn
    import torch.nn.functional as F

    import distributeddataparallel_amd as xddp
    from distributeddataparallel_amd import distributed as dist
    from distributeddataparallel_amd.parallel.comm_hooks import TopKState, topk_allreduce_hook

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
    state, buckets = TopKState(block=1024, k=64, algorithm=algorithm, start_iter=1), set()
    ddp.register_comm_hook(state, lambda s, b: (buckets.add(b.index()), topk_allreduce_hook(s, b))[1])
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
    every = torch.empty(world * 2, device=device)
    dist.all_gather_into_tensor(every, torch.tensor([ew, es], device=device))
    every = every.view(world, 2).double().cpu()
    ew_mean, ew_max, es_max = every[:, 0].mean().item(), every[:, 0].max().item(), every[:, 1].max().item()
    assert ew_max > 0 and (es_max > 0) == (algorithm == "twoshot"), "the residuals are not in use"
    outs = torch.stack(outs)
    vmax = max(s.abs().max().item() for s in shards) + ew_max + outs.abs().max().item() + es_max
    bound = ((ew_mean + es_max) / rounds + _q8_ref.ulp(outs.abs().amax(0).clamp_min(1e-300), dtype)
             + rounds * 2.0 ** -22 * vmax)
    miss = (outs.mean(0) - exact).abs()
    print(f"rank {rank} {algorithm} {dtype}: worst error / bound {(miss / bound).max().item():.4f}")
    assert (miss <= bound).all()
