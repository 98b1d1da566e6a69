"""Inputs and the fp64 reference shared by the window-attention tests (CPU tensors throughout)."""
import torch


def make(Bw, N, H, nW, bias_dtype, dtype=torch.bfloat16, D=32, seed=0):
    """qkv [Bw, N, 3, H, D], bias [H, N, N] or None, labels int32 [nW, N] or None (nW == 0), dO, scale.
    Labels are random in {0, 1, 2}: a token always sees itself, so no row is empty."""
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(Bw, N, 3, H, D, generator=gen).to(dtype)
    bias = None if bias_dtype is None else torch.randn(H, N, N, generator=gen).to(bias_dtype)
    labels = torch.randint(0, 3, (nW, N), generator=gen, dtype=torch.int32) if nW else None
    d_out = torch.randn(Bw, N, H, D, generator=gen).to(dtype)
    return qkv, bias, labels, d_out, D ** -0.5


def reference(qkv, bias, labels, d_out, scale, absolute=False):
    """fp64 from the rounded inputs, masked keys at -inf. Returns (o, dqkv, dbias, sum_w |dS|): o
    [Bw, N, H, D], dqkv in qkv's layout, both by autograd. With ``absolute`` the same formulas on
    absolute values with the true P (the magnitude each result's terms add up to): o = P |V|,
    dv = P^T |dO|, dq = scale G |K|, dk = scale G^T |Q| with G = P (|dO| |V|^T + sum_j P (|dO| |V|^T));
    dbias is None and the last entry sum_w G (what dS = P (dP - delta) is a difference of)."""
    Bw, N, _, H, _ = qkv.shape
    x = qkv.double().requires_grad_(not absolute)
    b = None if bias is None else bias.double().requires_grad_(not absolute)
    q, k, v = x.permute(2, 0, 3, 1, 4)  # [Bw, H, N, D]
    s = q @ k.transpose(-1, -2) * scale
    if b is not None:
        s = s + b
    if labels is not None:
        nW = labels.size(0)
        same = labels[:, :, None] == labels[:, None, :]
        s = s.view(Bw // nW, nW, H, N, N).masked_fill(~same[None, :, None], float("-inf")).view(Bw, H, N, N)
    p = torch.softmax(s, -1)
    g = d_out.double().transpose(1, 2)
    if not absolute:
        o = (p @ v).transpose(1, 2)
        o.backward(d_out.double())
        p, v = p.detach(), v.detach()
        dp = g @ v.transpose(-1, -2)
        ds = p * (dp - (p * dp).sum(-1, keepdim=True))
        return o.detach(), x.grad, None if b is None else b.grad, ds.abs().sum(0)
    g, q, k, v = g.abs(), q.abs(), k.abs(), v.abs()
    dp = g @ v.transpose(-1, -2)
    G = p * (dp + (p * dp).sum(-1, keepdim=True))
    parts = (scale * G @ k, scale * G.transpose(-1, -2) @ q, p.transpose(-1, -2) @ g)
    return (p @ v).transpose(1, 2), torch.stack(parts, 0).permute(1, 3, 0, 2, 4), None, G.sum(0)
