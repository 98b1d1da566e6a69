"""fp64 references and per-element / per-column error bounds for the row kernels (LayerNorm /
RMSNorm, softmax cross-entropy, RoPE, SwiGLU, GELU, bias_grad).

Every reference is a plain fp64 PyTorch computation that starts from the rounded inputs the kernel
sees (the bf16 / fp16 / fp32 tensors upcast to fp64). It runs wherever its inputs live.

Bounds (never a norm ratio over a whole tensor):

* element:     |got - ref| <= u * |ref| + c * 2^-24 * scale
* column sum:  |got - ref| <= u * |ref| + c * 2^-24 * sum_rows |term|

``u`` is one ulp of the storage type relative to the value (2^-7 bf16, 2^-10 fp16, 0 for fp32);
below the type's smallest normal number the ulp stops shrinking, so u |ref| is max(u |ref|, the
type's subnormal spacing) throughout.
``scale`` is, per element, the magnitude of the terms the operation adds up in fp32 (written next
to each reference below), so ``c`` counts fp32 roundings. Each ``c`` in ``C`` is 4 x the largest
error, in those units, of the ordinary fp32 torch implementation of the same operation against the
fp64 reference (measured on the CPU at the shapes and input distributions the GPU tests use; the
figure stands beside each entry). The factor 4 is for another summation order and for
``__expf`` / ``rsqrtf``. The kernels under test were never used to set a figure.
"""
import torch
import torch.nn.functional as F

U = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 0.0}
SUB = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24, torch.float32: 0.0}  # subnormal spacing
EPS32 = 2.0 ** -24
FLT_MIN = 2.0 ** -126

# 4 x (max over elements of |fp32 torch - fp64| / (2^-24 * scale)); the measured maximum in brackets
C = {
    "ln_y": 4 * 5.8,        # F.layer_norm / x * rsqrt(mean(x^2) + eps) * w           [5.77]
    "ln_mean": 4 * 1.7,     # native_layer_norm's mean                                 [1.63]
    "ln_rstd": 4 * 3.4,     # native_layer_norm's rstd / rsqrt(mean(x^2) + eps)        [3.31]
    "ln_dx": 4 * 4.1,       # autograd of the above (+ res in fp32)                    [4.06]
    "ln_col": 4 * 3.9,      # dgamma, dbeta of the above; fp32 sum(0) of res and dx    [3.81]
    "xent_lse": 4 * 1.5,    # torch.logsumexp                                          [1.45]
    "xent_loss": 4 * 1.7,   # logsumexp - x[target] per row [1.43]; F.cross_entropy's mean [1.66]
    "xent_grad": 4 * 2.0,   # autograd of F.cross_entropy                              [1.93]
    "rope": 4 * 2.0,        # x0 * c - x1 * s, x0 * s + x1 * c                         [1.96]
    "swiglu": 4 * 3.0,      # F.silu(a) * b                                            [2.97]
    "swiglu_da": 4 * 4.0,   # autograd of F.silu(a) * b                                [4.00]
    "swiglu_db": 4 * 3.1,   #                                                          [3.05]
    "gelu": 4 * 5.9,        # F.gelu                                                   [5.84]
    "dgelu": 4 * 4.8,       # autograd of F.gelu                                       [4.78]
    "bias_col": 4 * 2.5,    # fp32 sum(0) of g [0.68] and of autograd's g * gelu'(h)   [2.48]
}


def elem_bound(ref, dtype, c, scale=None):
    ref = ref.double()
    scale = ref.abs() if scale is None else scale.double()
    return (U[dtype] * ref.abs()).clamp_min(SUB[dtype]) + c * EPS32 * scale


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (inf where got is NaN / inf and ref is not, or the
    bound is zero and the values differ)"""
    got, ref = got.double().reshape(ref.shape), ref.double()
    err = (got - ref).abs()
    r = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(r), r)
    return r


def check(name, got, ref, bound):
    """Assert |got - ref| <= bound everywhere; print the worst ratio first (visible with -s)."""
    assert tuple(got.shape) == tuple(ref.shape), f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    r = ratio(got, ref, bound)
    worst = r.max().item() if r.numel() else 0.0
    print(f"{name}: max |err| / bound = {worst:.3f}")
    if not worst <= 1.0:
        i = int(r.flatten().argmax())
        g, f, b = got.flatten()[i].item(), ref.flatten()[i].item(), bound.flatten()[i].item()
        n = int((r > 1).sum())
        raise AssertionError(f"{name}: {n} of {r.numel()} elements out of bound; worst at flat index {i}: "
                             f"got {g!r}, ref {f!r}, |err| {abs(g - f):.3e} > bound {b:.3e}")


def check_elem(name, got, ref, dtype, c, scale=None):
    check(name, got, ref, elem_bound(ref, dtype, c, scale))


def check_colsum(name, got, ref, sum_abs, dtype, c):
    """Per-column bound of a sum over rows: u |ref| + c 2^-24 sum_r |term_r|."""
    check(name, got, ref, (U[dtype] * ref.double().abs()).clamp_min(SUB[dtype]) + c * EPS32 * sum_abs.double())


# ---- LayerNorm / RMSNorm ---------------------------------------------------------------------
def norm_ref(x, w, b, eps, rms, dy=None, res=None):
    """fp64 LayerNorm / RMSNorm over the last dim of x [rows, D] and, with dy, its backward by
    autograd; with res the gradient of ``norm(x) . dy + x . res`` (the residual form: dx += res).

    Scales (the fp32 term): y: |w| rstd (|x| + |mean|) + |b| (x - mean is a difference of those);
    mean: mean_j |x_j|; rstd: rstd (1 + 2^-23 (rstd mean_j |x_j|)^2): the relative rounding, plus the
    second-order term a two-pass variance keeps of the mean's own rounding (sum (x - m')^2 =
    sum (x - m)^2 + D (m - m')^2: invisible unless the common offset is ~10^4 standard deviations;
    a one-pass E[x^2] - E[x]^2 has a first-order term instead and misses this by far); dx: rstd (|gy| + mean_j |gy_j| + |xh| mean_j |gy_j xh_j|) + |res|
    with gy = dy w and xh the normalised x: the terms of the backward formula, taken absolutely.
    Column sums carry sum_r |term_r|: dgamma |dy xh|, dbeta |dy|, sum res |res|, sum dx |dx|."""
    x64 = x.double().requires_grad_(dy is not None)
    w64 = None if w is None else w.double().requires_grad_(dy is not None)
    b64 = None if b is None else b.double().requires_grad_(dy is not None)
    mean = torch.zeros_like(x64[:, :1]) if rms else x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    xh = (x64 - mean) * rstd
    y = xh if w64 is None else xh * w64
    if b64 is not None:
        y = y + b64
    wa = torch.ones_like(x64[0]) if w is None else w.double().abs()
    o = {"y": y.detach(), "mean": mean.detach()[:, 0], "rstd": rstd.detach()[:, 0],
         "y_scale": (wa * rstd * (x64.abs() + mean.abs())).detach() + (0 if b is None else b.double().abs()),
         "mean_scale": x64.detach().abs().mean(-1)}
    o["rstd_scale"] = o["rstd"] * (1 + 2 * EPS32 * (o["rstd"] * o["mean_scale"]) ** 2) if not rms else o["rstd"]
    if dy is None:
        return o
    dy64 = dy.double()
    loss = (y * dy64).sum()
    if res is not None:
        loss = loss + (x64 * res.double()).sum()
    loss.backward()
    xh = xh.detach()
    gy = dy64 if w is None else dy64 * w.double()
    r = rstd.detach()
    o["dx"] = x64.grad
    o["dx_scale"] = r * (gy.abs() + gy.abs().mean(-1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(-1, keepdim=True))
    if res is not None:
        o["dx_scale"] = o["dx_scale"] + res.double().abs()
        o["sres"], o["sres_abs"] = res.double().sum(0), res.double().abs().sum(0)
        o["sdx"], o["sdx_abs"] = o["dx"].sum(0), o["dx"].abs().sum(0)
    if w64 is not None:
        o["dgamma"], o["dgamma_abs"] = w64.grad, (dy64 * xh).abs().sum(0)
    if b64 is not None:
        o["dbeta"], o["dbeta_abs"] = b64.grad, dy64.abs().sum(0)
    return o


def norm_torch32(x, w, b, eps, rms, dy=None, res=None):
    """The ordinary fp32 torch implementation of the same (the yardstick the C figures come from,
    and the stand-in for the kernel in the CPU test): same keys as norm_ref, fp32."""
    x32 = x.detach().clone().float().requires_grad_(dy is not None)
    w32 = None if w is None else w.detach().clone().float().requires_grad_(dy is not None)
    b32 = None if b is None else b.detach().clone().float().requires_grad_(dy is not None)
    D = x.shape[-1]
    if rms:
        rstd = torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + eps)
        y = x32 * rstd
        y = y if w32 is None else y * w32
        o = {"y": y.detach(), "rstd": rstd.detach()[:, 0]}
    else:
        y, mean, rstd = torch.native_layer_norm(x32, (D,), w32, b32, eps)
        o = {"y": y.detach(), "mean": mean.detach().reshape(-1), "rstd": rstd.detach().reshape(-1)}
    if dy is None:
        return o
    y.backward(dy.float())
    o["dx"] = x32.grad if res is None else x32.grad + res.float()
    if res is not None:
        o["sres"], o["sdx"] = res.float().sum(0), o["dx"].sum(0)
    if w32 is not None:
        o["dgamma"] = w32.grad
    if b32 is not None:
        o["dbeta"] = b32.grad
    return o


def check_norm(tag, got, ref, xdt, wdt):
    """got: dict with any of norm_ref's keys (kernel outputs); x-like outputs are stored as xdt,
    parameter-like ones (dgamma, dbeta, the two sums) as wdt, mean / rstd as fp32."""
    for k, v in got.items():
        if v is None:
            continue
        if k == "y":
            check_elem(f"{tag} y", v, ref["y"], xdt, C["ln_y"], ref["y_scale"])
        elif k == "mean":
            check_elem(f"{tag} mean", v, ref["mean"], torch.float32, C["ln_mean"], ref["mean_scale"])
        elif k == "rstd":
            check_elem(f"{tag} rstd", v, ref["rstd"], torch.float32, C["ln_rstd"], ref["rstd_scale"])
        elif k == "dx":
            check_elem(f"{tag} dx", v, ref["dx"], xdt, C["ln_dx"], ref["dx_scale"])
        else:
            check_colsum(f"{tag} {k}", v, ref[k], ref[k + "_abs"], wdt, C["ln_col"])


# ---- softmax cross-entropy ---------------------------------------------------------------------
def xent_ref(logits, target, ignore_index=-100, g=1.0):
    """fp64 per-row lse and loss (0 on ignored rows), their mean over the non-ignored rows (the
    divisor clamped to 1, as ops.cross_entropy documents) and the gradient (softmax - onehot) g / count.

    Scales: lse: |lse| + 1 (the rounding of max + log(sum), and the relative error of the sum, which
    is absolute in the log); loss: |lse| + |x_t| + 1; gradient: (softmax + onehot) |g| / count x
    (1 + |x| + |lse|): exp(x - lse) has condition number |x - lse| on an argument formed in fp32."""
    x = logits.double()
    R, V = x.shape
    lse = torch.logsumexp(x, -1)
    keep = target != ignore_index
    t = torch.where(keep, target, torch.zeros_like(target))
    xt = x.gather(1, t[:, None])[:, 0]
    loss = torch.where(keep, lse - xt, torch.zeros_like(lse))
    count = keep.sum().clamp_min(1).double()
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    k = keep[:, None].double() * (g / count)
    xa = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))  # a masked (-inf) logit: p = 0 exactly
    return {"lse": lse, "loss": loss, "mean": loss.sum() / count, "count": count,
            "lse_scale": lse.abs() + 1, "loss_scale": keep.double() * (lse.abs() + xt.abs() + 1),
            "grad": (p - onehot) * k, "grad_scale": (p + onehot) * k.abs() * (1 + xa + lse.abs()[:, None])}


def xent_torch32(logits, target, ignore_index=-100, g=1.0):
    x = logits.detach().clone().float().requires_grad_()
    lse = torch.logsumexp(x.detach(), -1)
    keep = target != ignore_index
    t = torch.where(keep, target, torch.zeros_like(target))
    loss = torch.where(keep, lse - x.detach().gather(1, t[:, None])[:, 0], torch.zeros_like(lse))
    o = {"lse": lse, "loss": loss}
    if keep.any():
        m = F.cross_entropy(x, target, ignore_index=ignore_index)
        m.backward(torch.tensor(g, dtype=torch.float32, device=x.device))
        o["mean"], o["grad"] = m.detach(), x.grad
    return o


# ---- RoPE --------------------------------------------------------------------------------------
def rope_ref(x, cos, sin, positions=None, backward=False):
    """fp64 rotation of the (even, odd) pairs of x [B, S, H, Dh] by the fp32 tables' values; backward
    is the inverse rotation. Scale: |x0 c| + |x1 s| (resp. |x0 s| + |x1 c|), the two products summed."""
    S = x.shape[1]
    if positions is None:
        c, s = cos[:S].double()[None, :, None, :], sin[:S].double()[None, :, None, :]
    else:
        p = positions.long()
        c, s = cos.double()[p][:, :, None, :], sin.double()[p][:, :, None, :]
    if backward:
        s = -s
    x0, x1 = x[..., 0::2].double(), x[..., 1::2].double()
    y = torch.stack([x0 * c - x1 * s, x0 * s + x1 * c], -1).flatten(-2)
    sc = torch.stack([(x0 * c).abs() + (x1 * s).abs(), (x0 * s).abs() + (x1 * c).abs()], -1).flatten(-2)
    return y, sc


def rope_torch32(x, cos, sin, positions=None, backward=False):
    S = x.shape[1]
    if positions is None:
        c, s = cos[:S][None, :, None, :], sin[:S][None, :, None, :]
    else:
        c, s = cos[positions.long()][:, :, None, :], sin[positions.long()][:, :, None, :]
    if backward:
        s = -s
    x0, x1 = x[..., 0::2].float(), x[..., 1::2].float()
    return torch.stack([x0 * c - x1 * s, x0 * s + x1 * c], -1).flatten(-2)


# ---- SwiGLU / GELU -----------------------------------------------------------------------------
def swiglu_ref(a, b, g=None):
    """fp64 h = silu(a) b and, with g, da = g b s (1 + a (1 - s)), db = g a s, s = sigmoid(a).

    Scale: |value| cond with cond = 1 + |a| (1 - s), the condition number of sigmoid on an fp32
    argument (|a| where exp(-a) decides the value, 1 where the sigmoid has saturated). da's factor
    1 + a (1 - s) also carries the cancellation in 1 - s: formed to an absolute 2^-24 while
    exp(-a) >= 2^-24, to exp(-a) itself beyond: |a| min(1, 2^24 exp(-a)). Plus an underflow floor: a
    sigmoid below the smallest normal fp32 (a < -87) may be flushed to zero, which moves h by up to
    FLT_MIN |a b|, da by FLT_MIN |g b| (1 + |a|) and db by FLT_MIN |g a|; the floor is multiplied
    by 2^24 here because every scale is multiplied by c 2^-24 later."""
    a64, b64 = a.double(), b.double()
    s = torch.sigmoid(a64)
    cond = 1 + a64.abs() * (1 - s)
    canc = a64.abs() * torch.clamp(torch.exp(-a64) / EPS32, max=1.0)
    o = {"h": a64 * s * b64}
    o["h_scale"] = o["h"].abs() * cond + FLT_MIN / EPS32 * (a64 * b64).abs()
    if g is not None:
        g64 = g.double()
        o["da"] = g64 * b64 * s * (1 + a64 * (1 - s))
        o["db"] = g64 * a64 * s
        o["da_scale"] = ((g64 * b64).abs() * s * ((1 + a64.abs() * (1 - s)) * cond + canc)
                         + FLT_MIN / EPS32 * (g64 * b64).abs() * (1 + a64.abs()))
        o["db_scale"] = o["db"].abs() * cond + FLT_MIN / EPS32 * (g64 * a64).abs()
    return o


def swiglu_torch32(a, b, g=None):
    a32 = a.detach().clone().float().requires_grad_(g is not None)
    b32 = b.detach().clone().float().requires_grad_(g is not None)
    h = F.silu(a32) * b32
    o = {"h": h.detach()}
    if g is not None:
        h.backward(g.float())
        o["da"], o["db"] = a32.grad, b32.grad
    return o


def gelu_ref(x, g=None):
    """fp64 exact (erf) GELU x Phi(x) and, with g, g (Phi(x) + x phi(x)). Scale: |x| for the forward
    (Phi = 0.5 + 0.5 erf is formed to an absolute 2^-24 in fp32, whatever its size), and
    |g| (1 + |x| phi(x)) for the gradient."""
    x64 = x.double()
    cdf = 0.5 * (1 + torch.erf(x64 * 0.5 ** 0.5))
    pdf = torch.exp(-0.5 * x64 * x64) * (2 * torch.pi) ** -0.5
    o = {"y": x64 * cdf, "y_scale": x64.abs()}
    if g is not None:
        g64 = g.double()
        o["dh"] = g64 * (cdf + x64 * pdf)
        o["dh_scale"] = g64.abs() * (1 + x64.abs() * pdf)
    return o


def gelu_torch32(x, g=None):
    x32 = x.detach().clone().float().requires_grad_(g is not None)
    y = F.gelu(x32)
    o = {"y": y.detach()}
    if g is not None:
        y.backward(g.float())
        o["dh"] = x32.grad
    return o


def finite_in(ref, dtype):
    """Elements of the fp64 reference that the storage type can hold as a finite number."""
    return ref.abs() <= torch.finfo(dtype).max
