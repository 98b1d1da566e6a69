"""References, inputs and error bounds for the multi-tensor kernels (multi_tensor.hip): scale-copy /
pack / unpack, the L2 norm, fused SGD and fused Adam / AdamW with 32-bit states.

Every reference is plain PyTorch and runs wherever its inputs live; none touches the extension.
``ref_scale_copy`` reproduces the kernel's arithmetic exactly (one fp32 or fp64 multiply, one
round-to-nearest-even cast), so the copy family is compared bit for bit. The optimizer references do
**one** step in fp64 from explicit state, starting from the rounded tensors the kernel sees, and
return with every output its per-element ``scale``: the sum of the magnitudes of the terms the
update adds in fp32, each carried through the later operations (as in tests/_row_refs.py, whose
``elem_bound`` / ``check`` / ``U`` / ``SUB`` / ``EPS32`` are used, not copied).

Bounds:  |got - ref| <= u |ref| + c 2^-24 scale,  u the storage ulp of a low-precision parameter
written without a master (0 for fp32 outputs). Each ``c`` in ``C`` is 4 x the largest error, in
units of 2^-24 scale, of the ordinary fp32 torch implementation (``torch.optim.SGD`` / ``Adam`` /
``AdamW`` with ``foreach=False``, ``torch.linalg.vector_norm``) against the fp64 reference, measured
on the CPU over exactly the inputs and option tables below, which the GPU tests use too
(tests/test_mt_refs_cpu.py re-derives every figure). The factor 4 is for FMA contraction, another
summation order and ``sqrtf`` / division rounding. The kernels under test were never used to set a
figure.
"""
import math

import torch

from _row_refs import EPS32, SUB, U, check, elem_bound, ratio  # noqa: F401  (re-exported)

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64

# 4 x (max over elements, cases and options of |fp32 torch - fp64| / (2^-24 scale)); measured maximum in brackets
C = {
    "sgd_p": 4 * 2.6,     # torch.optim.SGD(foreach=False), parameter                    [2.591]
    "sgd_buf": 4 * 3.0,   # its momentum buffer                                          [2.925]
    "adam_p": 4 * 2.3,    # torch.optim.Adam / AdamW(foreach=False), parameter           [2.252]
    "adam_m": 4 * 2.7,    # exp_avg                                                      [2.692]
    "adam_v": 4 * 5.9,    # exp_avg_sq                                                   [5.806]
    # torch.linalg.vector_norm of the fp32 concatenation (fp32 / bf16 / fp16 lists). Its CPU kernel
    # accumulates lane-serially; x.square().sum().sqrt() in fp32 measures 0.64 on the same inputs.
    "l2norm": 4 * 27.3,   #                                                              [27.23]
}

# ---- sizes on the kernels' turnovers ------------------------------------------------------------
# lane vector switch (8), one iteration (2048), one chunk (8192) +- 1, two chunks +- 1, ragged multi-chunk
N = [0, 1, 7, 8, 9, 2047, 2048, 2049, 8191, 8192, 8193, 16384, 16385, 3 * 8192 + 5]
_SMALL = [1, 7, 8, 9, 2047, 2048, 2049]
_LARGE = [8193, 8191, 16385, 8192]
K_MAX_SEG = 40  # segments per launch (kMaxSeg)


def _many(n):
    s = [_SMALL[i % len(_SMALL)] for i in range(n)]
    for j, pos in enumerate((3, n // 2, n - 1)):
        s[pos] = _LARGE[j]
    return s


def sizes(kind):
    """Tensor sizes of one list. ``t41``: the second table holds one (ragged, two-block) segment.
    ``t83``: 80 non-empty tensors = two full tables, with zero-numel tensors at position 0, at the
    table boundary and as the whole remainder after the second table (so the final launch is a full
    table and nothing follows it). ``zeros``: nothing to launch at all."""
    if kind == "set":
        return list(N)
    if kind == "one":
        return [3 * 8192 + 5]
    if kind == "t40":
        return _many(40)
    if kind == "t41":
        return _many(41)
    if kind == "t83":
        a = _many(80)
        return [0] + a[:40] + [0] + a[40:] + [0]
    if kind == "zeros":
        return [0, 0, 0]
    raise KeyError(kind)


LISTS = ["set", "one", "t40", "t41", "t83", "zeros"]
assert all(sum(sizes(k)) < 300_000 for k in LISTS)


# ---- scale-copy -----------------------------------------------------------------------------------
def ref_scale_copy(src, dst_dtype, scale, scale_tensor=None):
    """dst = cast(src * scale [* scale_tensor]): fp32 arithmetic (``sc`` formed in fp32 first), or
    fp64 arithmetic if either side is fp64 (the separate fp64 kernel); the cast is torch's
    round-to-nearest-even."""
    if src.dtype == F64 or dst_dtype == F64:
        sc = torch.tensor(float(scale), dtype=F64, device=src.device)
        if scale_tensor is not None:
            sc = sc * scale_tensor.reshape(()).double()
        return (src.double() * sc).to(dst_dtype)
    sc = torch.tensor(float(scale), dtype=F32, device=src.device)
    if scale_tensor is not None:
        sc = sc * scale_tensor.reshape(()).float()
    return (src.float() * sc).to(dst_dtype)


def bf16_rne_bits(x):
    """bf16 bit patterns (int64 in [0, 65536)) of an fp32 tensor rounded to nearest even, in integer
    arithmetic on the fp32 bit pattern: an independent formulation of torch's cast. NaN -> 0x7fc0 with
    the sign kept."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return torch.where(nan, ((u >> 16) & 0x8000) | 0x7FC0, r & 0xFFFF)


def _f32_from_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(F32)


def copy_specials(dst_dtype):
    """fp32 inputs where a cast to ``dst_dtype`` can go wrong: +-0, exact ties of the 16-bit types with
    both fp32 neighbours (ties to an even and to an odd mantissa), +-the largest finite value of the
    destination, the first fp32 value that rounds up to inf, +-inf, NaN."""
    bits = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000]
    for base in (0x3F800000, 0x3F810000, 0xC0490000, 0x3EAA0000):  # bf16 ties: low half 0x8000, even / odd above
        bits += [base + 0x7FFF, base + 0x8000, base + 0x8001]
    for base in (0x3F800000, 0x3F802000, 0xC0492000):  # fp16 ties: 13 dropped bits = 0x1000
        bits += [base + 0x0FFF, base + 0x1000, base + 0x1001]
    x = _f32_from_bits(bits)
    if dst_dtype in (BF16, F16):
        big = torch.finfo(dst_dtype).max
        half_ulp = 2.0 ** (127 - 8) if dst_dtype == BF16 else 2.0 ** (15 - 11)  # half the spacing below max
        tie = torch.tensor([big + half_ulp], dtype=torch.float64).float()  # the tie with "2^emax+1": rounds to inf
        below = torch.nextafter(tie, torch.zeros(1))
        x = torch.cat([x, torch.tensor([big, -big]), tie, -tie, below, -below])
    else:
        big = torch.finfo(F32).max
        x = torch.cat([x, torch.tensor([big, -big])])
    return x


def copy_input(n, src_dtype, dst_dtype, seed):
    """A normal draw of n elements as ``src_dtype`` with the specials planted from element 1 on (as
    many as fit); an fp64 source also carries values beyond fp32's precision and range."""
    g = torch.Generator().manual_seed(seed)
    if src_dtype == F64:
        x = torch.randn(n, generator=g, dtype=F64)
        if n > 4:
            x[1], x[2], x[3] = 1e300, -1e-300, 1.0 + 2.0 ** -40
        return x
    x = torch.randn(n, generator=g)
    sp = copy_specials(dst_dtype if dst_dtype != F64 else F32)
    k = min(max(n - 1, 0), sp.numel())
    x[1:1 + k] = sp[:k]
    return x.to(src_dtype)


def subnormal_input(n, seed):
    """fp32 subnormals, and normals whose scaled value is subnormal in fp16 / bf16 / fp32."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-149, -100, (n,), generator=g).double()
    m = 1 + torch.rand(n, generator=g, dtype=F64)
    s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    x = (s * m * 2.0 ** e).float()
    h = (s * m * 2.0 ** torch.randint(-26, -13, (n,), generator=g).double()).float()  # fp16 subnormal range
    return torch.where(torch.arange(n) % 2 == 0, x, h)


# ---- L2 norm --------------------------------------------------------------------------------------
def ref_sumsq(tensors):
    """fp64 sum of squares over a list, and sum |x|^2 (every term is positive: its own scale)."""
    s = sum((t.double().square().sum() for t in tensors), torch.zeros((), dtype=F64))
    return s, s.clone()


def norm_bounds(sumsq, scale, max_norm, c):
    """(norm, its bound, clip coefficient, its bound) from the fp64 sum of squares. The norm's scale
    in fp32 roundings: the sum's relative error halves under the root (scale / (2 norm)), plus the
    root's own rounding; the coefficient min(1, max_norm / (norm + 1e-6)) adds the sum's and the
    quotient's roundings (2 more), and is 1 exactly when max_norm <= 0."""
    norm = sumsq.sqrt()
    nz = norm.clamp_min(1e-300)
    nb = c * EPS32 * (scale / (2 * nz) + norm)
    if max_norm > 0:
        coef = (max_norm / (norm + 1e-6)).clamp(max=1.0)
        cb = c * EPS32 * coef * (scale / (2 * nz * nz) + 3)
    else:
        coef, cb = torch.ones_like(norm), torch.zeros_like(norm)
    return norm, nb, coef, cb


def norm_input(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 3).to(dtype)


# ---- SGD ------------------------------------------------------------------------------------------
SGD_KEYS = ("momentum", "dampening", "nesterov", "weight_decay", "maximize", "gs", "first")
# A pairwise covering table (every legal pair of option values occurs; nesterov needs momentum and no
# dampening), generated greedily, plus the two plain momentum cases.
SGD_TABLE = [
    (0.0, 0.0, False, 0.0, False, False, True),
    (0.0, 0.1, False, 0.0, True, True, True),
    (0.0, 0.1, False, 0.01, False, False, False),
    (0.9, 0.0, True, 0.0, False, True, False),
    (0.9, 0.0, True, 0.01, True, False, True),
    (0.9, 0.1, False, 0.01, True, True, False),
    (0.9, 0.0, False, 0.0, False, False, False),
    (0.9, 0.1, False, 0.0, False, False, True),
]
SGD_LR = 0.1
GRAD_SCALE = 0.37
SGD_PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32), (F32, BF16)]  # (param, grad)
MASTER_PAIRS = [(m, g) for m in (BF16, F16) for g in (BF16, F16, F32)]       # (model param, grad)


def sgd_opts(row):
    return dict(zip(SGD_KEYS, row))


def opt_inputs(n, pdt, gdt, seed, master):
    """(param as pdt, fp32 master or None, grad as gdt) of n elements. With a master the parameter is
    its rounding."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g).to(gdt)
    if master:
        return w.to(pdt), w, gr
    return w.to(pdt), None, gr


def sgd_state(n, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randn(n, generator=g) * 0.5


def ref_sgd_step(p, g, buf, *, lr, momentum, dampening, weight_decay, nesterov, maximize, first,
                 grad_scale=None, master=None):
    """One torch.optim.SGD step in fp64 on w = master (if given) or p, with grad g * grad_scale.
    ``buf`` is read only if momentum != 0 and not ``first``. Returns p (fp64, unrounded: the new
    master too), buf, and the scales: d = g gs + wd w: |g gs| + wd |w|; buf = mom buf + (1 - damp) d:
    mom |buf| + (1 - damp) scale(d) (first: scale(d)); the step direction (nesterov: d + mom buf) its
    terms' scales added; p = w - lr dir: |w| + lr scale(dir)."""
    w = (p if master is None else master).double()
    gs = 1.0 if grad_scale is None else grad_scale.reshape(()).double()
    d = g.double() * gs * (-1.0 if maximize else 1.0)
    ds = d.abs()
    if weight_decay != 0:
        d = d + weight_decay * w
        ds = ds + weight_decay * w.abs()
    o = {}
    if momentum != 0:
        if first:
            nb, nbs = d.clone(), ds.clone()
        else:
            nb = momentum * buf.double() + (1 - dampening) * d
            nbs = momentum * buf.double().abs() + (1 - dampening) * ds
        o["buf"], o["buf_scale"] = nb, nbs
        if nesterov:
            d, ds = d + momentum * nb, ds + momentum * nbs
        else:
            d, ds = nb, nbs
    o["p"] = w - lr * d
    o["p_scale"] = w.abs() + lr * ds
    return o


def torch32_sgd_step(p, g, buf, *, lr, momentum, dampening, weight_decay, nesterov, maximize, first,
                     grad_scale=None, master=None, dtype=F32):
    """The same step by torch.optim.SGD(foreach=False) in ``dtype`` (fp32: the yardstick of C; fp64:
    the anchor of the reference). grad_scale is multiplied into the gradient first."""
    w = torch.nn.Parameter((p if master is None else master).detach().to(dtype).clone())
    gr = g.to(dtype)
    if grad_scale is not None:
        gr = gr * grad_scale.reshape(()).to(dtype)
    w.grad = gr
    opt = torch.optim.SGD([w], lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                          nesterov=nesterov, maximize=maximize, foreach=False)
    if momentum != 0 and not first:
        opt.state[w]["momentum_buffer"] = buf.detach().to(dtype).clone()
    opt.step()
    o = {"p": w.detach()}
    if momentum != 0:
        o["buf"] = opt.state[w]["momentum_buffer"]
    return o


# ---- Adam / AdamW ---------------------------------------------------------------------------------
ADAM_KEYS = ("decoupled", "weight_decay", "maximize", "gs", "step", "zero_state")
# every pair of option values occurs (a full factorial of the first four halves, steps and states cycled)
ADAM_TABLE = [
    (True, 0.0, False, False, 1, True),
    (True, 0.1, True, True, 2, False),
    (False, 0.1, False, True, 1000, True),
    (False, 0.0, True, False, 1, False),
    (True, 0.1, False, False, 1000, False),
    (False, 0.1, True, False, 2, True),
    (True, 0.0, True, True, 1000, True),
    (False, 0.0, False, True, 2, False),
    (True, 0.0, False, False, 2, True),
    (False, 0.1, True, True, 1, True),
    (True, 0.1, True, False, 1, False),
    (False, 0.0, False, False, 1000, False),
]
ADAM_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def adam_opts(row):
    return dict(zip(ADAM_KEYS, row))


def adam_inputs(n, pdt, gdt, seed, master, zero_state):
    """(param, master, grad, exp_avg, exp_avg_sq). Planted: element 0 has g = 0, m = 0, v = 0 (the
    denominator is eps alone), element 1 has |g| = 1e-4, element 2 |g| = 1e3."""
    p, m, gr = opt_inputs(n, pdt, gdt, seed, master)
    g = torch.Generator().manual_seed(seed + 2000)
    ea = torch.randn(n, generator=g) * 0.1
    es = torch.rand(n, generator=g) * 0.01
    if zero_state:
        ea, es = torch.zeros(n), torch.zeros(n)
    gr = gr.float()
    if n > 0:
        gr[0], ea[0], es[0] = 0.0, 0.0, 0.0
    if n > 2:
        gr[1], gr[2] = 1e-4, -1e3
    return p, m, gr.to(gdt), ea, es


def ref_adam_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, decoupled, maximize,
                  grad_scale=None, master=None):
    """One torch.optim.Adam (coupled L2) / AdamW (decoupled) step in fp64, no amsgrad. Scales:
    gg = g gs (+ wd w): |g gs| + wd |w|; m: b1 |m| + (1 - b1) scale(gg); v: b2 |v| + (1 - b2)
    scale(gg)^2; p = w - upd, upd = (lr / bc1) m / denom, denom = sqrt(v) / sqrt(bc2) + eps:
    |w| + (lr / bc1) scale(m) / denom + |upd| (1 + scale(v) / (2 sqrt(v) sqrt(bc2) denom)): m's and
    v's errors carried through the quotient, plus the quotient's own roundings."""
    w = (p if master is None else master).double()
    gs = 1.0 if grad_scale is None else grad_scale.reshape(()).double()
    gg = g.double() * gs * (-1.0 if maximize else 1.0)
    ggs = gg.abs()
    if weight_decay != 0:
        if decoupled:
            w = w * (1 - lr * weight_decay)
        else:
            gg = gg + weight_decay * w
            ggs = ggs + weight_decay * w.abs()
    m1 = beta1 * m.double() + (1 - beta1) * gg
    m1s = beta1 * m.double().abs() + (1 - beta1) * ggs
    v1 = beta2 * v.double() + (1 - beta2) * gg * gg
    v1s = beta2 * v.double().abs() + (1 - beta2) * ggs * ggs
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    root = v1.sqrt()
    denom = root / math.sqrt(bc2) + eps
    upd = (lr / bc1) * m1 / denom
    carried = v1s / (2 * root.clamp_min(1e-300) * math.sqrt(bc2) * denom)
    return {"p": w - upd, "m": m1, "v": v1, "m_scale": m1s, "v_scale": v1s,
            "p_scale": w.abs() + (lr / bc1) * m1s / denom + upd.abs() * (1 + carried)}


def torch32_adam_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, decoupled, maximize,
                      grad_scale=None, master=None, dtype=F32):
    w = torch.nn.Parameter((p if master is None else master).detach().to(dtype).clone())
    gr = g.to(dtype)
    if grad_scale is not None:
        gr = gr * grad_scale.reshape(()).to(dtype)
    w.grad = gr
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([w], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay, maximize=maximize,
              foreach=False)
    opt.state[w]["step"] = torch.tensor(float(step - 1))
    opt.state[w]["exp_avg"] = m.detach().to(dtype).clone()
    opt.state[w]["exp_avg_sq"] = v.detach().to(dtype).clone()
    opt.step()
    return {"p": w.detach(), "m": opt.state[w]["exp_avg"], "v": opt.state[w]["exp_avg_sq"]}


def worst(got, ref, scale):
    """max |got - ref| / (2^-24 scale) (0 where both the error and the scale are 0)."""
    err = (got.double() - ref.double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (EPS32 * scale.double()).clamp_min(1e-300))
    return r.max().item() if r.numel() else 0.0
