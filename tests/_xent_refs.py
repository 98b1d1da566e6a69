"""fp64 reference and error bounds for the cross-entropy of every head (cross_entropy_rows.hip via
ops/cross_entropy.py): label smoothing eps, z-loss z, reductions none / sum / mean.

    row loss      keep ((1 - eps)(lse - x_t) + eps (lse - mean_c x) + z lse^2)
    row gradient  g_r keep (p (1 + 2 z lse) - (1 - eps) onehot_t - eps / C)

Bounds follow tests/_row_refs.py: |got - ref| <= u |ref| + c 2^-24 scale, with scale the summed
magnitudes of the terms added:

    loss      keep (|lse| + (1 - eps) |x_t| + eps mean_c |x| + z lse^2 + 1)
    reduced   sum_r loss scale (/ count for "mean")
    gradient  (p (1 + 2 z |lse|) + (1 - eps) onehot + eps / C) |g_r| (1 + |x| + |lse|)

(g_r = g / count for "mean"). lse keeps _row_refs' scale |lse| + 1 and constant. Each new ``c`` is
4 x the largest error, in those units, of fp32 torch on the CPU (F.cross_entropy with
label_smoothing, plus z * logsumexp^2 by autograd) against this reference over ``cases()``: the
shapes, dtypes, (eps, z) pairs and distributions the GPU test uses. ``python tests/_xent_refs.py``
prints the maxima. The kernels under test were never used to set a figure.
"""
import torch
import torch.nn.functional as F

from _row_refs import C as RC, EPS32, U, check_elem, elem_bound  # noqa: F401

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

# 4 x (max over elements of |fp32 torch - fp64| / (2^-24 * scale)); the measured maximum in brackets
XC = {
    "loss": 4 * 2.9,          # per-row loss, every (eps, z)                                  [2.78]
    "reduced": 4 * 2.9,       # its sum, and its mean over the kept rows                      [2.81]
    "grad": 4 * 2.9,          # autograd of the above at eps = 0; g in {1, 3} and per row     [2.82]
    # eps > 0: torch backpropagates eps / C through a sum over the C classes, so its error grows
    # with the width ([5.8] at C = 1025, [16.1] at 4099, the maximum at 50257): one constant for the
    # narrow kernels' widths (C <= 1024), one for the wide kernels'
    "grad_smooth_narrow": 4 * 5.2,   #                                                        [5.06]
    "grad_smooth_wide": 4 * 115.0,   #                                                        [111.93]
}

WIDTHS = [1, 2, 10, 63, 64, 65, 1000, 1023, 1024, 1025, 2056, 4099, 50257]
TERM_WIDTHS = [10, 65, 1000, 1024, 1025, 4099, 50257]  # where (eps, z) != (0, 0) runs too
F16_WIDTHS = [10, 1000, 1025, 4099]
TERMS = [(0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4)]


def cases():
    """(C, dtype, eps, z) of the edge-shape test."""
    out = []
    for C in WIDTHS:
        for dt in (BF16, F32) + ((F16,) if C in F16_WIDTHS else ()):
            out.append((C, dt, 0.0, 0.0))
            if C in TERM_WIDTHS:
                out.extend((C, dt, e, z) for e, z in TERMS)
    return out


def rows_for(C):
    return 8 if C == 50257 else 33


def make_case(C, dtype, ignore_index=-100, rows=None, device="cpu", seed=0):
    """N(0, 1) logits rounded to dtype; targets pinned to column 0, column C - 1, class 3 (valid,
    ignored only when 3 is the ignore_index) and ignore_index. Generated on the CPU from the seed, so
    the CPU measurement and the GPU test see the same numbers."""
    rows = rows_for(C) if rows is None else rows
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=gen).to(dtype)
    t = torch.randint(0, C, (rows,), generator=gen)
    if rows >= 6:
        t[0], t[1] = 0, C - 1
        t[4] = min(3, C - 1)
        t[5] = ignore_index
    return x.to(device), t.to(device)


def xent_heads_ref(logits, target, ignore_index=-100, eps=0.0, z=0.0, reduction="mean", g=1.0):
    """fp64 lse, row losses, reduced loss and gradient from the rounded logits. ``g`` is a number
    (sum, mean) or a per-row tensor (none). Rows whose loss is not finite (a -inf logit at eps > 0)
    have scale 0 there: compare those exactly."""
    x = logits.double()
    R, C = x.shape
    lse = torch.logsumexp(x, -1)
    keep = target != ignore_index
    kd = keep.double()
    t = torch.where(keep, target, torch.zeros_like(target))
    xt = x.gather(1, t[:, None])[:, 0]
    xa = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))  # a masked logit: p = 0 exactly
    loss = (1 - eps) * (lse - xt)
    scale = lse.abs() + (1 - eps) * xt.abs() + 1
    if eps:
        loss = loss + eps * (lse - x.mean(-1))
        scale = scale + eps * xa.mean(-1)
    if z:
        loss = loss + z * lse ** 2
        scale = scale + z * lse ** 2
    loss = torch.where(keep, loss, torch.zeros_like(loss))
    scale = torch.where(torch.isfinite(loss), scale * kd, torch.zeros_like(scale))
    count = keep.sum().clamp_min(1).double()
    div = count if reduction == "mean" else 1.0
    g_r = (g.double() if torch.is_tensor(g) else torch.full_like(lse, float(g))) / div
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    k = (kd * g_r)[:, None]
    la = lse.abs()[:, None]
    return {"lse": lse, "lse_scale": lse.abs() + 1, "loss": loss, "loss_scale": scale, "count": count,
            "reduced": loss if reduction == "none" else loss.sum() / div,
            "reduced_scale": scale if reduction == "none" else scale.sum() / div,
            "grad": (p * (1 + 2 * z * lse[:, None]) - (1 - eps) * onehot - eps / C) * k,
            "grad_scale": (p * (1 + 2 * z * la) + (1 - eps) * onehot + eps / C) * k.abs() * (1 + xa + la)}


def xent_heads_torch32(logits, target, ignore_index=-100, eps=0.0, z=0.0, reduction="mean", g=1.0):
    """The ordinary fp32 torch form of the same (the yardstick the XC figures come from): row losses,
    reduced loss and gradient."""
    x = logits.detach().clone().float().requires_grad_()
    keep = target != ignore_index
    rows = F.cross_entropy(x, target, ignore_index=ignore_index, label_smoothing=eps, reduction="none")
    if z:
        rows = rows + z * torch.logsumexp(x, -1) ** 2 * keep
    if reduction == "none":
        red = rows
    else:
        red = rows.sum() if reduction == "sum" else rows.sum() / keep.sum().clamp_min(1)
    red.backward(g.float() if torch.is_tensor(g) else torch.tensor(float(g)))
    return {"loss": rows.detach(), "reduced": red.detach(), "grad": x.grad}


def grad_key(eps, C):
    return "grad" if not eps else "grad_smooth_narrow" if C <= 1024 else "grad_smooth_wide"


def units(got, ref, scale):
    """max |got - ref| / (2^-24 scale) over the elements with a finite reference and a scale."""
    ok = torch.isfinite(ref) & (scale > 0)
    if not ok.any():
        return 0.0
    return ((got.double() - ref)[ok].abs() / (EPS32 * scale[ok])).max().item()


def measure(quarter_of=None):
    """Largest fp32-torch error per constant over cases() x reductions x g; with ``quarter_of`` (the
    XC table) assert each stays within a quarter of its bound instead of only reporting."""
    worst = {"loss": 0.0, "reduced": 0.0, "grad": 0.0, "grad_smooth_narrow": 0.0, "grad_smooth_wide": 0.0}
    for C, dt, eps, z in cases():
        for ii in (-100, 3):
            x, t = make_case(C, dt, ii)
            for reduction, g in (("mean", 1.0), ("mean", 3.0), ("sum", 3.0), ("none", None)):
                if g is None:
                    g = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(1))
                ref = xent_heads_ref(x, t, ii, eps, z, reduction, g)
                got = xent_heads_torch32(x, t, ii, eps, z, reduction, g)
                for key in ("loss", "reduced", "grad"):
                    name = grad_key(eps, C) if key == "grad" else key
                    worst[name] = max(worst[name], units(got[key], ref[key], ref[key + "_scale"]))
    if quarter_of is not None:
        for key, w in worst.items():
            assert w <= quarter_of[key] / 4, f"{key}: fp32 torch is {w:.2f} units off, over a quarter of {quarter_of[key]}"
    return worst


if __name__ == "__main__":
    for key, w in measure().items():
        print(f"{key}: {w:.3f}")
