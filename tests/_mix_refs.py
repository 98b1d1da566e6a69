"""fp64 references and error bounds for Mixup / CutMix: the two-label cross-entropy
(cross_entropy_mixed.hip via ops/cross_entropy.py) and the image mix (mixup.hip via data/mixup.py).

With w_a = lam, w_b = 1 - lam and keep = (a != ignore_index) and (b != ignore_index):

    row loss      keep ((1 - eps)(lse - w_a x_a - w_b x_b) + eps (lse - mean_c x) + z lse^2)
    row gradient  g_r keep (p (1 + 2 z lse) - (1 - eps)(w_a onehot_a + w_b onehot_b) - eps / C)
    image         lam x_i + (1 - lam) x_j   (empty box), x_j inside the box and x_i outside (a copy)

A weight of exactly 0 leaves its term out (no 0 * inf). Bounds follow tests/_xent_refs.py:
|got - ref| <= u |ref| + c 2^-24 scale, with scale the summed magnitudes of the terms added:

    loss      keep (|lse| + (1 - eps)(w_a |x_a| + w_b |x_b|) + eps mean_c |x| + z lse^2 + 1)
    reduced   sum_r loss scale (/ count for "mean")
    gradient  (p (1 + 2 z |lse|) + (1 - eps)(w_a onehot_a + w_b onehot_b) + eps / C) |g_r| (1 + |x| + |lse|)
    image     |lam x_i| + |(1 - lam) x_j|

lse keeps _row_refs' scale |lse| + 1 and constant. Each ``c`` is 4 x the largest error, in those
units, of fp32 torch on the CPU against this reference: w_a F.cross_entropy(x, a) +
w_b F.cross_entropy(x, b) per row (with label_smoothing) plus z logsumexp^2, by autograd, over
``cases()`` x ``LAMS`` x both ignore_index values x the reductions and upstream gradients of the
GPU test; and lam * x + (1 - lam) * x[partner] over ``image_cases()``. ``python tests/_mix_refs.py``
prints the maxima. The kernels under test were never used to set a figure.
"""
import torch
import torch.nn.functional as F

from _row_refs import EPS32, U, check_elem, elem_bound  # noqa: F401
from _xent_refs import units

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

# 4 x (max over elements of |fp32 torch - fp64| / (2^-24 * scale)); the measured maximum in brackets
MC = {
    "loss": 4 * 3.3,                 # per-row loss, every (eps, z) and lam                    [3.14]
    "reduced": 4 * 3.3,              # its sum, and its mean over the kept rows                [3.14]
    "grad": 4 * 2.1,                 # autograd of the above at eps = 0                        [1.96]
    # eps > 0: torch backpropagates eps / C through a sum over the classes, twice here (as _xent_refs)
    "grad_smooth_narrow": 4 * 5.4,   # C <= 1024                                               [5.15]
    "grad_smooth_wide": 4 * 16.5,    # C in {1025, 4099}                                       [15.85]
    "mix": 4 * 2.0,                  # lam * x + (1 - lam) * x[partner] in fp32                [1.90]
}

ROWS = 33
WIDTHS = [1, 2, 10, 65, 1000, 1024, 1025, 4099]
F16_WIDTHS = [10, 1025]
TERMS = [(0.0, 0.0), (0.1, 1e-4)]
LAMS = ["0.3", "0", "1", "rows"]  # three scalars, and one weight per row
IGNORE = (-100, 3)
# rows of make_case with pinned targets, and of make_lam("rows") with pinned weights
ROW_SAME, ROW_ENDS, ROW_A_IGNORED, ROW_B_IGNORED, ROW_CLASS3 = 0, 1, 2, 3, 4
ROW_LAM0, ROW_LAM1, ROW_LAM_HALF = 6, 7, 8


def cases():
    """(C, dtype, eps, z) of the edge-shape test."""
    out = []
    for C in WIDTHS:
        for dt in (BF16, F32) + ((F16,) if C in F16_WIDTHS else ()):
            out.extend((C, dt, e, z) for e, z in TERMS)
    return out


def make_case(C, dtype, ignore_index=-100, rows=ROWS, device="cpu", seed=0):
    """N(0, 1) logits rounded to dtype and two targets per row; pinned: a == b, a on column 0 with b
    on column C - 1, a ignored, b ignored, a on class 3 (ignored when 3 is the ignore_index).
    Generated on the CPU from the seed: the CPU measurement and the GPU test see the same numbers."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=gen).to(dtype)
    a = torch.randint(0, C, (rows,), generator=gen)
    b = torch.randint(0, C, (rows,), generator=gen)
    if rows >= 9:
        b[ROW_SAME] = a[ROW_SAME]
        a[ROW_ENDS], b[ROW_ENDS] = 0, C - 1
        a[ROW_A_IGNORED] = ignore_index
        b[ROW_B_IGNORED] = ignore_index
        a[ROW_CLASS3] = min(3, C - 1)
    return x.to(device), a.to(device), b.to(device)


def make_lam(kind, rows=ROWS, device="cpu"):
    """fp32 [1] for the scalars of LAMS; "rows": U(0, 1) per row from a seeded generator with rows
    pinned to exactly 0, exactly 1 and 0.5."""
    if kind != "rows":
        return torch.tensor([float(kind)], dtype=F32, device=device)
    lam = torch.rand(rows, generator=torch.Generator().manual_seed(5))
    if rows >= 9:
        lam[ROW_LAM0], lam[ROW_LAM1], lam[ROW_LAM_HALF] = 0.0, 1.0, 0.5
    return lam.to(device)


def _weights(lam, rows):
    wa = lam.double().reshape(-1).expand(rows)
    return wa, 1 - wa


def _pick(wa, wb, va, vb):
    """w_a v_a + w_b v_b with a zero weight's term left out."""
    return torch.where(wb == 0, va, torch.where(wa == 0, vb, wa * va + wb * vb))


def mixed_ref(logits, a, b, lam, ignore_index=-100, eps=0.0, z=0.0, reduction="mean", g=1.0):
    """fp64 lse, row losses, reduced loss and gradient from the rounded logits and the fp32 lam.
    ``g`` is a number (sum, mean) or a per-row tensor (none). Rows whose loss is not finite have
    scale 0 there: compare those exactly."""
    x = logits.double()
    R, C = x.shape
    wa, wb = _weights(lam.to(x.device), R)
    lse = torch.logsumexp(x, -1)
    keep = (a != ignore_index) & (b != ignore_index)
    kd = keep.double()
    ta = torch.where(keep, a, torch.zeros_like(a))
    tb = torch.where(keep, b, torch.zeros_like(b))
    xa, xb = x.gather(1, ta[:, None])[:, 0], x.gather(1, tb[:, None])[:, 0]
    absx = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))  # a masked logit: p = 0 exactly
    loss = (1 - eps) * (lse - _pick(wa, wb, xa, xb))
    scale = lse.abs() + (1 - eps) * _pick(wa, wb, xa.abs(), xb.abs()) + 1
    if eps:
        loss = loss + eps * (lse - x.mean(-1))
        scale = scale + eps * absx.mean(-1)
    if z:
        loss = loss + z * lse ** 2
        scale = scale + z * lse ** 2
    loss = torch.where(keep, loss, torch.zeros_like(loss))
    scale = torch.where(torch.isfinite(loss), scale * kd, torch.zeros_like(scale))
    count = keep.sum().clamp_min(1).double()
    div = count if reduction == "mean" else 1.0
    g_r = (g.double().to(x.device) if torch.is_tensor(g) else torch.full_like(lse, float(g))) / div
    p = torch.exp(x - lse[:, None])
    hot = (torch.zeros_like(p).scatter_(1, ta[:, None], 1.0) * wa[:, None]
           + torch.zeros_like(p).scatter_(1, tb[:, None], 1.0) * wb[:, None])
    k = (kd * g_r)[:, None]
    la = lse.abs()[:, None]
    return {"lse": lse, "lse_scale": lse.abs() + 1, "loss": loss, "loss_scale": scale, "count": count,
            "reduced": loss if reduction == "none" else loss.sum() / div,
            "reduced_scale": scale if reduction == "none" else scale.sum() / div,
            "grad": (p * (1 + 2 * z * lse[:, None]) - (1 - eps) * hot - eps / C) * k,
            "grad_scale": (p * (1 + 2 * z * la) + (1 - eps) * hot + eps / C) * k.abs() * (1 + absx + la)}


def mixed_torch32(logits, a, b, lam, ignore_index=-100, eps=0.0, z=0.0, reduction="mean", g=1.0):
    """The ordinary fp32 torch form (the yardstick the MC figures come from): row losses, reduced
    loss and gradient."""
    x = logits.detach().clone().float().requires_grad_()
    wa = lam.float().reshape(-1)
    wb = 1 - wa
    keep = (a != ignore_index) & (b != ignore_index)
    rows = (wa * F.cross_entropy(x, a, ignore_index=ignore_index, label_smoothing=eps, reduction="none")
            + wb * F.cross_entropy(x, b, ignore_index=ignore_index, label_smoothing=eps, reduction="none"))
    rows = torch.where(keep, rows, torch.zeros_like(rows))
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


REDUCTIONS = (("mean", 1.0), ("mean", 3.0), ("sum", 3.0), ("none", None))  # (reduction, upstream g; None: per row)


def g_rows(rows=ROWS):
    return torch.randn(rows, generator=torch.Generator().manual_seed(1))


# ---- the image mix -------------------------------------------------------------------------------
IMAGE_SHAPES = [(1, 3, 5, 7), (2, 3, 5, 7), (3, 3, 5, 7), (1, 3, 32, 32), (2, 3, 32, 32), (3, 3, 32, 32),
                (3, 8, 9, 16), (2, 3, 224, 224)]
SMALL_DTYPES = (BF16, F16, F32)


def image_cases():
    """(shape, dtype): every dtype at the small shapes, bf16 at [2, 3, 224, 224]."""
    return [(s, dt) for s in IMAGE_SHAPES for dt in (SMALL_DTYPES if s[-1] < 224 else (BF16,))]


def make_images(shape, dtype, device="cpu", seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(device)


def image_lams(B, device="cpu"):
    """The general (not 0, not 1) weights of the blend test: one shared, one per sample."""
    per = 0.1 + 0.8 * torch.rand(B, generator=torch.Generator().manual_seed(7))
    return [torch.tensor([0.3], dtype=F32, device=device), per.to(device)]


def mix_ref(x, partner, lam):
    """fp64 lam x_i + (1 - lam) x_j and its scale; partner None is the flip."""
    x64 = x.double()
    xp = x64.flip(0) if partner is None else x64[partner.long()]
    w = lam.double().to(x.device).reshape(-1, 1, 1, 1)
    return w * x64 + (1 - w) * xp, (w * x64).abs() + ((1 - w) * xp).abs()


def mix_torch32(x, partner, lam):
    x32 = x.float()
    xp = x32.flip(0) if partner is None else x32[partner.long()]
    w = lam.float().to(x.device).reshape(-1, 1, 1, 1)
    return w * x32 + (1 - w) * xp


def measure(quarter_of=None):
    """Largest fp32-torch error per constant; with ``quarter_of`` (the MC table) assert each stays
    within a quarter of its bound instead of only reporting."""
    worst = {k: 0.0 for k in MC}
    for C, dt, eps, z in cases():
        for ii in IGNORE:
            x, a, b = make_case(C, dt, ii)
            for kind in LAMS:
                lam = make_lam(kind)
                for reduction, g in REDUCTIONS:
                    g = g_rows() if g is None else g
                    ref = mixed_ref(x, a, b, lam, ii, eps, z, reduction, g)
                    got = mixed_torch32(x, a, b, lam, ii, eps, z, reduction, g)
                    for key in ("loss", "reduced", "grad"):
                        name = grad_key(eps, C) if key == "grad" else key
                        worst[name] = max(worst[name], units(got[key], ref[key], ref[key + "_scale"]))
    for shape, dt in image_cases():
        x = make_images(shape, dt)
        for lam in image_lams(shape[0]):
            ref, scale = mix_ref(x, None, lam)
            worst["mix"] = max(worst["mix"], units(mix_torch32(x, None, lam), ref, scale))
    if quarter_of is not None:
        for key, w in worst.items():
            assert w <= quarter_of[key] / 4, f"{key}: fp32 torch is {w:.2f} units off, over a quarter of {quarter_of[key]}"
    return worst


if __name__ == "__main__":
    for key, w in measure().items():
        print(f"{key}: {w:.3f}")
