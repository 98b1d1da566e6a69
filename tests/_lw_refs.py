"""References, inputs and error bounds for the layer-wise trust-ratio optimizers (FusedLAMB / FusedLARS;
``fused_lamb`` / ``fused_lars`` of multi_tensor.hip). Sizes, dtype pairs, inputs, ``check`` and
``elem_bound`` are those of tests/_mt_refs.py and tests/_row_refs.py (imported, not copied).

The references do **one** step of one tensor in fp64 from explicit state and return, with every
output, its per-element ``scale`` (the magnitudes of the terms fp32 adds, carried through the later
operations, as in ``_mt_refs.ref_adam_step``), the fp64 norms, the trust ratio and the ratio's own
scale. The ratio's relative error, in units of 2^-24:

    norm of exact inputs      1.5   (the sum's relative error halves under the root, + the root's rounding)
    norm of u (LAMB)          1.5 + sum(|u| scale(u)) / |u|^2   (u's own error carried into its norm)
    LAMB  r = |w| / |u|       + 1   (the quotient)
    LARS  lam = tc |w| / (|g| |gs| + wd |w| + eps)   + 5   (|gs|, two sums, the product, the quotient)

and it enters p's scale as lr r |u| (LARS: |d|) times that term. Where the ratio is 1 by rule
(adaptation off, or a norm exactly zero) its scale is 0: the kernels must return exactly 1.

Bounds follow ``_mt_refs.C``:  |got - ref| <= u |ref| + c 2^-24 scale. Each ``c`` in ``C`` is 4 x the
largest error of the plain fp32 torch implementation below (``torch32_lamb_step`` /
``torch32_lars_step``: one torch op per operation, ``torch.linalg.vector_norm``, nothing fused) against
the fp64 reference, measured on the CPU over exactly the lists, dtype pairs and option tables the
GPU tests use (tests/test_lw_refs_cpu.py re-derives every figure). The factor 4 is for FMA
contraction, another summation order and ``sqrtf`` / division rounding, as in ``_mt_refs``. The
kernels under test were never used to set a figure.
"""
import math

import torch

import _mt_refs as M
from _mt_refs import BF16, F16, F32, F64  # noqa: F401
from _row_refs import EPS32, check, elem_bound  # noqa: F401  (re-exported)

# 4 x (max over elements, tensors, dtype pairs and options of |fp32 torch - fp64| / (2^-24 scale)); measured
# maximum in brackets
C = {
    "lamb_p": 4 * 10.6,   # parameter (the ratio's error, vector_norm's above all, carried)      [10.518]
    "lamb_m": 4 * 2.8,    # exp_avg                                                      [2.748]
    "lamb_v": 4 * 4.6,    # exp_avg_sq                                                   [4.513]
    # trust ratio |w| / |u|: torch.linalg.vector_norm's CPU kernel accumulates lane-serially
    # (_mt_refs.C["l2norm"] measures 27 on the same sizes). On a scale that already carries rel >= 4
    # this bound is about 2e-5 relative: loose enough that one dropped element among the 24581 of the
    # largest tensor would pass it. The GPU tests therefore also check exact norms on one-hot tensors
    # (test_every_element_reaches_its_norm), where a dropped element cannot hide.
    "lamb_r": 4 * 16.0,   #                                                              [15.970]
    "lars_p": 4 * 3.9,    # parameter                                                    [3.849]
    "lars_buf": 4 * 4.1,  # momentum buffer                                              [4.010]
    "lars_r": 4 * 4.8,    # trust ratio lam                                              [4.786]
}

NORM_ERR = 1.5  # relative error of sqrt(sum x^2) over exact inputs, in units of 2^-24 (see above)

# ---- lists ----------------------------------------------------------------------------------------
LISTS = ["set", "one", "t41", "t83", "zeros"]
ZERO_P, ZERO_G = 2049, 9  # the two tensors appended to "set": an all-zero parameter, an all-zero gradient


def sizes(kind):
    """``_mt_refs.sizes``; ``set`` gets two more tensors: one whose parameter (and master) is all zero,
    one whose gradient is all zero."""
    return M.sizes(kind) + ([ZERO_P, ZERO_G] if kind == "set" else [])


def zero_roles(kind):
    """(index of the all-zero parameter, index of the all-zero gradient), or (None, None)."""
    n = len(sizes(kind))
    return (n - 2, n - 1) if kind == "set" else (None, None)


# ---- LAMB -----------------------------------------------------------------------------------------
LAMB_KEYS = ("weight_decay", "always_adapt", "bias_correction", "maximize", "gs", "step", "zero_state")
# every pair of option values occurs (greedy pairwise cover); rows 1 and 7 have no adaptation (r = 1)
LAMB_TABLE = [
    (0.1, True, True, False, False, 1000, True),
    (0.0, False, False, True, True, 1000, False),
    (0.1, False, True, False, True, 2, False),
    (0.0, True, False, True, False, 1, True),
    (0.1, True, False, True, True, 2, True),
    (0.1, False, False, False, False, 1, False),
    (0.0, True, True, True, True, 1, False),
    (0.0, False, False, False, False, 2, True),
]
LAMB_HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-6)


def lamb_opts(row):
    """(keyword arguments of ref_lamb_step but grad_scale, uses grad_scale, zero_state)."""
    o = dict(zip(LAMB_KEYS, row))
    gs, zero = o.pop("gs"), o.pop("zero_state")
    o["adapt"] = o["weight_decay"] != 0 or o.pop("always_adapt")
    o.pop("always_adapt", None)
    return dict(**LAMB_HP, **o), gs, zero


def lamb_inputs(kind, pdt, gdt, master, zero_state):
    """Per tensor of the list (param, master or None, grad, exp_avg, exp_avg_sq), from
    ``_mt_refs.adam_inputs``, with the two zero tensors of ``set``."""
    zp, zg = zero_roles(kind)
    out = []
    for i, n in enumerate(sizes(kind)):
        p, mw, g, ea, es = M.adam_inputs(n, pdt, gdt, i, master, zero_state)
        if i == zp:
            p, mw = torch.zeros_like(p), (torch.zeros_like(mw) if master else None)
        if i == zg:
            g = torch.zeros_like(g)
        out.append((p, mw, g, ea, es))
    return out


def ref_lamb_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, bias_correction, adapt, maximize,
                  grad_scale=None, master=None):
    """One LAMB step of one tensor in fp64. ``adapt`` is ``weight_decay != 0 or always_adapt``. Without
    it (r = 1) this is ``_mt_refs.ref_adam_step(decoupled=True)``: w - lr (q + wd w) = w (1 - lr wd) - lr q."""
    w = (p if master is None else master).double()
    gs = 1.0 if grad_scale is None else grad_scale.reshape(()).double()
    gg = g.double() * gs * (-1.0 if maximize else 1.0)
    ggs = gg.abs()
    m1 = beta1 * m.double() + (1 - beta1) * gg
    m1s = beta1 * m.double().abs() + (1 - beta1) * ggs
    v1 = beta2 * v.double() + (1 - beta2) * gg * gg
    v1s = beta2 * v.double().abs() + (1 - beta2) * ggs * ggs
    bc1, bc2 = (1 - beta1 ** step, 1 - beta2 ** step) if bias_correction else (1.0, 1.0)
    root = v1.sqrt()
    denom = root / math.sqrt(bc2) + eps
    q = (m1 / bc1) / denom
    carried = v1s / (2 * root.clamp_min(1e-300) * math.sqrt(bc2) * denom)
    u = q + weight_decay * w
    us = m1s / bc1 / denom + q.abs() * (1 + carried) + weight_decay * w.abs()
    wn, un = w.square().sum().sqrt(), u.square().sum().sqrt()
    r, rel = torch.ones((), dtype=F64, device=w.device), torch.zeros((), dtype=F64, device=w.device)
    if adapt and wn != 0 and un != 0:
        r = wn / un
        rel = 2 * NORM_ERR + (u.abs() * us).sum() / (un * un) + 1
    return {"p": w - lr * r * u, "m": m1, "v": v1, "m_scale": m1s, "v_scale": v1s,
            "p_scale": w.abs() + lr * r * us + lr * r * u.abs() * (1 + rel),
            "w_norm": wn, "u_norm": un, "r": r, "r_scale": r * rel}


def torch32_lamb_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, bias_correction, adapt, maximize,
                      grad_scale=None, master=None, dtype=F32):
    """The same step, one torch op per operation in ``dtype`` (fp32: the yardstick of C)."""
    w = (p if master is None else master).to(dtype)
    gg = g.to(dtype)
    if grad_scale is not None:
        gg = gg * grad_scale.reshape(()).to(dtype)
    if maximize:
        gg = -gg
    m1 = m.to(dtype) * beta1 + gg * (1 - beta1)
    v1 = v.to(dtype) * beta2 + gg * gg * (1 - beta2)
    bc1, bc2 = (1 - beta1 ** step, 1 - beta2 ** step) if bias_correction else (1.0, 1.0)
    u = (m1 / bc1) / (v1.sqrt() / math.sqrt(bc2) + eps)
    if weight_decay != 0:
        u = u + w * weight_decay
    r = torch.ones((), dtype=dtype)
    if adapt:
        wn, un = torch.linalg.vector_norm(w), torch.linalg.vector_norm(u)
        r = torch.where((wn != 0) & (un != 0), wn / un, r)
    return {"p": w - lr * r * u, "m": m1, "v": v1, "r": r}


# ---- LARS -----------------------------------------------------------------------------------------
LARS_KEYS = M.SGD_KEYS
# the SGD_TABLE rows (their distinct momentum / dampening / nesterov / maximize / first parts) crossed with
# weight_decay and grad_scale
_rest = list(dict.fromkeys(r[:3] + r[4:5] + r[6:] for r in M.SGD_TABLE))  # (momentum, dampening, nesterov, maximize, first)
LARS_TABLE = [r[:3] + (wd, r[3], gs, r[4]) for r in _rest for wd in (0.0, 0.01) for gs in (False, True)]
LARS_HP = dict(lr=M.SGD_LR, trust_coefficient=0.02, eps=1e-8)
LAM_ERR = 2 * NORM_ERR + 5


def lars_opts(row):
    """(keyword arguments of ref_lars_step but grad_scale, uses grad_scale)."""
    o = dict(zip(LARS_KEYS, row))
    gs = o.pop("gs")
    return dict(**LARS_HP, **o), gs


def lars_inputs(kind, pdt, gdt, master):
    """Per tensor of the list (param, master or None, grad, momentum buffer), from ``_mt_refs.opt_inputs``
    / ``sgd_state``, with the two zero tensors of ``set``."""
    zp, zg = zero_roles(kind)
    out = []
    for i, n in enumerate(sizes(kind)):
        p, mw, g = M.opt_inputs(n, pdt, gdt, i, master)
        if i == zp:
            p, mw = torch.zeros_like(p), (torch.zeros_like(mw) if master else None)
        if i == zg:
            g = torch.zeros_like(g)
        out.append((p, mw, g, M.sgd_state(n, i)))
    return out


def ref_lars_step(p, g, buf, *, lr, momentum, dampening, weight_decay, nesterov, maximize, first, trust_coefficient,
                  eps, adapt=True, grad_scale=None, master=None):
    """One LARS step of one tensor in fp64. Without ``adapt`` (lam = 1) this is ``_mt_refs.ref_sgd_step``."""
    w = (p if master is None else master).double()
    gs = 1.0 if grad_scale is None else grad_scale.reshape(()).double()
    d = g.double() * gs * (-1.0 if maximize else 1.0)
    ds = d.abs()
    wn, gn = w.square().sum().sqrt(), g.double().square().sum().sqrt() * abs(gs)
    if weight_decay != 0:
        d = d + weight_decay * w
        ds = ds + weight_decay * w.abs()
    lam, rel = torch.ones((), dtype=F64, device=w.device), torch.zeros((), dtype=F64, device=w.device)
    if adapt and wn != 0 and gn != 0:
        lam = trust_coefficient * wn / (gn + weight_decay * wn + eps)
        rel = rel + LAM_ERR
        d, ds = lam * d, lam * ds + (lam * d).abs() * (1 + rel)
    o = {"w_norm": wn, "g_norm": gn, "r": lam, "r_scale": lam * rel}
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


def torch32_lars_step(p, g, buf, *, lr, momentum, dampening, weight_decay, nesterov, maximize, first,
                      trust_coefficient, eps, adapt=True, grad_scale=None, master=None, dtype=F32):
    """The same step, one torch op per operation in ``dtype`` (fp32: the yardstick of C)."""
    w = (p if master is None else master).to(dtype)
    gr = g.to(dtype)
    gs = torch.ones((), dtype=dtype) if grad_scale is None else grad_scale.reshape(()).to(dtype)
    lam = torch.ones((), dtype=dtype)
    if adapt:
        wn, gn = torch.linalg.vector_norm(w), torch.linalg.vector_norm(gr) * gs.abs()
        lam = torch.where((wn != 0) & (gn != 0), trust_coefficient * wn / (gn + weight_decay * wn + eps), lam)
    d = gr * (-gs if maximize else gs)
    if weight_decay != 0:
        d = d + w * weight_decay
    if adapt:
        d = d * lam
    o = {"r": lam}
    if momentum != 0:
        o["buf"] = d.clone() if first else buf.to(dtype) * momentum + d * (1 - dampening)
        d = d + o["buf"] * momentum if nesterov else o["buf"]
    o["p"] = w - lr * d
    return o


# ---- the cases of the GPU tests, which the constants are measured over ------------------------------
ALL_PAIRS = [(p, g, False) for p, g in M.SGD_PAIRS] + [(p, g, True) for p, g in M.MASTER_PAIRS]
# (list, table row) run next to every row on "set"
LAMB_EXTRA = [("one", 0), ("t41", 2), ("t83", 4)]
LARS_EXTRA = [("one", 15), ("t41", 23), ("t83", 19)]  # nesterov; momentum + dampening + maximize; first step


def cases(table, extra):
    """(list kind, row) of one dtype pair: every row on ``set``, then the extra lists."""
    return [("set", r) for r in table] + [(k, table[i]) for k, i in extra]


# ---- whole lists ----------------------------------------------------------------------------------
def ref_list(step_fn, tensors, **kw):
    """``step_fn`` over a list of per-tensor argument tuples ``(p, master or None, *rest)``: the
    per-element outputs concatenated in list order, ``r`` / ``r_scale`` stacked ([N], fp64)."""
    outs = [step_fn(p, *rest, master=mw, **kw) for p, mw, *rest in tensors]
    res = {}
    for k in (outs[0] if outs else {}):
        if outs[0][k].dim() == 0:
            res[k] = torch.stack([o[k] for o in outs])
        else:
            res[k] = torch.cat([o[k] for o in outs])
    return res


def ratio_bound(ref, c):
    return c * EPS32 * ref["r_scale"]
