"""Inputs, the fp64 reference and the error bound of the Adafactor tests (tests/test_adafactor_gpu.py,
tests/test_adafactor_cpu.py).

Bound per output: ``K[output] * eps(output dtype) * max(|ref|, RMS(ref))``. ``K`` is 4 x the largest
error, in the same units, of ``torch.optim.Adafactor`` in fp32 on the CPU (``foreach`` on and off:
the same figures) against ``ref_step`` over the fp32 form of exactly the inputs of the GPU tests
(every shape list and degenerate input x every row of ``OPTS``); the factor 4 is for another
summation order, FMA contraction and the parameter's own rounding. The kernels under test were
never used to set it.
"""
import torch

# measured maxima, each with the input it occurs on (all inputs in fp32, no master):
#   w        4.110  make((65, 257), 0, ..., OPTS[3], zero="param")   (test_degenerate_inputs_stay_finite)
#   row_var  3.848  make((2, 2049, 9), 7, ..., OPTS[2])               (MIXED + VECS, index 7)
#   col_var  8.734  two_tables(OPTS[1])[32], 156 x 248
#   variance 2.051  the (8192,) vector of MIXED + VECS under OPTS[2]
K = {"w": 4 * 4.2, "row_var": 4 * 3.9, "col_var": 4 * 8.8, "variance": 4 * 2.1}
TR, TC = 64, 256  # the tile of af_stats_kernel / af_usq_kernel / af_apply_kernel
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
HP = dict(lr=1e-2, beta2_decay=-0.8, eps2=1e-3)
# (step, weight_decay, maximize, grad_scale, eps1 (None: finfo(w).eps), d, state scale); row 0 clips
# (RMS(u) / d > 1), rows 1 and 2 do not (test_clip_regimes asserts both)
OPTS = [(7, 0.0, False, None, None, 1.0, 0.01), (1, 0.1, True, 0.5, 2.0 ** -16, 8.0, 0.0),
        (7, 0.1, False, 3.0, None, 8.0, 1.0), (1, 0.0, True, None, 2.0 ** -16, 1.0, 0.0)]
CLIPS = {0: True, 1: False, 2: False}
PAIRS = [(p, g, False) for p in (F32, BF16, F16) for g in (F32, BF16)] + [(p, g, True) for p in (BF16, F16)
                                                                         for g in (F32, BF16)]
ROWS = [1, TR - 1, TR, TR + 1, 2 * TR + 3]
COLS = [1, 7, 8, 9, TC - 8, TC + 1, 2 * TC + 8]
VECS = [(1,), (7,), (8,), (2047,), (8192,), (8193,)]  # the flat kernel's vector, iteration and chunk edges
FOLD_ROWS = 2048  # rows per row block of af_fold_kernel
MIXED = [(TR + 1, TC + 1), (3, TR, 8), (1, 9), (2, 1, 5, 2 * TC + 8), (2047,), (8193,), (), (2, FOLD_ROWS + 1, 9)]


def shapes_of_row(r):
    """Every column edge at B = 1 and at B = 3 (3-D and 4-D in turn)."""
    return [s for j, c in enumerate(COLS) for s in ((r, c), (3, 1, r, c) if j % 2 else (3, r, c))]


def make(shape, i, pdt, gdt, master, opt, zero=None):
    """(param, master or None, grad, {state}) of one tensor on the CPU."""
    gen = torch.Generator().manual_seed(4321 + i)
    rnd = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    w, g = 0.05 * rnd(*shape), rnd(*shape)
    if len(shape) >= 2:  # rows and columns of different magnitude, so the two factors matter
        g = g * (0.5 + rnd(*shape[:-1], 1).abs()) * (0.5 + rnd(*shape[:-2], 1, shape[-1]).abs())
        if zero == "row":
            g[..., shape[-2] // 2, :] = 0
        if zero == "col":
            g[..., :, shape[-1] // 2] = 0
    if zero == "grad":
        g = torch.zeros(shape)
    if zero == "param":
        w = torch.zeros(shape)
    mk = lambda *s: opt[6] * (0.1 + rnd(*s).abs()) if opt[0] > 1 else torch.zeros(s)  # noqa: E731
    if len(shape) >= 2:
        st = {"row_var": mk(*shape[:-1], 1), "col_var": mk(*shape[:-2], 1, shape[-1])}
    else:
        st = {"variance": mk(*shape)}
    return w.to(pdt), (w if master else None), g.to(gdt), st


def two_tables(opt):
    """A zero-numel matrix, 42 matrices, 41 vectors, a zero-numel vector and a zero-numel matrix: more than
    the 40 tensors of one segment table of either kind, a third of the matrices with C % 8 == 0 (the
    16-byte path). The last matrix and the last vector land in second tables."""
    mats = [(1 + 5 * i, (1 + (37 * i) % 300 + 7) // 8 * 8 if i % 3 == 0 else 1 + (37 * i) % 300) for i in range(42)]
    shapes = [(0, 5)] + mats + [(1 + 211 * i,) for i in range(41)] + [(0,), (3, 0)]
    return [make(s, i, BF16, BF16, True, opt) for i, s in enumerate(shapes)]


def kwargs(opt, wdt):
    step, wd, maximize, gs, eps1, d, _ = opt
    return dict(HP, step=step, weight_decay=wd, maximize=maximize, d=d, gs=gs,
                eps1=torch.finfo(wdt).eps if eps1 is None else eps1)


def ref_step(w, g, st, *, lr, beta2_decay, eps1, eps2, d, weight_decay, step, maximize, gs):
    """One Adafactor step of one tensor in fp64."""
    w, g = w.double(), g.double() * (1.0 if gs is None else gs) * (-1.0 if maximize else 1.0)
    omb, rho = float(step) ** beta2_decay, min(lr, step ** -0.5)
    alpha = max(eps2, w.square().mean().sqrt().item()) * rho
    w, out = w * (1 - lr * weight_decay), {}
    if g.dim() >= 2:
        rv = torch.lerp(st["row_var"].double(), g.square().mean(-1, keepdim=True), omb)
        cv = torch.lerp(st["col_var"].double(), g.square().mean(-2, keepdim=True), omb)
        var = rv * cv / rv.mean(-2, keepdim=True).clamp_min(eps1)
        out.update(row_var=rv, col_var=cv)
    else:
        var = out["variance"] = torch.lerp(st["variance"].double(), g * g, omb)
    u = g * var.clamp_min(eps1 * eps1).rsqrt()
    out["clip"] = u.square().mean().sqrt().item() / d
    out["w"] = w - alpha / max(1.0, out["clip"]) * u
    return out


def close(got, ref, k, what):
    ref = ref.to(got.device)
    bound = K[k] * torch.finfo(got.dtype).eps * torch.maximum(ref.abs(), ref.square().mean().sqrt())
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), f"{what}: max err / bound = {(err / bound).max().item():.3f}"
