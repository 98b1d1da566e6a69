"""References shared by the 8-bit optimizer-state tests (test_adam8_cpu.py, test_adam8_gpu.py):
an e4m3 decoder built from the bit fields, and the checks of the state format.

Format under test (FusedAdamW(state_bits=8)): per parameter uint8 codes ``exp_avg_q`` /
``exp_avg_sq_q`` (numel, memory order) and fp32 scales ``exp_avg_scale`` / ``exp_avg_sq_scale``, one per
128 elements; a code is the OCP e4m3 code of value / scale, scale = group max / 448; the second
moment is stored as s = sqrt(v).
"""
import numpy as np
import torch

GROUP = 128


def e4m3_values(device="cpu") -> torch.Tensor:
    """fp32 value of each of the 256 OCP e4m3 codes (sign 1, exponent 4 (bias 7), mantissa 3)."""
    out = []
    for code in range(256):
        sign = -1.0 if code & 0x80 else 1.0
        e, m = (code >> 3) & 0xF, code & 7
        if e == 15 and m == 7:
            out.append(float("nan"))
        elif e == 0:
            out.append(sign * m / 8 * 2.0 ** -6)
        else:
            out.append(sign * (1 + m / 8) * 2.0 ** (e - 7))
    return torch.tensor(out, dtype=torch.float32, device=device)


def expand(scale: torch.Tensor, n: int) -> torch.Tensor:
    return scale.repeat_interleave(GROUP)[:n]


def decode(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return e4m3_values(codes.device)[codes.long()] * expand(scale, codes.numel())


def group_max(x: torch.Tensor) -> torch.Tensor:
    n = x.numel()
    ng = (n + GROUP - 1) // GROUP
    return torch.nn.functional.pad(x.abs().flatten(), (0, ng * GROUP - n)).view(ng, GROUP).amax(1)


def check_shapes(st, numel):
    ng = (numel + GROUP - 1) // GROUP
    for name in ("exp_avg", "exp_avg_sq"):
        q, sc = st[name + "_q"], st[name + "_scale"]
        assert q.dtype == torch.uint8 and tuple(q.shape) == (numel,), (name, q.dtype, q.shape)
        assert sc.dtype == torch.float32 and tuple(sc.shape) == (ng,), (name, sc.dtype, sc.shape)
    assert "exp_avg" not in st and "exp_avg_sq" not in st


def check_neighbours(st, m_exact: torch.Tensor, s_exact: torch.Tensor, what=""):
    """Every decoded m and s lies within one e4m3 step of the exact value: where the exact value is
    in the normal range of its group's grid (|exact| / scale >= 2^-6) a step is at most 2^-3 |exact|,
    below it a step is scale * 2^-9. (The class is taken from the exact value, not from the code: a
    value just under 2^-6 scale may round up to the first normal code, one subnormal step away.) No
    code is the NaN code, and a non-zero s never decodes to 0."""
    for name, exact in (("exp_avg", m_exact), ("exp_avg_sq", s_exact)):
        exact = exact.flatten().double()
        q, sc = st[name + "_q"], st[name + "_scale"]
        assert ((q & 0x7F) != 0x7F).all(), f"{what}{name}: NaN code"
        dec = decode(q, sc).double()
        scale = expand(sc, q.numel()).double()
        bound = torch.where(exact.abs() >= scale * 2.0 ** -6, exact.abs() * 2.0 ** -3, scale * 2.0 ** -9)
        err = (dec - exact).abs()
        bad = err > bound
        assert not bad.any(), (f"{what}{name}: {int(bad.sum())} elements off by more than one code step, first at "
                               f"{int(bad.nonzero()[0])}: exact {exact[bad][0].item()} decoded {dec[bad][0].item()}")
    s_dec = decode(st["exp_avg_sq_q"], st["exp_avg_sq_scale"])
    assert (s_dec[s_exact.flatten() > 0] > 0).all(), f"{what}a non-zero s decoded to 0"
    assert (st["exp_avg_sq_q"] < 0x80).all(), f"{what}a negative s code"


def check_scales(st, m_exact: torch.Tensor, s_exact: torch.Tensor, what=""):
    """Each scale is (group max) / 448, exactly: the correctly rounded fp32 quotient (numpy's; torch
    may multiply by a rounded 1 / 448 on the device)."""
    for name, exact in (("exp_avg", m_exact), ("exp_avg_sq", s_exact)):
        want = torch.from_numpy(group_max(exact.float()).cpu().numpy() / np.float32(448.0))
        got = st[name + "_scale"].cpu()
        assert torch.equal(got, want), (f"{what}{name}_scale: {int((got != want).sum())} of {got.numel()} differ, "
                                        f"max |diff| {float((got - want).abs().max())}")


def dyadic(shape, gen, device="cpu"):
    """Gradients k / 64, |k| <= 64: with betas = (0.5, 0.5) every product of the moment update is
    exact, so each moment is rounded once whatever the order and fusing of the operations, and a test
    can follow the fp32 trajectory exactly with plain torch operations."""
    return (torch.randint(-64, 65, shape, generator=gen).float() / 64).to(device)


def exact_moments_b05(m_prev: torch.Tensor, v_prev: torch.Tensor, g: torch.Tensor):
    """The fp32 moments after one step with betas = (0.5, 0.5) (see dyadic)."""
    m = 0.5 * m_prev + 0.5 * g
    v = 0.5 * v_prev + (0.5 * g) * g
    return m, v


def run_whole_and_sliced(device, pieces_of):
    """Two steps on a 1000-element parameter, whole and in pieces: (whole param, state), (sliced ...)."""
    from distributeddataparallel_amd.optim import FusedAdamW

    torch.manual_seed(1)
    out = []
    init = torch.randn(1000)
    grads = [torch.randn(1000) for _ in range(2)]
    for pieces in (None, pieces_of):
        p = torch.nn.Parameter(init.clone().to(device))
        opt = FusedAdamW([p], lr=1e-2, weight_decay=0.1, state_bits=8, seed=11)
        for g in grads:
            g = g.to(device)
            if pieces is None:
                p.grad = g
                opt.step()
            else:
                opt.advance([p])
                for lo, hi in pieces:
                    # only [lo, hi) of the gradient has "arrived" with this piece, and what came before
                    have = torch.full_like(g, float("nan"))
                    have[:hi] = g[:hi]
                    opt.step_slices([(p, have, lo, hi)])
        out.append((p, opt.state[p]))
    return out


SLICINGS = [[(0, 300), (300, 1000)], [(0, 128), (128, 129), (129, 1000)]]
