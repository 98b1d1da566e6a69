#!/usr/bin/env python
"""Window attention on xddp's HIP kernels (window_attn.hip) against the op's own eager fallback and
against ``F.scaled_dot_product_attention`` with the bias and the mask folded into ``attn_mask``:
forward and forward + backward, device events around batches of calls, the three sides alternating,
medians over the rounds.

Shapes: Swin-T's four stages at batch 256, N = 49, D = 32 in bf16, with a bf16 bias that needs a
gradient, without labels and with the labels of a shifted block. Per shape: the times, and the rate
over the bytes the operation has to move (forward: qkv in, o out; forward + backward: that plus
qkv and dO in, dqkv out) against 8 TB/s of HBM. Also prints the kernels' registers, LDS, scratch and
occupancy from the compiler (``--no-timing`` prints only those and needs no GPU).

    python scripts/window_attn_bench.py [--rounds 11] [--out profiles/r20_window_attn.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mixup_bench  # noqa: E402  (batch_ms and the compiler-remark table)

HBM_TBS = 8.0
SHAPES = [(16384, 3, 64), (4096, 6, 16), (1024, 12, 4), (256, 24, 1)]  # Bw, H, windows per image
N, D = 49, 32


def bench_shape(Bw, H, nW, with_labels, rounds, calls, emit):
    from distributeddataparallel_amd.models.swin import shift_labels
    from distributeddataparallel_amd.ops.window_attention import _eager, window_attention, window_attention_supported

    torch.manual_seed(0)
    qkv = torch.randn(Bw, N, 3, H, D, device="cuda").to(torch.bfloat16).requires_grad_()
    bias = torch.randn(H, N, N, device="cuda").to(torch.bfloat16).requires_grad_()
    d_out = torch.randn(Bw, N, H, D, device="cuda").to(torch.bfloat16)
    labels = None
    if with_labels:
        side = 7 * int(round(nW ** 0.5))
        labels = (shift_labels(side, side, 7, 3) if nW > 1 else torch.randint(0, 3, (1, N), dtype=torch.int32)).cuda()
    scale = D ** -0.5
    assert window_attention_supported(qkv, bias, labels)

    def sdpa():
        q, k, v = qkv.permute(2, 0, 3, 1, 4)
        m = bias
        if labels is not None:
            same = labels[:, :, None] == labels[:, None, :]
            m = (bias[None] + torch.zeros_like(same, dtype=bias.dtype).masked_fill(~same, -100.0)[:, None])
            m = m.repeat(Bw // labels.size(0), 1, 1, 1)
        return F.scaled_dot_product_attention(q, k, v, attn_mask=m, scale=scale).transpose(1, 2)

    fwd = {"xddp": lambda: window_attention(qkv, bias, labels, scale),
           "eager": lambda: _eager(qkv, bias, labels, scale), "sdpa": sdpa}
    ref = fwd["eager"]().float()
    err = {k: (f().float() - ref).abs().max().item() for k, f in fwd.items() if k != "eager"}
    tag = f"Bw {Bw:>5} H {H:>2} {'labels' if with_labels else 'plain '}"
    emit(f"# {tag}: max |o - eager o|: xddp {err['xddp']:.3e}, sdpa {err['sdpa']:.3e}")
    both = {k: (lambda f=f: torch.autograd.grad(f(), (qkv, bias), d_out)) for k, f in fwd.items()}
    io = Bw * N * H * D * 2  # bytes of one [Bw, N, H, D] bf16 tensor
    for name, sides, nbytes in (("fwd    ", fwd, 4 * io), ("fwd+bwd", both, 4 * io + 7 * io)):
        for run in sides.values():
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(rounds):
            for k, run in sides.items():
                ms[k].append(mixup_bench.batch_ms(run, calls))
        med = {k: statistics.median(v) for k, v in ms.items()}
        floor_us = nbytes / (HBM_TBS * 1e12) * 1e6
        cells = "   ".join(f"{k} {med[k] * 1e3:8.1f} us [{min(ms[k]) * 1e3:.1f} .. {max(ms[k]) * 1e3:.1f}]" for k in sides)
        emit(f"{tag} {name} {cells}   vs eager {med['eager'] / med['xddp']:.2f}x  vs sdpa {med['sdpa'] / med['xddp']:.2f}x   "
             f"{nbytes / med['xddp'] / 1e9:.2f} TB/s of compulsory bytes, floor {floor_us:.1f} us: "
             f"{100 * floor_us / (med['xddp'] * 1e3):.0f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-timing", action="store_true", help="only the kernel-resource table (needs no GPU)")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not args.no_timing:
        if not torch.cuda.is_available():
            sys.exit("window_attn_bench: needs a GPU")
        emit(f"# per call, median [min .. max] of {args.rounds} alternating rounds of {args.calls} calls between device "
             f"events; N = {N}, D = {D}, bf16, bf16 bias with gradient; eager = the op's torch fallback, sdpa = "
             f"F.scaled_dot_product_attention with bias and mask in attn_mask")
        emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
        for Bw, H, nW in SHAPES:
            for with_labels in (False, True):
                bench_shape(Bw, H, nW, with_labels, args.rounds, args.calls, emit)
    from distributeddataparallel_amd._build import EXTRA_HIP_FLAGS

    mixup_bench.resources(emit, ["distributeddataparallel_amd/csrc/kernels/window_attn.hip"],
                          EXTRA_HIP_FLAGS["window_attn.hip"].split())
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
