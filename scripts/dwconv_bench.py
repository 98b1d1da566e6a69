#!/usr/bin/env python
"""Depthwise convolution on xddp's HIP kernels (dwconv.hip) against ``F.conv2d(groups=C)`` on
channels_last tensors (the library path a ConvNeXt block took before): forward, input gradient and
weight + bias gradient separately, device events around batches of calls, the two sides
alternating, medians over the rounds.

Shapes: the four ConvNeXt-T stages at batch 256 in bf16 with k = 7, and k = 3 at the first.
Per kernel: the time, the rate over the bytes the operation needs (forward and input gradient: one
read and one write of the map; weight gradient: two reads), the FMA rate (k k per element), and
which of the two bounds it on an MI355X (8 TB/s HBM; 78.6 TFLOP/s vector fp32 without packed
operations = 39.3 T FMA/s). The maps of stages 2 .. 4 fit the 256 MB Infinity Cache, so their byte
rates are not HBM rates. Also prints the kernels' registers, LDS, scratch and occupancy from the
compiler (``--no-timing`` prints only those and needs no GPU).

    python scripts/dwconv_bench.py [--rounds 15] [--out profiles/r19_dwconv.txt]
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

HBM_TBS, FMA_TPS = 8.0, 39.3
SHAPES = [(256, 96, 56, 56, 7), (256, 192, 28, 28, 7), (256, 384, 14, 14, 7), (256, 768, 7, 7, 7), (256, 96, 56, 56, 3)]


def bench_shape(B, C, H, W, k, rounds, calls, emit):
    from distributeddataparallel_amd._native import load

    C_ = load()
    torch.manual_seed(0)
    x = torch.randn(B, C, H, W, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = torch.randn_like(x)
    w = torch.randn(C, 1, k, k, device="cuda").to(torch.bfloat16)
    b = torch.randn(C, device="cuda").to(torch.bfloat16)
    w_taps = w.reshape(C, k * k).t().contiguous()
    conv = torch.ops.aten.convolution_backward
    args = ([C], (1, 1), (k // 2, k // 2), (1, 1), False, (0, 0), C)
    sides = {
        "forward": (lambda: C_.dwconv_forward(x, w_taps, b, False), lambda: F.conv2d(x, w, b, padding=k // 2, groups=C)),
        "dgrad": (lambda: C_.dwconv_forward(dy, w_taps, None, True), lambda: conv(dy, x, w, *args, (True, False, False))),
        "wgrad+bias": (lambda: C_.dwconv_wgrad(dy, x, k, True), lambda: conv(dy, x, w, *args, (False, True, True))),
    }
    err = (sides["forward"][0]().float() - sides["forward"][1]().float()).abs().max().item()
    emit(f"# [{B}, {C}, {H}, {W}] k = {k} bf16: max |y - library y| = {err:.3e}")
    nbytes, fmas = 2 * x.numel() * 2, x.numel() * k * k
    floor_us = max(nbytes / (HBM_TBS * 1e12), fmas / (FMA_TPS * 1e12)) * 1e6
    bound = "FMA" if fmas / FMA_TPS > nbytes / HBM_TBS else "bytes"
    for name, (ours, theirs) in sides.items():
        for run in (ours, theirs):
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        a, t = [], []
        for _ in range(rounds):
            a.append(mixup_bench.batch_ms(ours, calls))
            t.append(mixup_bench.batch_ms(theirs, calls))
        ma, mt = statistics.median(a), statistics.median(t)
        emit(f"{C:>4} x {H}x{W} k{k} {name:<11} xddp {ma * 1e3:8.1f} us [{min(a) * 1e3:.1f} .. {max(a) * 1e3:.1f}]   "
             f"library {mt * 1e3:8.1f} us [{min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}]   ratio {mt / ma:.2f}x   "
             f"{nbytes / ma / 1e9:.2f} TB/s  {fmas / ma / 1e9:.2f} T FMA/s  floor {floor_us:.1f} us ({bound}): "
             f"{100 * floor_us / (ma * 1e3):.0f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-timing", action="store_true", help="only the kernel-resource table (needs no GPU)")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not args.no_timing:
        if not torch.cuda.is_available():
            sys.exit("dwconv_bench: needs a GPU")
        emit(f"# per call, median [min .. max] of {args.rounds} alternating rounds of {args.calls} calls between device "
             f"events; library = F.conv2d(groups=C) / aten.convolution_backward on channels_last bf16")
        emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
        for shape in SHAPES:
            bench_shape(*shape, args.rounds, args.calls, emit)
    from distributeddataparallel_amd._build import EXTRA_HIP_FLAGS

    mixup_bench.resources(emit, ["distributeddataparallel_amd/csrc/kernels/dwconv.hip"],
                          EXTRA_HIP_FLAGS["dwconv.hip"].split())
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
