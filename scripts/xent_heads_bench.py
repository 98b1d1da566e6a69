#!/usr/bin/env python
"""Forward + backward time of ops.cross_entropy at the heads' shapes against the torch form each
workload uses today, F.cross_entropy(x.float(), t): device events around batches of calls, the two
sides alternating, medians over the rounds. The Llama shape with z-loss is compared against the
op's own default path (cross_entropy.hip, no z-loss). Also prints the new kernels' registers,
scratch and occupancy when the build tree is there.

    python scripts/xent_heads_bench.py [--rounds 15] [--out profiles/r12_cross_entropy_heads.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from distributeddataparallel_amd.ops.cross_entropy import check_targets, cross_entropy  # noqa: E402

KERNELS = "distributeddataparallel_amd/csrc/kernels/cross_entropy_rows.hip"


def step(fn, x, t):
    x.grad = None
    fn(x, t).backward()


def batch_ms(fn, x, t, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        step(fn, x, t)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def graph_ms(fn, x, t, calls):
    """The same step captured in a HIP graph and replayed: device time without the host's enqueue."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(fn, x, t)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn(x, t).backward()
    g.replay()
    torch.cuda.synchronize()

    def run():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            g.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls
    return run


def compare(name, rows, C, dtype, ours, theirs, their_name, rounds, calls, emit):
    torch.manual_seed(0)
    x = torch.randn(rows, C, device="cuda").to(dtype).requires_grad_()
    t = torch.randint(0, C, (rows,), device="cuda")
    for fn in (ours, theirs):  # warm up both sides at this shape
        for _ in range(3):
            step(fn, x, t)
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(batch_ms(ours, x, t, calls))
        b.append(batch_ms(theirs, x, t, calls))
    check_targets(block=True)
    ga, gb = graph_ms(ours, x, t, calls), graph_ms(theirs, x, t, calls)
    ra, rb = [], []
    for _ in range(rounds):
        ra.append(ga())
        rb.append(gb())
    ma, mb = statistics.median(ra), statistics.median(rb)
    emit(f"{name:<44} graph replay: xddp {ma * 1e3:9.1f} us [{min(ra) * 1e3:.1f} .. {max(ra) * 1e3:.1f}]   "
         f"{their_name} {mb * 1e3:9.1f} us [{min(rb) * 1e3:.1f} .. {max(rb) * 1e3:.1f}]   ratio {mb / ma:.2f}x")
    ma, mb = statistics.median(a), statistics.median(b)
    emit(f"{name:<44} eager:        xddp {ma * 1e3:9.1f} us [{min(a) * 1e3:.1f} .. {max(a) * 1e3:.1f}]   "
         f"{their_name} {mb * 1e3:9.1f} us [{min(b) * 1e3:.1f} .. {max(b) * 1e3:.1f}]   ratio {mb / ma:.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-resources", action="store_true", help="skip the compiler's kernel-resource table")
    ap.add_argument("--no-llama", action="store_true", help="skip the [4096, 128256] shape (3 GB)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("xent_heads_bench: needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# forward + backward per call, median [min .. max] of {args.rounds} alternating rounds; graph replay = the "
         f"step captured in a HIP graph (device time), eager = enqueued from Python (host-bound at the small shapes)")
    emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    f32, bf16 = torch.float32, torch.bfloat16
    compare("fp32 [32, 10]", 32, 10, f32, lambda x, t: cross_entropy(x, t),
            lambda x, t: F.cross_entropy(x.float(), t), "torch", args.rounds, 200, emit)
    compare("bf16 [256, 1000] (cross_entropy.hip, as before)", 256, 1000, bf16, lambda x, t: cross_entropy(x, t),
            lambda x, t: F.cross_entropy(x.float(), t), "torch", args.rounds, 200, emit)
    compare("bf16 [256, 1000] reduction=sum", 256, 1000, bf16, lambda x, t: cross_entropy(x, t, reduction="sum"),
            lambda x, t: F.cross_entropy(x.float(), t, reduction="sum"), "torch", args.rounds, 200, emit)
    compare("bf16 [256, 1000] label_smoothing=0.1", 256, 1000, bf16,
            lambda x, t: cross_entropy(x, t, label_smoothing=0.1),
            lambda x, t: F.cross_entropy(x.float(), t, label_smoothing=0.1), "torch", args.rounds, 200, emit)
    if not args.no_llama:
        compare("bf16 [4096, 128256] z_loss=1e-4", 4096, 128256, bf16, lambda x, t: cross_entropy(x, t, z_loss=1e-4),
                lambda x, t: cross_entropy(x, t), "default path (no z-loss)", args.rounds, 5, emit)
    if (not args.no_resources and os.path.exists("distributeddataparallel_amd/build/build.ninja")
            and os.path.exists("/opt/rocm/bin/hipcc")):
        emit("# kernel resources (hipcc -Rpass-analysis=kernel-resource-usage)")
        r = subprocess.run([sys.executable, "scripts/kernel_resources.py", KERNELS], capture_output=True, text=True)
        for s in sorted(r.stdout.splitlines(), key=lambda s: s.split("  ")[-1]):
            emit(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
