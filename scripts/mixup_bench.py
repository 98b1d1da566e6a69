#!/usr/bin/env python
"""Mixup / CutMix on the device against the torch compositions a recipe would otherwise write:
forward + backward, device events around batches of calls, the two sides alternating, medians over
the rounds, eager and as a HIP-graph replay (device time without the host's enqueue).

* image mix, bf16 [256, 3, 224, 224] channels_last: ``data.mix_images`` against
  ``x * lam + x.flip(0) * (1 - lam)`` (Mixup) and against a clone plus the box assignment
  (CutMix); the mix has no backward. Bytes: two image reads and one write for Mixup, one and one
  for CutMix (each output element has one source).
* two-label loss with label_smoothing = 0.1, bf16 [256, 1000] and fp32 [32, 10]:
  ``cross_entropy(x, MixedTarget(a, b, lam))`` against ``lam * CE(x, a) + (1 - lam) * CE(x, b)``
  with CE this package's hard-target op, and with CE ``F.cross_entropy`` on the fp32 upcast.

Also prints the new kernels' registers, LDS, scratch and occupancy from the compiler
(``--no-timing`` prints only those and needs no GPU).

    python scripts/mixup_bench.py [--rounds 15] [--out profiles/r13_mixup.txt]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

KERNELS = ["distributeddataparallel_amd/csrc/kernels/mixup.hip",
           "distributeddataparallel_amd/csrc/kernels/cross_entropy_mixed.hip"]
HBM_TBS = 8.0  # MI355X peak HBM bandwidth, TB/s


def batch_ms(run, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def graphed(run):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        run()
    g.replay()
    torch.cuda.synchronize()
    return g.replay


def compare(name, ours, theirs, their_name, rounds, calls, emit, nbytes=None):
    for run in (ours, theirs):  # warm up both sides at this shape
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    for label, fa, fb in (("graph replay", graphed(ours), graphed(theirs)), ("eager", ours, theirs)):
        a, b = [], []
        for _ in range(rounds):
            a.append(batch_ms(fa, calls))
            b.append(batch_ms(fb, calls))
        ma, mb = statistics.median(a), statistics.median(b)
        bw = f"   ({nbytes / (ma * 1e-3) / 1e12:.2f} TB/s over the bytes the rule needs)" if nbytes else ""
        emit(f"{name:<40} {label + ':':<13} xddp {ma * 1e3:9.1f} us [{min(a) * 1e3:.1f} .. {max(a) * 1e3:.1f}]   "
             f"{their_name} {mb * 1e3:9.1f} us [{min(b) * 1e3:.1f} .. {max(b) * 1e3:.1f}]   ratio {mb / ma:.2f}x{bw}")


def bench_images(rounds, emit):
    from distributeddataparallel_amd.data import mix_images

    B, H, W = 256, 224, 224
    torch.manual_seed(0)
    x = torch.randn(B, 3, H, W, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    image = x.numel() * x.element_size()
    lam = torch.tensor([0.3], device="cuda")
    empty = torch.zeros(1, 4, dtype=torch.int32, device="cuda")
    y0, y1, x0, x1 = 40, 180, 30, 170  # a box of 39 % of the image
    box = torch.tensor([[y0, y1, x0, x1]], dtype=torch.int32, device="cuda")

    def torch_mixup():  # lam is a Python number here, as in the usual recipe: baked into the launches
        return x * 0.3 + x.flip(0) * (1 - 0.3)

    def torch_cutmix():
        out = x.clone()
        out[:, :, y0:y1, x0:x1] = x.flip(0)[:, :, y0:y1, x0:x1]
        return out

    want = x.clone()
    want[:, :, y0:y1, x0:x1] = x.flip(0)[:, :, y0:y1, x0:x1]
    assert torch.equal(mix_images(x, None, lam, box), want), "CutMix differs from the torch indexing"
    err = (mix_images(x, None, lam, empty).float() - torch_mixup().float()).abs().max().item()
    emit(f"# Mixup against the torch composition: max |difference| {err:.3e} (bf16 outputs of N(0, 1) inputs)")
    emit(f"# bytes the rule needs: Mixup reads two images and writes one ({3 * image / 1e6:.0f} MB); CutMix reads each "
         f"output element's one source and writes it ({2 * image / 1e6:.0f} MB). The {image / 1e6:.0f} MB batch fits the "
         f"256 MB Infinity Cache, so the rate over those bytes is not an HBM rate (HBM peak: {HBM_TBS:.0f} TB/s)")
    compare("Mixup  bf16 [256, 3, 224, 224] NHWC", lambda: mix_images(x, None, lam, empty), torch_mixup, "torch",
            rounds, 20, emit, 3 * image)
    compare("CutMix bf16 [256, 3, 224, 224] NHWC", lambda: mix_images(x, None, lam, box), torch_cutmix, "torch",
            rounds, 20, emit, 2 * image)


def bench_loss(rows, C, dtype, rounds, emit):
    from distributeddataparallel_amd.ops import MixedTarget
    from distributeddataparallel_amd.ops.cross_entropy import check_targets, cross_entropy

    torch.manual_seed(0)
    x = torch.randn(rows, C, device="cuda").to(dtype).requires_grad_()
    a = torch.randint(0, C, (rows,), device="cuda")
    b = a.flip(0)
    lam = torch.tensor([0.3], device="cuda")
    target = MixedTarget(a, b, lam)

    def step(fn):
        def run():
            x.grad = None
            fn().backward()
        return run

    ours = step(lambda: cross_entropy(x, target, label_smoothing=0.1))
    pkg = step(lambda: lam[0] * cross_entropy(x, a, label_smoothing=0.1)
               + (1 - lam[0]) * cross_entropy(x, b, label_smoothing=0.1))
    tor = step(lambda: lam[0] * F.cross_entropy(x.float(), a, label_smoothing=0.1)
               + (1 - lam[0]) * F.cross_entropy(x.float(), b, label_smoothing=0.1))
    ours()
    g = x.grad.clone()
    tor()
    emit(f"# {dtype} [{rows}, {C}]: max |gradient difference| to the torch composition "
         f"{(g.float() - x.grad.float()).abs().max().item():.3e}")
    name = f"loss {str(dtype).replace('torch.', '')} [{rows}, {C}] smoothing 0.1"
    compare(name, ours, pkg, "2 x xddp hard-target", rounds, 200, emit)
    compare(name, ours, tor, "2 x F.cross_entropy", rounds, 200, emit)
    check_targets(block=True)


def resources(emit):
    """VGPRs, LDS, scratch and occupancy per kernel, from the compiler's remarks."""
    ninja = "distributeddataparallel_amd/build/build.ninja"
    if not (os.path.exists(ninja) and os.path.exists("/opt/rocm/bin/hipcc")):
        emit("# kernel resources: no build tree or no hipcc here")
        return
    flags = re.search(r"^hipflags = (.*)$", open(ninja).read(), re.M).group(1).split()
    emit("# kernel resources (hipcc -Rpass-analysis=kernel-resource-usage)")
    keys = {"VGPRs": "vgpr", "VGPRs Spill": "spill", "LDS Size [bytes/block]": "lds", "ScratchSize [bytes/lane]": "scratch",
            "Occupancy [waves/SIMD]": "occ"}
    for src in KERNELS:
        err = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-c", src, "-o", os.devnull,
                              "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True).stderr
        cur, rows = None, []
        for line in err.splitlines():
            m = re.search(r"remark: \s*([A-Za-z \[\]/]+): (\S+)", line)
            if not m:
                continue
            k, v = m.group(1).strip(), m.group(2)
            if k == "Function Name":
                cur = {"name": v}
                rows.append(cur)
            elif cur is not None and k in keys:
                cur[keys[k]] = v
        out = []
        for r in rows:
            n = subprocess.run(["c++filt"], input=r["name"], capture_output=True, text=True).stdout.strip()
            n = re.sub(r"xddp::kernels::\(anonymous namespace\)::", "", n)
            n = re.sub(r"^void ", "", re.sub(r"\(.*", "", n))
            out.append(f"{r.get('vgpr', '?'):>4} vgpr  spill {r.get('spill', '?'):>2}  lds {r.get('lds', '?'):>4} B  "
                       f"scratch {r.get('scratch', '?'):>2} B  occ {r.get('occ', '?'):>2}  {n}")
        for s in sorted(out, key=lambda s: s.split("  ")[-1]):
            emit(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--no-resources", action="store_true", help="skip the compiler's kernel-resource table")
    ap.add_argument("--no-timing", action="store_true", help="only the kernel-resource table (needs no GPU)")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not args.no_timing:
        if not torch.cuda.is_available():
            sys.exit("mixup_bench: needs a GPU")
        emit(f"# forward + backward per call (the image mix: forward only), median [min .. max] of {args.rounds} "
             f"alternating rounds; graph replay = the step captured in a HIP graph (device time), eager = enqueued "
             f"from Python (host-bound at the small shapes)")
        emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
        bench_images(args.rounds, emit)
        bench_loss(256, 1000, torch.bfloat16, args.rounds, emit)
        bench_loss(32, 10, torch.float32, args.rounds, emit)
    if not args.no_resources:
        resources(emit)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
