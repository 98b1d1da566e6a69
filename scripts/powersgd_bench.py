#!/usr/bin/env python
"""The four compute stages of one PowerSGD step (project, orthonormalize, backproject, reconstruct; no
collectives) on the fused kernels (csrc/kernels/powersgd.hip) against the arithmetic of ``powerSGD_hook``
for the same work (``add_`` of the error, clone, three ``matmul`` per matrix, ``_orthogonalize`` per P,
subtraction), in one process on one GPU: device events around batches of calls, the two sides
alternating, medians over the rounds, after warm-up.

Buckets: the default 25 MiB cap filled with ResNet-50's last-stage matrices ([512, 2048], [512, 4608],
[2048, 512] in turn), and the wk, wv, wq gradients of one Llama-3-8B layer ([1024, 4096] twice,
[4096, 4096]; a tensor above the cap is a bucket of its own, here they are timed as one list). Ranks 1, 4
and 32, bucket dtypes fp32 and bf16. Bytes per fp32 gradient element, computed: the composition 44, the
fused step 32 (G and E read twice, then read and written once), both without P and Q.

    python scripts/powersgd_bench.py [--rounds 9] [--out profiles/r16_powersgd.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import q8_bench  # noqa: E402  (batch_ms, and the compiler's resource table)

BUCKET_BYTES = 25 * 2 ** 20
RESNET = [(512, 2048), (512, 4608), (2048, 512)]
LLAMA = [(1024, 4096), (1024, 4096), (4096, 4096)]


def fill(shapes, cap):
    out, total, i = [], 0, 0
    while total + shapes[i % len(shapes)][0] * shapes[i % len(shapes)][1] <= cap:
        out.append(shapes[i % len(shapes)])
        total += out[-1][0] * out[-1][1]
        i += 1
    return out


def buffers(shapes, rank, dtype):
    total = sum(n * m for n, m in shapes)
    gen = torch.Generator(device="cuda").manual_seed(0)
    flat = (torch.randn(total, device="cuda", generator=gen) * 1e-2).to(dtype)
    mats, o = [], 0
    for n, m in shapes:
        mats.append(flat[o:o + n * m].view(n, m))
        o += n * m
    rs = [min(n, m, rank) for n, m in shapes]
    return flat, mats, rs


def bench(name, shapes, rank, dtype, rounds, emit):
    from distributeddataparallel_amd.ops import powersgd as psgd
    from distributeddataparallel_amd.parallel.comm_hooks.powerSGD_hook import _orthogonalize

    flat, mats, rs = buffers(shapes, rank, dtype)
    err = torch.zeros(flat.numel(), device="cuda")
    errs = [err[g.storage_offset():g.storage_offset() + g.numel()] for g in mats]
    ps = [torch.empty(g.shape[0], r, device="cuda") for g, r in zip(mats, rs)]
    qs = [torch.randn(g.shape[1], r, device="cuda") for g, r in zip(mats, rs)]
    plan = psgd.plan(mats, errs, ps, qs)
    plan.orthonormalize_q(0.0)
    # the existing hook keeps E, P and Q in the bucket dtype
    flat2, err2 = flat.clone(), torch.zeros_like(flat)
    mats2 = [flat2[g.storage_offset():g.storage_offset() + g.numel()].view_as(g) for g in mats]
    ps2, qs2 = [p.to(dtype) for p in ps], [q.to(dtype) for q in qs]
    stages = {"project": plan.project, "orthonormalize": lambda: plan.orthonormalize_p(0.0),
              "backproject": plan.backproject, "reconstruct": lambda: plan.reconstruct(0.5)}

    def ours():
        for f in stages.values():
            f()

    def theirs():
        flat2.add_(err2)
        cp = flat2.clone()
        for g, q, p in zip(mats2, qs2, ps2):
            torch.matmul(g, q, out=p)
        for p in ps2:
            _orthogonalize(p.unsqueeze(0))
        for g, q, p in zip(mats2, qs2, ps2):
            torch.matmul(g.t(), p, out=q)
        for g, q, p in zip(mats2, qs2, ps2):
            torch.matmul(p, q.t(), out=g)
        err2.copy_(cp - flat2)

    for run in (ours, theirs):
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    calls = 10
    a, b = [], []
    for _ in range(rounds):
        a.append(q8_bench.batch_ms(ours, calls))
        b.append(q8_bench.batch_ms(theirs, calls))
    per = {k: statistics.median(q8_bench.batch_ms(f, calls) for _ in range(rounds)) for k, f in stages.items()}
    ma, mb = statistics.median(a), statistics.median(b)
    nbytes = flat.numel() * (4 * flat.element_size() + 16)  # G and E: two reads, then a read and a write
    tag = str(dtype).replace("torch.", "")
    emit(f"{name:<8} {tag:<8} r={rank:<2} {len(shapes):3d} matrices {flat.numel() / 1e6:5.1f} M el  fused "
         f"{ma * 1e3:8.1f} us [{min(a) * 1e3:.1f} .. {max(a) * 1e3:.1f}] ({nbytes / (ma * 1e-3) / 1e12:.2f} TB/s of G, E)  "
         f"torch {mb * 1e3:8.1f} us [{min(b) * 1e3:.1f} .. {max(b) * 1e3:.1f}]  ratio {mb / ma:.2f}x")
    emit("         stages (us): " + "  ".join(f"{k} {v * 1e3:.1f}" for k, v in per.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--no-resources", action="store_true", help="skip the compiler's kernel-resource table")
    ap.add_argument("--no-timing", action="store_true", help="only the kernel-resource table (needs no GPU)")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if args.no_timing:
        pass
    elif torch.cuda.is_available():
        emit(f"# one PowerSGD step without collectives, per call: median [min .. max] of {args.rounds} alternating "
             f"rounds of device-event-timed batches of 10 calls, after warm-up")
        emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; TB/s = (4 sizeof(dtype) + 16) bytes per "
             f"element over the median; the working sets fit the 256 MB Infinity Cache, so these are not HBM rates")
        for dtype in (torch.float32, torch.bfloat16):
            cap = BUCKET_BYTES // torch.empty((), dtype=dtype).element_size()
            for rank in (1, 4, 32):
                bench("resnet50", fill(RESNET, cap), rank, dtype, args.rounds, emit)
                bench("llama3", LLAMA, rank, dtype, args.rounds, emit)
        emit("# the hook's step time with its collectives on several GPUs: not measured (one GPU)")
    else:
        emit("# timings: not measured (no GPU here)")
    if not args.no_resources:
        q8_bench.KERNEL = "distributeddataparallel_amd/csrc/kernels/powersgd.hip"
        q8_bench.resources(lambda s: emit("# kernel resources (hipcc -Rpass-analysis=kernel-resource-usage); <T, RP>"
                                          if s.startswith("# kernel resources (") else s))
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
