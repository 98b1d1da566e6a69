#!/usr/bin/env python
"""The three onebit kernels (csrc/kernels/onebit_comm.hip) against a torch composition of the same
rules, in one process on one GPU: device events around batches of calls, the two sides alternating,
medians over the rounds, after warm-up (the harness of scripts/q8_bench.py).

The bucket is the default 25 MiB bucket cap, as bf16 and as fp32 gradients, block 1024, W = 8:

* ``onebit_compress``          against add / abs / per-block mean / sign / pack bits / scale / subtract;
* ``onebit_decode_mean``       against unpack bits / select +-scale / sum over W / divide / copy;
* ``onebit_reduce_recompress`` against the two in sequence with the server residual.

For context the q8 kernels run on the same bucket (block 512), timed alone.

Byte models (G = block, s = sizeof(dtype), p = 1/8 + 4/G payload bytes per element): compress reads
n s, reads and writes the residual (8 n) and writes n p, 12.13 B per fp32 element; decode-mean
reads W n p and writes n s; reduce-recompress reads W n p, reads and writes 8 n and writes n p. The
step time of the hook on several GPUs is not measured here (one GPU); the bytes a rank moves per
bucket element are computed, not timed.

    python scripts/onebit_bench.py [--rounds 15] [--out profiles/r17_onebit_allreduce.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from q8_bench import batch_ms, compare, resources  # noqa: E402

KERNEL = "distributeddataparallel_amd/csrc/kernels/onebit_comm.hip"
BUCKET_BYTES = 25 * 2 ** 20
G, W, G8 = 1024, 8, 512


def torch_compress(x, err, weights):
    """The rules of the format as torch ops (n is a multiple of G here): payload parts returned."""
    v = (x.float() + err).view(-1, G)
    scale = v.abs().sum(1, keepdim=True) / float(G)
    neg = v < 0
    packed = (neg.view(-1, 8).to(torch.uint8) * weights).sum(1).to(torch.uint8)
    err.copy_((v - torch.where(neg, -scale, scale)).view(-1))
    return packed, scale


def torch_decode_mean(all_packed, all_scale, shifts):
    """[W, n / 8] sign bytes and [W, n / G, 1] scales -> the fp32 mean [n / G, G]."""
    neg = ((all_packed[..., None] >> shifts) & 1).bool().view(W, -1, G)
    return torch.where(neg, -all_scale, all_scale).sum(0) / float(W)


def solo(name, run, calls, rounds, emit):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t = [batch_ms(run, calls) for _ in range(rounds)]
    emit(f"{name:<34} xddp {statistics.median(t) * 1e3:8.1f} us [{min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}]")


def bench(dtype, rounds, emit):
    from distributeddataparallel_amd.ops import onebit, q8

    size = torch.empty((), dtype=dtype).element_size()
    n = BUCKET_BYTES // size
    torch.manual_seed(0)
    grads = [(torch.randn(n, device="cuda") * 1e-3).to(dtype) for _ in range(W)]
    out = torch.empty_like(grads[0])
    err, err_t, serr = (torch.zeros(n, device="cuda") for _ in range(3))
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")
    shifts = torch.arange(8, dtype=torch.uint8, device="cuda")
    wire = onebit.payload_bytes(n, G, 1)
    one = torch.empty(wire, dtype=torch.uint8, device="cuda")
    stacked = torch.cat([onebit.compress(g, torch.zeros(n, device="cuda"), G, 1) for g in grads])
    parts = [torch_compress(g, torch.zeros(n, device="cuda"), weights) for g in grads]
    all_packed, all_scale = torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])
    tag = str(dtype).replace("torch.", "")
    src = n * size
    emit(f"# {tag}: n = {n} elements ({src / 2 ** 20:.0f} MiB), payload {wire / 2 ** 20:.2f} MiB per rank")

    def torch_reduce_recompress():
        torch_compress(torch_decode_mean(all_packed, all_scale, shifts).view(-1), serr, weights)

    compare(f"compress {tag}", lambda: onebit.compress(grads[0], err, G, 1, out=one),
            lambda: torch_compress(grads[0], err_t, weights), src + 8 * n + wire, rounds, 200, emit)
    compare(f"decode_mean W={W} -> {tag}", lambda: onebit.decode_mean(stacked, out, G, W, "mean"),
            lambda: out.copy_(torch_decode_mean(all_packed, all_scale, shifts).view(-1)), W * wire + src,
            rounds, 100, emit)
    compare(f"reduce_recompress W={W} ({tag} bucket)",
            lambda: onebit.reduce_recompress(stacked, serr, G, W, out=one), torch_reduce_recompress,
            (W + 1) * wire + 8 * n, rounds, 100, emit)
    wire8 = q8.payload_bytes(n, G8, 1)
    one8 = torch.empty(wire8, dtype=torch.uint8, device="cuda")
    stacked8 = torch.cat([q8.quantize(g, G8, 1) for g in grads])
    solo(f"q8 quantize {tag} (block {G8})", lambda: q8.quantize(grads[0], G8, 1, out=one8), 200, rounds, emit)
    solo(f"q8 dequantize_mean W={W} -> {tag}", lambda: q8.dequantize_mean(stacked8, out, G8, W, "mean"), 100,
         rounds, emit)
    solo(f"q8 reduce_requant W={W}", lambda: q8.reduce_requantize(stacked8, G8, W, out=one8), 100, rounds, emit)


def wire_table(emit):
    p = 1 / 8 + 4 / G
    emit("# bytes a rank sends (= receives) per bucket element, computed: ring fp32 8 (W-1)/W, ring bf16 4 (W-1)/W,")
    emit(f"# q8 twoshot 2 (W-1)/W (1+8/{G8}), onebit allgather (W-1)(1/8+4/G), onebit twoshot 2 (W-1)/W (1/8+4/G); "
         f"G = {G}")
    emit("#   W   fp32 ring   bf16 ring   q8 twoshot   onebit allgather   onebit twoshot")
    for w in (2, 4, 8, 16):
        f = (w - 1) / w
        emit(f"# {w:3d}   {8 * f:9.2f}   {4 * f:9.2f}   {2 * f * (1 + 8 / G8):10.2f}   {(w - 1) * p:16.3f}   "
             f"{2 * f * p:14.3f}")


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
            sys.exit("onebit_bench: needs a GPU")
        emit(f"# per call, median [min .. max] of {args.rounds} alternating rounds of device-event-timed batches; "
             f"block {G}; TB/s = the byte model over the median")
        emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; the buffers fit the 256 MB Infinity "
             f"Cache, so the rates are not HBM rates")
        for dtype in (torch.bfloat16, torch.float32):
            bench(dtype, args.rounds, emit)
        emit("# hook step time on several GPUs: not measured (one GPU)")
        wire_table(emit)
    if not args.no_resources:
        resources(emit, KERNEL)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
