#!/usr/bin/env python
"""The three topk kernels (csrc/kernels/topk_comm.hip) against a torch composition of the same
rules, in one process on one GPU: device events around batches of calls, the two sides alternating,
medians over the rounds, after warm-up (the harness of scripts/q8_bench.py).

The bucket is the default 25 MiB bucket cap, as bf16 and as fp32 gradients, block 2048, k = 32,
W = 8:

* ``topk_compress``        against add / abs / topk / sort the indices / gather / scatter 0 / copy;
* ``topk_decode_mean``     against zeros / W scatter_add in rank order / divide / copy;
* ``topk_reduce_reselect`` against the two in sequence with the server residual.

The composition's ``topk`` breaks ties in an order of its own, so it is the same work, not the same
bytes. ``topk_compress`` is also timed on a bucket of one repeated value, where every block is all
ties and the bit search cannot stop early. For context the onebit kernels run on the same bucket
(block 1024), timed alone.

Byte models (G = block, s = sizeof(dtype), p = 6 k / G payload bytes per element): compress reads
n s, reads and writes the residual (8 n) and writes n p; decode-mean reads W n p and writes n s;
reduce-reselect reads W n p, reads and writes 8 n and writes n p. The step time of the hook on
several GPUs is not measured here (one GPU); the bytes a rank moves per bucket element are
computed, not timed.

    python scripts/topk_bench.py [--rounds 15] [--out profiles/r18_topk_allreduce.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from onebit_bench import solo  # noqa: E402
from q8_bench import compare, resources  # noqa: E402

KERNEL = "distributeddataparallel_amd/csrc/kernels/topk_comm.hip"
BUCKET_BYTES = 25 * 2 ** 20
G, K, W, G1 = 2048, 32, 8, 1024


def torch_compress(x, err):
    """The rules of the format as torch ops (n is a multiple of G here): payload parts returned."""
    v = (x.float() + err).view(-1, G)
    idx = v.abs().topk(K, dim=1).indices.sort(1).values
    val = v.gather(1, idx)
    err.copy_(v.scatter(1, idx, 0.0).view(-1))
    return val, idx


def torch_decode_mean(all_val, all_idx):
    """[W, n / G, K] values and offsets -> the fp32 mean [n / G, G], added up in rank order."""
    d = torch.zeros(all_val.size(1), G, device=all_val.device)
    for r in range(W):
        d.scatter_add_(1, all_idx[r], all_val[r])
    return d / float(W)


def bench(dtype, rounds, emit):
    from distributeddataparallel_amd.ops import onebit, topk

    size = torch.empty((), dtype=dtype).element_size()
    n = BUCKET_BYTES // size
    torch.manual_seed(0)
    grads = [(torch.randn(n, device="cuda") * 1e-3).to(dtype) for _ in range(W)]
    flat = torch.full((n,), 1e-3, device="cuda").to(dtype)
    out = torch.empty_like(grads[0])
    err, err_t, err_f, serr, serr_t = (torch.zeros(n, device="cuda") for _ in range(5))
    wire = topk.payload_bytes(n, G, K, 1)
    one = torch.empty(wire, dtype=torch.uint8, device="cuda")
    stacked = torch.cat([topk.compress(g, torch.zeros(n, device="cuda"), G, K, 1) for g in grads])
    parts = [torch_compress(g, torch.zeros(n, device="cuda")) for g in grads]
    all_val, all_idx = torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])
    tag = str(dtype).replace("torch.", "")
    src = n * size
    emit(f"# {tag}: n = {n} elements ({src / 2 ** 20:.0f} MiB), payload {wire / 2 ** 20:.3f} MiB per rank")

    def torch_reduce_reselect():
        torch_compress(torch_decode_mean(all_val, all_idx).view(-1), serr_t)

    compare(f"compress {tag}", lambda: topk.compress(grads[0], err, G, K, 1, out=one),
            lambda: torch_compress(grads[0], err_t), src + 8 * n + wire, rounds, 100, emit)
    solo(f"compress {tag}, one repeated value", lambda: topk.compress(flat, err_f.zero_(), G, K, 1, out=one), 100,
         rounds, emit)
    compare(f"decode_mean W={W} -> {tag}", lambda: topk.decode_mean(stacked, out, G, K, W, "mean"),
            lambda: out.copy_(torch_decode_mean(all_val, all_idx).view(-1)), W * wire + src, rounds, 100, emit)
    compare(f"reduce_reselect W={W} ({tag} bucket)",
            lambda: topk.reduce_reselect(stacked, serr, G, K, W, out=one), torch_reduce_reselect,
            (W + 1) * wire + 8 * n, rounds, 50, emit)
    wire1 = onebit.payload_bytes(n, G1, 1)
    one1 = torch.empty(wire1, dtype=torch.uint8, device="cuda")
    stacked1 = torch.cat([onebit.compress(g, torch.zeros(n, device="cuda"), G1, 1) for g in grads])
    solo(f"onebit compress {tag} (block {G1})", lambda: onebit.compress(grads[0], err, G1, 1, out=one1), 100, rounds,
         emit)
    solo(f"onebit decode_mean W={W} -> {tag}", lambda: onebit.decode_mean(stacked1, out, G1, W, "mean"), 100, rounds,
         emit)
    solo(f"onebit reduce_recompress W={W}", lambda: onebit.reduce_recompress(stacked1, serr, G1, W, out=one1), 100,
         rounds, emit)


def wire_table(emit):
    p, p1 = 6 * K / G, 1 / 8 + 4 / G1
    emit("# bytes a rank sends (= receives) per bucket element, computed: ring fp32 8 (W-1)/W, ring bf16 4 (W-1)/W,")
    emit(f"# q8 twoshot 2 (W-1)/W (1+8/512), onebit twoshot 2 (W-1)/W (1/8+4/{G1}), topk allgather (W-1) 6k/G, "
         f"topk twoshot 2 (W-1)/W 6k/G; G = {G}, k = {K}")
    emit("#   W   fp32 ring   bf16 ring   q8 twoshot   onebit twoshot   topk allgather   topk twoshot")
    for w in (2, 4, 8, 16):
        f = (w - 1) / w
        emit(f"# {w:3d}   {8 * f:9.2f}   {4 * f:9.2f}   {2 * f * (1 + 8 / 512):10.2f}   {2 * f * p1:14.3f}   "
             f"{(w - 1) * p:14.3f}   {2 * f * p:12.3f}")


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
            sys.exit("topk_bench: needs a GPU")
        emit(f"# per call, median [min .. max] of {args.rounds} alternating rounds of device-event-timed batches; "
             f"block {G}, k {K}; TB/s = the byte model over the median")
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
