#!/usr/bin/env python
"""The three q8 kernels (csrc/kernels/q8_comm.hip) against the torch composition that
``quantization_perchannel_hook`` runs for the same work, in one process on one GPU: device events
around batches of calls, the two sides alternating, medians over the rounds, after warm-up.

The bucket is the default 25 MiB bucket cap, as bf16 and as fp32 gradients, block 512:

* ``q8_quantize``            against the hook's pad / min / max / scale / zero point / round / cast;
* ``q8_dequantize_mean`` W=8 against its ``(all_q.float() - zp) * scale`` + ``mean(0)`` + copy;
* ``q8_reduce_requant``  W=8 against the two in sequence (the hook has no such step: it is what a
  two-shot all-reduce built from its ops would run).

Byte models (G = block): quantize reads n sizeof(dtype) and writes n (1 + 8 / G); dequantize-mean
reads W n (1 + 8 / G) and writes n sizeof(dtype); reduce-requantize reads W n (1 + 8 / G) and
writes n (1 + 8 / G). The step time of the hook on several GPUs is not measured here (one GPU);
the bytes a rank moves per bucket element are computed, not timed.

    python scripts/q8_bench.py [--rounds 15] [--out profiles/r14_q8_allreduce.txt]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

KERNEL = "distributeddataparallel_amd/csrc/kernels/q8_comm.hip"
BUCKET_BYTES = 25 * 2 ** 20
G, W = 512, 8


def batch_ms(run, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def compare(name, ours, theirs, nbytes, rounds, calls, emit):
    for run in (ours, theirs):
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(batch_ms(ours, calls))
        b.append(batch_ms(theirs, calls))
    ma, mb = statistics.median(a), statistics.median(b)
    emit(f"{name:<34} xddp {ma * 1e3:8.1f} us [{min(a) * 1e3:.1f} .. {max(a) * 1e3:.1f}]  {nbytes / 1e6:6.1f} MB "
         f"-> {nbytes / (ma * 1e-3) / 1e12:.2f} TB/s   torch {mb * 1e3:8.1f} us [{min(b) * 1e3:.1f} .. "
         f"{max(b) * 1e3:.1f}]   ratio {mb / ma:.1f}x")


def torch_quantize(buf):
    """quantization_perchannel_hook up to its all-gather."""
    n = buf.numel()
    rows = (n + G - 1) // G
    x = torch.zeros(rows * G, dtype=torch.float32, device=buf.device)
    x[:n] = buf.float()
    x = x.view(rows, G)
    lo, hi = x.min(1, keepdim=True).values, x.max(1, keepdim=True).values
    scale = ((hi - lo) / 255.0).clamp_min(1e-12)
    zp = (-lo / scale).round().clamp(0, 255)
    q = (x / scale + zp).round().clamp(0, 255).to(torch.uint8)
    return q, torch.cat([scale, zp], 1).contiguous()


def torch_finish(all_q, all_p, buf):
    """quantization_perchannel_hook after its all-gather."""
    deq = (all_q.float() - all_p[..., 1:2]) * all_p[..., 0:1]
    buf.copy_(deq.mean(0).reshape(-1)[:buf.numel()].to(buf.dtype))


def bench(dtype, rounds, emit):
    from distributeddataparallel_amd.ops import q8

    n = BUCKET_BYTES // torch.empty((), dtype=dtype).element_size()
    torch.manual_seed(0)
    grads = [(torch.randn(n, device="cuda") * 1e-3).to(dtype) for _ in range(W)]
    out = torch.empty_like(grads[0])
    wire = q8.payload_bytes(n, G, 1)
    one = torch.empty(wire, dtype=torch.uint8, device="cuda")
    stacked = torch.cat([q8.quantize(g, G, 1) for g in grads])
    all_q = torch.stack([torch_quantize(g)[0] for g in grads])
    all_p = torch.stack([torch_quantize(g)[1] for g in grads])
    tag = str(dtype).replace("torch.", "")
    src = n * out.element_size()
    emit(f"# {tag}: n = {n} elements ({src / 2 ** 20:.0f} MiB), payload {wire / 2 ** 20:.2f} MiB per rank")

    def torch_reduce_requant():
        torch_finish(all_q, all_p, out)
        torch_quantize(out)

    compare(f"quantize {tag}", lambda: q8.quantize(grads[0], G, 1, out=one), lambda: torch_quantize(grads[0]),
            src + wire, rounds, 200, emit)
    compare(f"dequantize_mean W={W} -> {tag}", lambda: q8.dequantize_mean(stacked, out, G, W, "mean"),
            lambda: torch_finish(all_q, all_p, out), W * wire + src, rounds, 100, emit)
    compare(f"reduce_requant W={W} ({tag} bucket)", lambda: q8.reduce_requantize(stacked, G, W, out=one),
            torch_reduce_requant, (W + 1) * wire, rounds, 100, emit)


def wire_table(emit):
    emit("# bytes a rank sends (= receives) per bucket element, computed: ring fp32 8 (W-1)/W, ring bf16 4 (W-1)/W,")
    emit(f"# q8 allgather (W-1)(1+8/G), q8 twoshot 2 (W-1)/W (1+8/G); G = {G}")
    emit("#   W   fp32 ring   bf16 ring   q8 allgather   q8 twoshot")
    for w in (2, 4, 8, 16, 64):
        f = (w - 1) / w
        emit(f"# {w:3d}   {8 * f:9.2f}   {4 * f:9.2f}   {(w - 1) * (1 + 8 / G):12.2f}   {2 * f * (1 + 8 / G):10.2f}")


def resources(emit, KERNEL=KERNEL):
    """VGPRs, LDS, scratch and occupancy per kernel, from the compiler's remarks."""
    from distributeddataparallel_amd._build import EXTRA_HIP_FLAGS

    ninja = "distributeddataparallel_amd/build/build.ninja"
    if not (os.path.exists(ninja) and os.path.exists("/opt/rocm/bin/hipcc")):
        emit("# kernel resources: no build tree or no hipcc here")
        return
    flags = re.search(r"^hipflags = (.*)$", open(ninja).read(), re.M).group(1).split()
    flags += EXTRA_HIP_FLAGS[os.path.basename(KERNEL)].split()
    err = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-c", KERNEL, "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True).stderr
    keys = {"VGPRs": "vgpr", "LDS Size [bytes/block]": "lds", "ScratchSize [bytes/lane]": "scratch",
            "Occupancy [waves/SIMD]": "occ"}
    rows, cur = [], None
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
    emit("# kernel resources (hipcc -Rpass-analysis=kernel-resource-usage); <T, G>")
    out = []
    for r in rows:
        name = subprocess.run(["c++filt"], input=r["name"], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(.*", "", re.sub(r"xddp::(kernels|dev)::(\(anonymous namespace\)::)?", "", name))
        out.append(f"{r.get('vgpr', '?'):>4} vgpr  lds {r.get('lds', '?'):>2} B  scratch {r.get('scratch', '?'):>2} B  "
                   f"occ {r.get('occ', '?'):>2}  {re.sub(r'^void ', '', name)}")
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
            sys.exit("q8_bench: needs a GPU")
        emit(f"# per call, median [min .. max] of {args.rounds} alternating rounds of device-event-timed batches; "
             f"block {G}; TB/s = the byte model over the median")
        emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; the buffers fit the 256 MB Infinity "
             f"Cache, so the rates are not HBM rates")
        for dtype in (torch.bfloat16, torch.float32):
            bench(dtype, args.rounds, emit)
        emit("# hook step time on several GPUs: not measured (one GPU)")
        wire_table(emit)
    if not args.no_resources:
        resources(emit)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
