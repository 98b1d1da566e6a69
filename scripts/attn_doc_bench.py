"""Document-masked causal flash attention at the Llama-3-8B shape (B1, S4096, H32/8, D128): plain
causal against ``docs`` with one document, 8 x 512, 64 x 64 and a fixed-seed ragged layout, forward
and forward+backward. Device-event timing; the cases are interleaved in one process over several
repetitions and the median per case is printed (with the ratio to plain causal).

usage: python scripts/attn_doc_bench.py [--reps 7] [--iters 200] [--plain-only] [--json]
(XDDP_BENCH_ROOT=<another checkout> imports the package from there: with --plain-only, the A/B of
plain causal attention between two builds, run alternately.)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.environ.get("XDDP_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributeddataparallel_amd.ops.attention import flash_attention  # noqa: E402

B, S, H, HKV, D = 1, 4096, 32, 8, 128


def bounds(lengths):
    """doc_start / doc_end ([1, S] int32 on the GPU) of one row holding documents of these lengths."""
    assert sum(lengths) == S and min(lengths) >= 1
    ends = torch.tensor(lengths).cumsum(0)
    ids = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))
    start = (ends - torch.tensor(lengths))[ids]

    class Docs:
        doc_start = start.to(torch.int32)[None].contiguous().cuda()
        doc_end = ends[ids].to(torch.int32)[None].contiguous().cuda()

    return Docs


def ragged(seed=0, mean=256):
    """Document lengths >= 1 drawn once from a fixed seed (exponential, mean ~256), filling S."""
    g = torch.Generator().manual_seed(seed)
    lens, left = [], S
    while left > 0:
        n = min(left, 1 + int(torch.empty(()).exponential_(1.0 / mean, generator=g)))
        lens.append(n)
        left -= n
    return lens


def visible_pairs(lengths):
    return sum(n * (n + 1) // 2 for n in lengths)


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--plain-only", action="store_true", help="plain causal only (A/B of two builds)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_doc_bench: needs a GPU")
    torch.manual_seed(0)
    q = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, S, HKV, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, S, HKV, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    g = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16)
    layouts = {"plain causal": None}
    if not a.plain_only:
        layouts.update({"docs 1 x 4096": [S], "docs 8 x 512": [512] * 8, "docs 64 x 64": [64] * 64,
                        "docs ragged": ragged()})
    cases = {}
    for name, lens in layouts.items():
        kw = {} if lens is None else {"docs": bounds(lens)}
        cases[name] = (lambda kw=kw: flash_attention(q, k, v, causal=True, **kw),
                       lambda kw=kw: flash_attention(q, k, v, causal=True, **kw).backward(g))
    times = {n: ([], []) for n in cases}
    for fns in cases.values():  # warm every case up: code objects, allocator
        for fn in fns:
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):  # interleaved: every repetition visits every case
        for n, fns in cases.items():
            for fn, acc in zip(fns, times[n]):
                acc.append(event_ms(fn, a.iters))
    med = {n: tuple(statistics.median(t) for t in ts) for n, ts in times.items()}
    if a.json:
        print(json.dumps({n: {"fwd_ms": round(f, 4), "fwd_bwd_ms": round(fb, 4)} for n, (f, fb) in med.items()}))
        return
    pf, pfb = med["plain causal"]
    full = visible_pairs([S])
    print(f"# B{B} S{S} H{H}/{HKV} D{D} bf16 causal; median of {a.reps} x {a.iters} calls, event-timed, interleaved")
    for n, (f, fb) in med.items():
        lens = layouts[n]
        share = 1.0 if lens is None else visible_pairs(lens) / full
        lo, hi = min(times[n][1]), max(times[n][1])
        print(f"{n:14s} fwd {f:7.3f} ms ({f / pf:5.2f}x plain) | fwd+bwd {fb:7.3f} ms ({fb / pfb:5.2f}x plain, "
              f"range {lo:.3f}-{hi:.3f}) | visible (q, k) pairs {share:6.3f} of causal"
              + ("" if lens is None else f" | {len(lens)} docs"))


if __name__ == "__main__":
    main()
