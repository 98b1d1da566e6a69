#!/usr/bin/env python
"""FP8 GEMM vs the bf16 library GEMM at the Llama-3-8B projection shapes (4096 tokens), all three
forms of each linear (Y, dX, dW as NT GEMMs). Event-timed: warm-up, then the median of several
batches of back-to-back launches on one stream.

usage: python scripts/gemm_fp8_bench.py [--tokens 4096] [--out FILE]
rows per GEMM: gemm_fp8_nt alone | gemm_fp8_nt + the casts it needs | torch.mm bf16 (hipBLASLt) |
torch._scaled_mm (where it runs).
"""
import argparse
import statistics
import sys

import torch

from distributeddataparallel_amd._native import load


def timed(fn, iters=20, reps=5, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / iters)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    C = load()
    T = a.tokens
    lines = [f"# gemm_fp8_nt vs bf16 torch.mm, tokens = {T}; ms per call (median of 5 x 20 launches), TFLOP/s in ()",
             f"# {'form':4} {'M':>6} {'N':>6} {'K':>6} | {'fp8 gemm':>16} | {'fp8 + casts':>16} | {'bf16 mm':>16} | {'_scaled_mm':>16}"]
    dev = "cuda"
    for N, K in [(4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336)]:
        x = torch.randn(T, K, device=dev).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16)
        dy = torch.randn(T, N, device=dev).to(torch.bfloat16)
        q = lambda t, f: C.fp8_quantize(t, C.fp8_amax(t), f, True)  # noqa: E731
        xq, xqT, sx = q(x, 0)
        wq, wqT, sw = q(w, 0)
        dq, dqT, sd = q(dy, 1)
        # (form, a, b, fmts, casts run for this GEMM in a training step, bf16 equivalent)
        forms = [
            ("Y", xq, wq, sx, sw, 0, 0, lambda: (q(x, 0), q(w, 0)), lambda: torch.mm(x, w.t())),
            ("dX", dq, wqT, sd, sw, 1, 0, lambda: q(dy, 1), lambda: torch.mm(dy, w)),
            ("dW", dqT, xqT, sd, sx, 1, 0, lambda: None, lambda: torch.mm(dy.t(), x)),
        ]
        for name, A, B, sa, sb, fa, fb, casts, bf16 in forms:
            M_, N_, K_ = A.shape[0], B.shape[0], A.shape[1]
            fl = 2.0 * M_ * N_ * K_ / 1e9
            t_g = timed(lambda: C.gemm_fp8_nt(A, B, sa, sb, fa, fb))
            t_c = timed(lambda: (casts(), C.gemm_fp8_nt(A, B, sa, sb, fa, fb)))
            t_b = timed(bf16)
            try:
                dts = (torch.float8_e4m3fn, torch.float8_e5m2)
                Af, Bf = A.view(dts[fa]), B.view(dts[fb]).t()
                one = torch.ones((), device=dev)
                t_s = timed(lambda: torch._scaled_mm(Af, Bf, scale_a=one, scale_b=one, out_dtype=torch.bfloat16))
                s_s = f"{t_s:7.3f} ({fl / t_s:6.0f})"
            except Exception as e:  # noqa: BLE001
                s_s = f"n/a ({type(e).__name__})"
            lines.append(f"  {name:4} {M_:6d} {N_:6d} {K_:6d} | {t_g:7.3f} ({fl / t_g:6.0f}) | {t_c:7.3f} ({fl / t_c:6.0f}) | "
                         f"{t_b:7.3f} ({fl / t_b:6.0f}) | {s_s:>16}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
