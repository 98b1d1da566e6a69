#!/usr/bin/env python
"""Time FusedAdamW.step with 32-bit and with 8-bit (block-scaled e4m3) optimizer states on the
Llama-3-8B parameter shapes (bf16 parameters and gradients, fp32 master weights).

    python scripts/adam8_bench.py                # the full 8.03 B-parameter list
    python scripts/adam8_bench.py --scale 0.125  # 4 of the 32 layers, 1/8 of the vocabulary

Both optimizers step the same parameter and gradient tensors (each with its own masters and
states), alternating in one process after a warm-up; the times are medians of device-event timings.
Bytes moved are counted from the shapes: per parameter 28 B with fp32 moments (master and both
moments read + written, gradient read, parameter written) and 16.125 B with 8-bit moments (master
read + written, gradient read, parameter written, two code bytes read + written, two fp32 scales
per 128 elements read + written). Prints one line per variant and a final JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributeddataparallel_amd.optim import FusedAdamW  # noqa: E402

BYTES_PER_PARAM = {32: 28.0, 8: 12.0 + 4.0 + 16.0 / 128}


def llama3_8b_shapes(scale: float):
    dim, ffn, kv, vocab, layers = 4096, 14336, 1024, 128256, 32
    layers = max(1, round(layers * scale))
    vocab = max(128, int(vocab * scale) // 128 * 128)
    shapes = [(vocab, dim)]
    for _ in range(layers):
        shapes += [(dim,), (dim, dim), (kv, dim), (kv, dim), (dim, dim), (dim,), (ffn, dim), (dim, ffn), (ffn, dim)]
    return shapes + [(dim,), (vocab, dim)]


def state_bytes(opt):
    return sum(t.numel() * t.element_size() for st in opt.state.values() for k, t in st.items()
               if torch.is_tensor(t) and k != "master")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the layers and of the vocabulary")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("adam8_bench.py measures the HIP kernels: no GPU found")
    dev = torch.device("cuda", 0)
    params = []
    for shape in llama3_8b_shapes(a.scale):
        p = torch.nn.Parameter(torch.empty(shape, device=dev, dtype=torch.bfloat16).normal_(0, 0.02))
        p.grad = torch.empty_like(p).normal_(0, 1e-3)
        params.append(p)
    n = sum(p.numel() for p in params)
    opts = {bits: FusedAdamW(params, lr=1e-5, weight_decay=0.1, master_weights=True, state_bits=bits)
            for bits in (32, 8)}
    times = {32: [], 8: []}
    for it in range(a.warmup + a.steps):
        for bits in (32, 8):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            opts[bits].step()
            t1.record()
            t1.synchronize()
            if it >= a.warmup:
                times[bits].append(t0.elapsed_time(t1))
    result = {"params": n, "scale": a.scale, "steps": a.steps}
    for bits in (32, 8):
        ms = statistics.median(times[bits])
        moved = n * BYTES_PER_PARAM[bits]
        sb = state_bytes(opts[bits])
        print(f"state_bits={bits:2d}: {ms:8.3f} ms/step (min {min(times[bits]):.3f}, max {max(times[bits]):.3f}), "
              f"{moved / 1e9:7.2f} GB moved, {moved / ms / 1e9:5.2f} TB/s, moments {sb / 1e9:6.2f} GB "
              f"({sb / n:.3f} B/param)")
        result[f"ms_{bits}"] = ms
        result[f"tbps_{bits}"] = moved / ms / 1e9
        result[f"state_bytes_{bits}"] = sb
    result["time_ratio_8_over_32"] = result["ms_8"] / result["ms_32"]
    print(f"8-bit / 32-bit time: {result['time_ratio_8_over_32']:.3f} (bytes: {BYTES_PER_PARAM[8] / 28:.3f})")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
