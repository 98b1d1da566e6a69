#!/usr/bin/env python
"""Time FusedAdamW.step on the Llama-3-8B parameter shapes (bf16 parameters and gradients) in four
configurations: 32-bit or 8-bit (block-scaled e4m3) moments, each with fp32 master weights or with
stochastically rounded parameters and no master (param_rounding="stochastic").

    python scripts/sr_params_bench.py                          # all four, the full 8.03 B parameters
    python scripts/sr_params_bench.py --configs 8m,8s          # a subset (what fits the memory)
    python scripts/sr_params_bench.py --scale 0.125            # 4 of the 32 layers, 1/8 of the vocabulary

The optimizers step the same parameter and gradient tensors (each with its own states), one after the
other within every iteration, after a warm-up; the times are medians of device-event timings around
FusedAdamW.step. Bytes moved per parameter are counted from the shapes: gradient read 2 and parameter
written 2 in every configuration; master read + written 8, or the bf16 parameter read 2; fp32 moments
read + written 16, or two code bytes read + written 4 and two fp32 scales per 128 elements read +
written 0.125. Resident bytes are all four configurations' states at once plus 4 B per parameter of
parameters and gradients: about 257 GB at --scale 1. Prints one line per configuration and a final
JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from adam8_bench import llama3_8b_shapes  # noqa: E402
from distributeddataparallel_amd.optim import FusedAdamW  # noqa: E402

MOMENTS = {32: 16.0, 8: 4.0 + 16.0 / 128}
CONFIGS = {  # name: (state_bits, stochastic)
    "32m": (32, False), "32s": (32, True), "8m": (8, False), "8s": (8, True),
}


def bytes_per_param(bits: int, stochastic: bool) -> float:
    return 2.0 + 2.0 + (2.0 if stochastic else 8.0) + MOMENTS[bits]


def state_bytes(opt):
    return sum(t.numel() * t.element_size() for st in opt.state.values() for t in st.values() if torch.is_tensor(t))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the layers and of the vocabulary")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="32m,32s,8m,8s",
                    help="comma-separated: 32m / 8m = fp32 masters, 32s / 8s = stochastic rounding, no master")
    a = ap.parse_args(argv)
    names = a.configs.split(",")
    if not names or any(n not in CONFIGS for n in names):
        raise SystemExit(f"--configs takes a comma-separated subset of {sorted(CONFIGS)}")
    if not torch.cuda.is_available():
        raise SystemExit("sr_params_bench.py measures the HIP kernels: no GPU found")
    dev = torch.device("cuda", 0)
    params = []
    for shape in llama3_8b_shapes(a.scale):
        p = torch.nn.Parameter(torch.empty(shape, device=dev, dtype=torch.bfloat16).normal_(0, 0.02))
        p.grad = torch.empty_like(p).normal_(0, 1e-3)
        params.append(p)
    n = sum(p.numel() for p in params)
    opts = {}
    for name in names:
        bits, stochastic = CONFIGS[name]
        opts[name] = FusedAdamW(params, lr=1e-5, weight_decay=0.1, state_bits=bits, master_weights=not stochastic,
                                param_rounding="stochastic" if stochastic else "nearest")
    times = {name: [] for name in names}
    for it in range(a.warmup + a.steps):
        for name in names:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            opts[name].step()
            t1.record()
            t1.synchronize()
            if it >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    result = {"params": n, "scale": a.scale, "steps": a.steps, "configs": names}
    for name in names:
        bits, stochastic = CONFIGS[name]
        ms = statistics.median(times[name])
        moved = n * bytes_per_param(bits, stochastic)
        sb = state_bytes(opts[name])
        print(f"state_bits={bits:2d} {'stochastic, no master' if stochastic else 'fp32 master          '}: "
              f"{ms:8.3f} ms/step (min {min(times[name]):.3f}, max {max(times[name]):.3f}), "
              f"{moved / n:6.3f} B/param moved, {moved / ms / 1e9:5.2f} TB/s, optimizer state {sb / 1e9:6.2f} GB "
              f"({sb / n:.3f} B/param)")
        result[name] = {"ms": ms, "min_ms": min(times[name]), "max_ms": max(times[name]),
                        "tbps": moved / ms / 1e9, "state_bytes": sb}
    for bits in (32, 8):
        m, s = f"{bits}m", f"{bits}s"
        if m in result and s in result:
            ratio = result[s]["ms"] / result[m]["ms"]
            result[f"time_ratio_{s}_over_{m}"] = ratio
            print(f"state_bits={bits}: stochastic / master time {ratio:.3f} "
                  f"(bytes: {bytes_per_param(bits, True) / bytes_per_param(bits, False):.3f})")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
