#!/usr/bin/env python
"""Time FusedAdafactor.step against torch.optim.Adafactor (foreach on and off) and FusedAdamW on the
ViT-L/16 and Llama-3-8B parameter shapes, and record what the compiler made of every kernel.

    python scripts/adafactor_bench.py                       # ViT-L/16, Llama-3-8B at --scale 0.25, two single tensors
    python scripts/adafactor_bench.py --resources-only      # no GPU: compile adafactor.hip, list the kernels

Per list, every variant steps the same bf16 parameter and gradient tensors (each with its own
states), alternating in one process after a warm-up; times are medians of device-event timings.
``fused_adafactor`` and ``fused_adamw`` keep fp32 masters; ``fused_adafactor_nomaster`` and torch's
Adafactor (which has none) update the bf16 parameters directly. The byte model per parameter of a
matrix (bf16 parameter and gradient, fp32 master): the statistics pass reads g and w (6 B), the
sum(u^2) pass reads g (2 B), the apply pass reads g and w and writes w and the parameter (12 B):
20 B, against AdamW's 28 B; without masters 4 + 2 + 6 = 12 B. The partial slabs add 4 B per 64 rows
and per 256 columns. Reading g three times is inherent: the column factor and the RMS of u each
need all of g first. No speed ratio is a pass condition; the report says what was measured.

Writes the report to --out (default profiles/r15_adafactor.txt) and prints a final JSON line.
"""
import argparse
import json
import os
import re
import shlex
import shutil
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributeddataparallel_amd import _build  # noqa: E402
from distributeddataparallel_amd.optim import FusedAdafactor, FusedAdamW  # noqa: E402
from layerwise_optim_bench import llama3_8b_shapes, make_params, model_shapes, time_variants  # noqa: E402

# single tensors the tiling must not degenerate on: ViT's patch embedding (3072 matrices of 16 x 16, each
# smaller than a tile) and Llama-3-8B's output projection at its full height
SINGLE = {"patch_embed": [(1024, 3, 16, 16)], "lm_head": [(128256, 4096)]}
BYTES = {"fused_adafactor": 20.0, "fused_adafactor_nomaster": 12.0, "fused_adamw": 28.0}
FIELDS = {"vgprs": r"\bVGPRs: (\d+)", "agprs": r"AGPRs: (\d+)", "sgprs": r"SGPRs: (\d+)",
          "scratch_bytes_per_lane": r"ScratchSize \[bytes/lane\]: (\d+)",
          "lds_bytes_per_block": r"LDS Size \[bytes/block\]: (\d+)", "waves_per_simd": r"Occupancy \[waves/SIMD\]: (\d+)"}


def kernel_resources():
    """Compile adafactor.hip with the build's flags and -Rpass-analysis=kernel-resource-usage:
    ``{demangled kernel name: {field: value}}``."""
    ninja = _build.write_ninja().read_text().splitlines()
    flags = next(line for line in ninja if line.startswith("hipflags = "))[len("hipflags = "):]
    cmd = [str(_build.ROCM / "bin" / "hipcc"), *shlex.split(flags), *shlex.split(_build.EXTRA_HIP_FLAGS["adafactor.hip"]),
           "-Rpass-analysis=kernel-resource-usage", "-c", str(_build.CSRC / "kernels" / "adafactor.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
        for key, pat in FIELDS.items():
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    filt = shutil.which("llvm-cxxfilt", path=str(_build.ROCM / "lib" / "llvm" / "bin")) or shutil.which("c++filt")
    names = subprocess.run([filt, *kernels], capture_output=True, text=True).stdout.split("\n") if filt else []
    names += [""] * len(kernels)  # (no demangler: the mangled names)
    return {(n.split("(")[0].replace("void xddp::kernels::", "") if n else k): v for (k, v), n in zip(kernels.items(), names)}


def resource_lines(res):
    head = f"{'kernel':64s} {'VGPR':>5s} {'AGPR':>5s} {'SGPR':>5s} {'LDS B':>6s} {'scratch B/lane':>15s} {'waves/SIMD':>11s}"
    rows = [f"{k:64s} {v.get('vgprs', -1):5d} {v.get('agprs', -1):5d} {v.get('sgprs', -1):5d} "
            f"{v.get('lds_bytes_per_block', -1):6d} {v.get('scratch_bytes_per_lane', -1):15d} {v.get('waves_per_simd', -1):11d}"
            for k, v in sorted(res.items())]
    return ["kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):", head, *rows]


def state_bytes(opt, n):
    return sum(v.numel() * v.element_size() for st in opt.state.values() for v in st.values() if torch.is_tensor(v)) / n


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=float, default=0.25, help="fraction of Llama-3-8B's layers and vocabulary")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lists", default="vit_l,llama,patch_embed,lm_head")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r15_adafactor.txt"))
    ap.add_argument("--resources-only", action="store_true", help="compile and list the kernels; write --out as JSON")
    ap.add_argument("--resources-from", default=None, help="JSON written by --resources-only (skips the compile)")
    a = ap.parse_args(argv)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.resources_only:
        res = kernel_resources()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("\n".join(resource_lines(res)))
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("adafactor_bench.py measures the HIP kernels: no GPU found")
    if a.resources_from:
        with open(a.resources_from) as f:
            res = json.load(f)
    else:
        res = kernel_resources()
    dev = torch.device("cuda", 0)
    lines = [f"FusedAdafactor.step on {torch.cuda.get_device_name(0)}: medians of {a.steps} device-event timings per "
             f"variant, alternating, after {a.warmup} warm-up rounds; bf16 parameters and gradients", ""]
    result = {"scale": a.scale, "steps": a.steps}
    for name in a.lists.split(","):
        shapes = llama3_8b_shapes(a.scale) if name == "llama" else SINGLE.get(name) or model_shapes(name)
        params = make_params(shapes, torch.bfloat16, dev)
        n = sum(p.numel() for p in params)
        kw = dict(lr=1e-2, weight_decay=0.01)
        variants = {"fused_adafactor": FusedAdafactor(params, master_weights=True, **kw),
                    "fused_adafactor_nomaster": FusedAdafactor(params, **kw),
                    "fused_adamw": FusedAdamW(params, lr=1e-3, weight_decay=0.01, master_weights=True),
                    "torch_adafactor": torch.optim.Adafactor(params, foreach=False, **kw),
                    "torch_adafactor_foreach": torch.optim.Adafactor(params, foreach=True, **kw)}
        times = time_variants(variants, a.steps, a.warmup)
        med = {k: statistics.median(v) for k, v in times.items()}
        title = name + (f" (--scale {a.scale}: that fraction of the layers and of the vocabulary)" if name == "llama" else "")
        lines.append(f"{title}: {len(params)} tensors, {n / 1e6:.1f} M parameters")
        for k, v in times.items():
            model = f", {n * BYTES[k] / med[k] / 1e9:5.2f} TB/s by the byte model ({BYTES[k]:.0f} B/param)" if k in BYTES else ""
            lines.append(f"  {k:25s} {med[k]:9.3f} ms/step (min {min(v):.3f}, max {max(v):.3f}); optimizer state "
                         f"{state_bytes(variants[k], n):6.3f} B/param{model}")
        lines.append(f"  fused_adafactor / fused_adamw: {med['fused_adafactor'] / med['fused_adamw']:.3f} (byte model "
                     f"{20 / 28:.2f}); torch_adafactor / fused_adafactor_nomaster: "
                     f"{med['torch_adafactor'] / med['fused_adafactor_nomaster']:.2f}x; torch_adafactor_foreach / "
                     f"fused_adafactor_nomaster: {med['torch_adafactor_foreach'] / med['fused_adafactor_nomaster']:.2f}x")
        lines.append("")
        result[name] = {"tensors": len(params), "params": n, **{f"ms_{k}": v for k, v in med.items()},
                        **{f"state_bytes_{k}": state_bytes(o, n) for k, o in variants.items()}}
        del variants, params
        torch.cuda.empty_cache()
    lines += resource_lines(res)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
