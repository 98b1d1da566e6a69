#!/usr/bin/env python
"""Time FusedLAMB.step and FusedLARS.step against the fused optimizers without a trust ratio and
against ``torch._foreach`` implementations of the same formulas (what a user would write today).

    python scripts/layerwise_optim_bench.py                 # Llama-3-8B at --scale 0.25, ViT-L, ResNet-50
    python scripts/layerwise_optim_bench.py --scale 0.125

Per list, every variant steps the same parameter and gradient tensors (each with its own states and
masters), alternating in one process after a warm-up; times are medians of device-event timings.
LAMB lists: bf16 parameters and gradients, fp32 masters. The byte model per parameter: AdamW 28 B
(master and both moments read + written, gradient read, parameter written); LAMB 40 B (stage 1 reads
master, gradient and both moments and writes the moments: 22 B; stage 3 reads master and moments and
writes master and parameter: 18 B), 40 / 28 = 1.43. The ResNet-50 list is fp32 with momentum: SGD
20 B (parameter, momentum read + written, gradient read), LARS 28 B (+ one read of w and g), 1.40.
The only pass condition: the fused step is faster than the _foreach one on every list (exit status 1
otherwise). Prints one line per variant and a final JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributeddataparallel_amd.optim import FusedAdamW, FusedLAMB, FusedLARS, FusedSGD  # noqa: E402

LAMB = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
LARS = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, trust_coefficient=1e-3, eps=1e-8)


def llama3_8b_shapes(scale):
    dim, ffn, kv, vocab, layers = 4096, 14336, 1024, 128256, 32
    layers = max(1, round(layers * scale))
    vocab = max(128, int(vocab * scale) // 128 * 128)
    shapes = [(vocab, dim)]
    for _ in range(layers):
        shapes += [(dim,), (dim, dim), (kv, dim), (kv, dim), (dim, dim), (dim,), (ffn, dim), (dim, ffn), (ffn, dim)]
    return shapes + [(dim,), (vocab, dim)]


def model_shapes(name):
    from distributeddataparallel_amd import models
    with torch.device("meta"):
        m = models.vit.vit_l_16() if name == "vit_l" else models.resnet.resnet50()
    return [tuple(p.shape) for p in m.parameters()]


class ForeachLAMB:
    """LAMB with fp32 masters in torch._foreach ops, one list op per operation."""

    def __init__(self, params):
        self.params = params
        self.w = [p.detach().float() for p in params]
        self.m = [torch.zeros_like(w) for w in self.w]
        self.v = [torch.zeros_like(w) for w in self.w]
        self.g = [torch.empty_like(w) for w in self.w]
        self.t = 0

    @torch.no_grad()
    def step(self):
        self.t += 1
        b1, b2 = LAMB["betas"]
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        torch._foreach_copy_(self.g, [p.grad for p in self.params])
        torch._foreach_mul_(self.m, b1)
        torch._foreach_add_(self.m, self.g, alpha=1 - b1)
        torch._foreach_mul_(self.v, b2)
        torch._foreach_addcmul_(self.v, self.g, self.g, value=1 - b2)
        den = torch._foreach_sqrt(self.v)
        torch._foreach_div_(den, math.sqrt(bc2))
        torch._foreach_add_(den, LAMB["eps"])
        u = torch._foreach_div(self.m, den)
        torch._foreach_div_(u, bc1)
        torch._foreach_add_(u, self.w, alpha=LAMB["weight_decay"])
        wn, un = torch.stack(torch._foreach_norm(self.w)), torch.stack(torch._foreach_norm(u))
        r = torch.where((wn != 0) & (un != 0), wn / un, torch.ones_like(wn)) * -LAMB["lr"]
        torch._foreach_mul_(u, r.unbind(0))
        torch._foreach_add_(self.w, u)
        torch._foreach_copy_(self.params, self.w)


class ForeachLARS:
    """LARS over momentum SGD on fp32 parameters in torch._foreach ops."""

    def __init__(self, params):
        self.params = params
        self.buf = None

    @torch.no_grad()
    def step(self):
        ps = [p.detach() for p in self.params]
        gs = [p.grad for p in self.params]
        wd = LARS["weight_decay"]
        wn, gn = torch.stack(torch._foreach_norm(ps)), torch.stack(torch._foreach_norm(gs))
        lam = torch.where((wn != 0) & (gn != 0), LARS["trust_coefficient"] * wn / (gn + wd * wn + LARS["eps"]),
                          torch.ones_like(wn))
        d = torch._foreach_add(gs, ps, alpha=wd)
        torch._foreach_mul_(d, lam.unbind(0))
        if self.buf is None:
            self.buf = [x.clone() for x in d]
        else:
            torch._foreach_mul_(self.buf, LARS["momentum"])
            torch._foreach_add_(self.buf, d)
        torch._foreach_add_(ps, self.buf, alpha=-LARS["lr"])


def make_params(shapes, dtype, dev):
    params = []
    for shape in shapes:
        p = torch.nn.Parameter(torch.empty(shape, device=dev, dtype=dtype).normal_(0, 0.02))
        p.grad = torch.empty_like(p).normal_(0, 1e-3)
        params.append(p)
    return params


def time_variants(variants, steps, warmup):
    times = {k: [] for k in variants}
    for it in range(warmup + steps):
        for name, opt in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            opt.step()
            t1.record()
            t1.synchronize()
            if it >= warmup:
                times[name].append(t0.elapsed_time(t1))
    return times


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=float, default=0.25, help="fraction of Llama-3-8B's layers and vocabulary")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lists", default="llama,vit_l,resnet50")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("layerwise_optim_bench.py measures the HIP kernels: no GPU found")
    dev = torch.device("cuda", 0)
    result, ok = {"scale": a.scale, "steps": a.steps}, True
    for name in a.lists.split(","):
        lamb = name != "resnet50"
        shapes = llama3_8b_shapes(a.scale) if name == "llama" else model_shapes(name)
        params = make_params(shapes, torch.bfloat16 if lamb else torch.float32, dev)
        n = sum(p.numel() for p in params)
        if lamb:
            variants = {"fused_lamb": FusedLAMB(params, master_weights=True, **LAMB),
                        "fused_adamw": FusedAdamW(params, lr=LAMB["lr"], betas=LAMB["betas"], eps=LAMB["eps"],
                                                  weight_decay=LAMB["weight_decay"], master_weights=True),
                        "foreach_lamb": ForeachLAMB(params)}
            new, base, naive, bytes_new, bytes_base = "fused_lamb", "fused_adamw", "foreach_lamb", 40.0, 28.0
        else:
            sgd = {k: LARS[k] for k in ("lr", "momentum", "weight_decay")}
            variants = {"fused_lars": FusedLARS(params, **LARS), "fused_sgd": FusedSGD(params, **sgd),
                        "foreach_lars": ForeachLARS(params)}
            new, base, naive, bytes_new, bytes_base = "fused_lars", "fused_sgd", "foreach_lars", 28.0, 20.0
        times = time_variants(variants, a.steps, a.warmup)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"{name}: {len(params)} tensors, {n / 1e6:.1f} M parameters")
        for k, v in times.items():
            moved = n * (bytes_new if k == new else bytes_base) if k != naive else float("nan")
            print(f"  {k:13s} {med[k]:9.3f} ms/step (min {min(v):.3f}, max {max(v):.3f})"
                  + (f", {moved / med[k] / 1e9:5.2f} TB/s by the byte model" if k != naive else ""))
        print(f"  {new} / {base}: {med[new] / med[base]:.3f} (byte model {bytes_new / bytes_base:.2f}); "
              f"{naive} / {new}: {med[naive] / med[new]:.2f}x")
        result[name] = {"tensors": len(params), "params": n, **{f"ms_{k}": v for k, v in med.items()},
                        "ratio_to_base": med[new] / med[base], "byte_model": bytes_new / bytes_base,
                        "speedup_over_foreach": med[naive] / med[new]}
        ok = ok and med[new] < med[naive]
        del variants, params
        torch.cuda.empty_cache()
    result["fused_beats_foreach"] = ok
    print(json.dumps(result))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
