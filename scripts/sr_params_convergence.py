#!/usr/bin/env python
"""Train llama_tiny (bf16) on fixed synthetic data with FusedAdamW in three configurations and print
the loss curves' end points: (a) fp32 master weights, (b) stochastically rounded parameters without
a master, (c) round-to-nearest parameters without a master. Same initial weights, data order and
seeds; the learning rate is small enough that most updates are below half a bf16 ulp of the weight,
where (c) drops them.

    python scripts/sr_params_convergence.py [--steps 400] [--lr 5e-5] [--state-bits 32]

A recorded run, not a test: prints one line per configuration and a final JSON line.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributeddataparallel_amd.models.llama import llama_tiny  # noqa: E402
from distributeddataparallel_amd.optim import FusedAdamW  # noqa: E402

CONFIGS = {"master": dict(master_weights=True), "stochastic": dict(param_rounding="stochastic"), "nearest": {}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--state-bits", type=int, default=32)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    gen = torch.Generator().manual_seed(0)
    # 128 fixed sequences of 64 tokens: a random walk over the vocabulary with small steps (learnable)
    steps = torch.randint(-3, 4, (128, 65), generator=gen)
    data = (torch.randint(0, 512, (128, 1), generator=gen) + steps.cumsum(1)).remainder(512).to(dev)
    order = [torch.randperm(128, generator=gen)[:a.batch] for _ in range(a.steps)]
    torch.manual_seed(0)
    init = llama_tiny().state_dict()
    result = {"steps": a.steps, "lr": a.lr, "state_bits": a.state_bits, "device": dev.type}

    def loss_of(model, rows):
        logits = model(rows[:, :-1])
        return F.cross_entropy(logits.float().reshape(-1, logits.shape[-1]), rows[:, 1:].reshape(-1))

    for name, kw in CONFIGS.items():
        model = llama_tiny()
        model.load_state_dict(init)
        model = model.to(dev, dtype=torch.bfloat16)
        opt = FusedAdamW(model.parameters(), lr=a.lr, weight_decay=0.0, state_bits=a.state_bits, seed=1, **kw)
        curve = []
        for it in range(a.steps):
            opt.zero_grad(set_to_none=True)
            loss = loss_of(model, data[order[it]])
            loss.backward()
            opt.step()
            curve.append(loss.item())
        with torch.no_grad():
            final = loss_of(model, data).item()
        first, last = sum(curve[:10]) / 10, sum(curve[-10:]) / 10
        print(f"{name:10s}: loss on all 128 sequences after {a.steps} steps {final:.4f}; "
              f"training loss, mean of the first 10 steps {first:.4f}, of the last 10 {last:.4f}")
        result[name] = {"final": final, "first10": first, "last10": last}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
