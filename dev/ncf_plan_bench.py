"""NeuralCF step (forward + BCELoss + backward, hipGraph replay) at a batch and id order bench.py does not offer:
    python dev/ncf_plan_bench.py [--batch N] [--order uniform|by_user|by_item] [--steps K] [--warmup W]
Run from the root of the tree to be measured (the package is imported from the working directory, so the same script
times a parent checkout beside the change).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.getcwd())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--order", default="uniform", choices=["uniform", "by_user", "by_item"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from deeplearningrecommendationsystem_amd import synth
    from deeplearningrecommendationsystem_amd.graph import GraphedStep
    from deeplearningrecommendationsystem_amd.loss import BCELoss
    from deeplearningrecommendationsystem_amd.model import NeuralCF
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = NeuralCF(943, 1682, 64, [128, 64, 32, 16, 8]).to(dev)
    model.train()
    gen = synth.generator(7)
    u, i = synth.id_batch(a.batch, gen=gen)
    if a.order != "uniform":
        order = torch.argsort(u if a.order == "by_user" else i, stable=True)
        u, i = u[order], i[order]
    y = synth.labels(a.batch, True, gen)
    step = GraphedStep(model, BCELoss(), [u.to(dev), i.to(dev)], y.to(dev))
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / a.steps * 1e6
    print(json.dumps({"metric": "neuralcf fwd+bwd step, hipGraph replay", "batch": a.batch, "order": a.order,
                      "us_per_step": us, "steps": a.steps, "warmup": a.warmup, "loss": float(loss.item())}))


if __name__ == "__main__":
    main()
