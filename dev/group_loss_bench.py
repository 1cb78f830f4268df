#!/usr/bin/env python3
"""What training on a group loss costs beside the pointwise step; prints one JSON line.

Three legs under one captured NeuralCF step (64 / [128, 64, 32, 16, 8], ml-20m table sizes, k = ``--negatives`` drawn
negatives per positive, batch = the benchmark's 65536 rounded down to a multiple of 1 + k), on the synthetic
ml-20m-shaped observed set of dev/loader_bench.py --neg-leg:

  (a) ungrouped loader (``ctr_load_batch_neg``) + ``BCELoss``: the pointwise path;
  (b) grouped loader (``ctr_load_batch_groups``) + ``BPRLoss``;
  (c) grouped loader + ``SampledSoftmaxLoss``.

Every replay is preceded by the loader launch that draws the next batch.  The legs alternate inside every round and each
leg of a round is timed by a host clock around ``--seconds`` worth of steps that end in a device synchronise; the result
quotes the median and the spread over ``--rounds`` rounds.  Read (b) and (c) against (a), never against themselves.  The
loader and loss kernels' own times come from a separate run under the profiler (no counters in that run):

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_group -- \
        python dev/group_loss_bench.py --only-profile-legs
    python dev/group_loss_bench.py --stats-csv out/prof_group/<...>_kernel_stats.csv --out profiles/group_loss_bench.json
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (batch_of: the benchmark's own batch)
from deeplearningrecommendationsystem_amd import model as zoo  # noqa: E402
from deeplearningrecommendationsystem_amd.data import DeviceLoader, ObservedPairs  # noqa: E402
from deeplearningrecommendationsystem_amd.graph import GraphedStep  # noqa: E402
from deeplearningrecommendationsystem_amd.loss import BCELoss, BPRLoss, SampledSoftmaxLoss  # noqa: E402

DEV = "cuda:0"
KERNELS = ("load_batch_neg_kernel", "load_batch_groups_kernel", "bce_fwd_kernel", "group_loss_fwd_kernel",
           "group_loss_bwd_kernel")


def fed_step(loader, loss_fn, a):
    """leg(steps): one loader launch and one replay of the step captured over the loader's static buffers, per step"""
    torch.manual_seed(1234)
    with torch.device(DEV):
        model = zoo.NeuralCF(a.users, a.items, 64, [128, 64, 32, 16, 8])
    args, rating = loader.static_batch()
    for _ in loader.epoch(0):
        break                                    # the static buffers hold a valid batch before the capture reads them
    step = GraphedStep(model, loss_fn, list(args), rating)

    def draws():
        epoch = 0
        while True:
            for first, count in loader.ranges[:loader._num_full]:     # full batches only: the tail is not captured
                loader._launch(loader._full, epoch, first, count, True)
                yield
            epoch += 1
    feed = draws()

    def leg(steps):
        for _ in range(steps):
            next(feed)
            step()
    return leg


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def kernel_times(path):
    """{kernel name: {calls, average_us, min_us, max_us}} of the loader and loss kernels in a rocprofv3 --stats CSV"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if any(k in row["Name"] for k in KERNELS):
                out[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                    "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="length of one timed window")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--negatives", type=int, default=4)
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263)
    ap.add_argument("--only-profile-legs", action="store_true", help="run every leg for --warmup steps: the profiler's run")
    ap.add_argument("--stats-csv", help="rocprofv3 --stats kernel CSV of an --only-profile-legs run, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_loss_bench.py needs the GPU: there is nothing to measure without one")
    k = a.negatives
    batch = bench.batch_of("neuralcf") // (1 + k) * (1 + k)
    rng = np.random.default_rng(0)                                   # the observed set of dev/cf_bench.py
    pop = 1.0 / np.arange(1, a.items + 1)
    pop = pop[rng.permutation(a.items)]
    u = torch.from_numpy(rng.integers(0, a.users, a.pairs)).to(DEV)
    i = torch.from_numpy(rng.choice(a.items, size=a.pairs, p=pop / pop.sum())).to(DEV)
    observed = ObservedPairs(u, i, a.users, a.items)
    users = torch.repeat_interleave(torch.arange(a.users, device=DEV), observed.indptr.diff())   # the distinct pairs
    items = observed.indices.long()
    ones = torch.ones(users.shape[0], 1, device=DEV)

    def loader(grouped):
        return DeviceLoader.pairs(users, items, ones, batch, seed=1, negatives=k, observed=observed, grouped=grouped)

    loaders = {"a_ungrouped_bce": loader(False), "b_grouped_bpr": loader(True), "c_grouped_softmax": loader(True)}
    losses = {"a_ungrouped_bce": BCELoss(), "b_grouped_bpr": BPRLoss(k), "c_grouped_softmax": SampledSoftmaxLoss(k)}
    legs = {name: fed_step(loaders[name], losses[name], a) for name in loaders}
    for leg in legs.values():
        leg(a.warmup)
    torch.cuda.synchronize()
    if a.only_profile_legs:
        return
    steps = max(a.warmup, int(a.seconds * 1e6 / timed(legs["b_grouped_bpr"], a.warmup)))
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, leg in legs.items():
            times[name].append(timed(leg, steps))
    for ld in loaders.values():
        ld.check_bad_index()
    res = {"metric": "group_loss_step_vs_pointwise_step", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "window_seconds": a.seconds, "rounds": a.rounds, "batch": batch, "negatives": k, "users": a.users,
           "items": a.items, "positives": int(users.shape[0]), "steps_per_window": steps}
    for name, ts in times.items():
        res[name] = {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}
    base = times["a_ungrouped_bce"]
    for name in ("b_grouped_bpr", "c_grouped_softmax"):
        res[name]["minus_a_us"] = statistics.median(times[name]) - statistics.median(base)
        res[name]["per_round_minus_a_us"] = [t - x for x, t in zip(base, times[name])]
    if a.stats_csv:
        res["kernels_rocprofv3"] = kernel_times(a.stats_csv)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
