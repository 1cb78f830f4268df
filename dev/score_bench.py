#!/usr/bin/env python3
"""What the score-level evaluation costs at ml-20m shape; prints one JSON line.

138 493 users and 14.8 M samples with synthetic labels (Bernoulli 0.3) and scores (uniform); the samples per user
follow the activity law of ``synth.implicit_split`` (weight ``rand^3 + 0.05``, a multinomial draw), and the users
interleave.  Two things are measured:

  pointwise  ``ctr_score_counts`` plus the two small copies ``score_metrics`` makes, against the torch composition it
             replaces: ``Evaluator.eval`` (five numbers, about ten passes) plus ``torch.nn.BCELoss`` read back;
  gauc       the ``ctr_gauc_groups`` launch pair alone over the plan of the set, with its pair evaluations per second
             (the cost model: sum over groups of size x size rounded up to slabs).

The legs of pointwise alternate inside every round, each timed by a host clock around calls that end in a device
synchronise; the result quotes the median and the spread over ``--rounds`` rounds.  The kernels' own times come from a
separate run under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_score -- python dev/score_bench.py --only-kernels
    python dev/score_bench.py --stats-csv out/prof_score/<...>_kernel_stats.csv --out profiles/score_bench_ml20m.json
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeplearningrecommendationsystem_amd import ops  # noqa: E402
from deeplearningrecommendationsystem_amd.evaluator import Evaluator, UserGroups, gauc_from_counts, score_metrics  # noqa: E402

DEV = "cuda:0"
KERNELS = ("score_counts_kernel", "gauc_small_kernel", "gauc_slab_kernel")


def sample_users(a):
    """(N,) int64 user of every sample: sizes by the activity law of synth.implicit_split, the users interleaved"""
    gen = torch.Generator().manual_seed(5)
    activity = torch.rand(a.users, generator=gen, dtype=torch.float64) ** 3 + 0.05
    users = torch.multinomial(activity, a.samples, replacement=True, generator=gen)
    return users.to(DEV)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def stats(ts):
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}


def kernel_times(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if any(name in row["Name"] for name in KERNELS):
                out[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                    "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--samples", type=int, default=14_800_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--only-kernels", action="store_true", help="run the kernels alone: the profiler's run")
    ap.add_argument("--stats-csv", help="rocprofv3 --stats kernel CSV of an --only-kernels run, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bench.py needs the GPU: there is nothing to measure without one")
    n = a.samples
    gen = torch.Generator(device=DEV).manual_seed(3)
    p = torch.rand(n, device=DEV, generator=gen)
    y = (torch.rand(n, device=DEV, generator=gen) < 0.3).float()
    groups = UserGroups(sample_users(a))
    g = groups.num_groups
    counts = torch.zeros(8, dtype=torch.int64, device=DEV)
    sums = torch.empty((-(-n // ops.SCORE_CHUNK), 4), dtype=torch.float64, device=DEV)
    pos, neg = (torch.zeros(g, dtype=torch.int32, device=DEV) for _ in range(2))
    u2 = torch.zeros(g, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    bce = torch.nn.BCELoss()

    def hip_pointwise():
        counts.zero_()
        ops.score_counts(p, y, counts, sums)
        return counts.cpu(), sums.cpu()

    def torch_pointwise():
        return Evaluator.eval(y, p), float(bce(p, y))

    def hip_gauc():
        u2.zero_()
        ops.gauc_groups(p, y, groups.order, groups.offsets, groups.small_groups, groups.slab_group, groups.slab_first,
                        pos, neg, u2, err)

    if a.only_kernels:
        for _ in range(a.calls):
            ops.score_counts(p, y, counts, sums)
            hip_gauc()
        torch.cuda.synchronize()
        return
    for fn in (hip_pointwise, torch_pointwise, hip_gauc):
        fn()
    sizes = groups.sizes()
    pairs = groups.pair_evaluations()
    res = {"metric": "score_level_evaluation", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "users": g, "samples": n, "rounds": a.rounds, "calls_per_window": a.calls,
           "groups": {"max": groups.max_group, "median": float(sizes.median()), "small": int(groups.small_groups.numel()),
                      "slabs": int(groups.slab_group.numel())},
           "pair_evaluations": pairs, "bytes": {"score_counts_read": 8 * n, "gauc_read_once": 12 * n}}
    th, tt, tg = [], [], []
    for _ in range(a.rounds):
        th.append(timed(hip_pointwise, a.calls))
        tt.append(timed(torch_pointwise, a.calls))
        tg.append(timed(hip_gauc, a.calls))
    assert int(err.item()) == 0
    metrics = score_metrics(y, p, groups)
    shared = Evaluator.eval(y, p)
    assert all(abs(m - w) <= 1e-4 for m, w in zip(metrics[3:8], shared)), (metrics, shared)
    assert abs(metrics.logloss - float(bce(p, y))) <= 1e-4 * metrics.logloss
    assert gauc_from_counts(pos, neg, u2).gauc == metrics.gauc
    res["pointwise"] = {"ctr_score_counts_and_copies": stats(th), "pytorch_evaluator_eval_bceloss": stats(tt)}
    res["gauc"] = {"ctr_gauc_groups_launch_pair": stats(tg),
                   "pair_evaluations_per_s": pairs / (statistics.median(tg) * 1e-6)}
    res["values"] = {"logloss": metrics.logloss, "auc": metrics.auc, "gauc": metrics.gauc,
                     "users_scored": metrics.users_scored}
    if a.stats_csv:
        res["kernels_rocprofv3"] = kernel_times(a.stats_csv)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
