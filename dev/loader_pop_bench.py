#!/usr/bin/env python3
"""What popularity-weighted negatives cost the grouped loader; prints one JSON line (profiles/loader_pop_bench.json).

The shape and the method are those of ``dev/loader_bench.py --neg-leg``: the NeuralCF step (ml-20m table sizes, batch
65536, captured) on the synthetic ml-20m-shaped observed set of dev/cf_bench.py, every replay preceded by one loader
launch.  Two legs that alternate inside every round of one process:

  (a) the grouped loader that draws its negatives uniformly (``ctr_load_batch_groups``);
  (b) the grouped loader with ``item_sampler=ItemSampler.popularity(observed, 0.75)`` (``ctr_load_batch_groups_pop``),
      log-q column written.

Each leg of a round is timed by a host clock around ``--seconds`` worth of steps that end in a device synchronise; the
result quotes the median and the spread (min, max) over ``--rounds`` rounds.  Per leg it also states the expected
tries per draw, computed on the host from the set: the mean over the positives of 1 / (1 - Q_u), Q_u the mass of user
u's observed items under the leg's distribution (uniform: row length / items; weighted: the table's q).  The loader
kernels' own times come from a profiler run of the same legs:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_pop -- python dev/loader_pop_bench.py --only-loader-leg
    python dev/loader_pop_bench.py --stats-csv out/prof_pop/<...>_kernel_stats.csv --out profiles/loader_pop_bench.json

``--uniform-only`` runs leg (a) alone and needs nothing of the weighted arm: it is what a checkout of the commit before
the weighted arm can run, for the comparison of the uniform kernels across the two builds (``--parent-stats-csv``,
``--parent-neg-stats-csv`` merge that build's profiler CSVs; ``--neg-stats-csv`` this build's
``dev/loader_bench.py --neg-leg`` one).
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
from deeplearningrecommendationsystem_amd.loss import BCELoss  # noqa: E402

DEV = "cuda:0"
KERNELS = ("load_batch_kernel", "load_batch_neg_kernel", "load_batch_groups_kernel", "load_batch_neg_pop_kernel",
           "load_batch_groups_pop_kernel")


def loader_kernel_times(path):
    """{kernel name: {calls, average_us, min_us, max_us}} of the loader kernels in a rocprofv3 --stats CSV"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if any(k in row["Name"] for k in KERNELS):
                out[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                    "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def run(a):
    batch, k = bench.batch_of("neuralcf"), a.negatives
    batch -= batch % (1 + k)
    rng = np.random.default_rng(0)                                   # the observed set of dev/cf_bench.py
    pop = 1.0 / np.arange(1, a.items + 1)
    pop = pop[rng.permutation(a.items)]
    u = torch.from_numpy(rng.integers(0, a.users, a.pairs)).to(DEV)
    i = torch.from_numpy(rng.choice(a.items, size=a.pairs, p=pop / pop.sum())).to(DEV)
    observed = ObservedPairs(u, i, a.users, a.items)
    rows = observed.indptr.diff()
    users = torch.repeat_interleave(torch.arange(a.users, device=DEV), rows)     # the positives: the distinct pairs
    items = observed.indices.long()
    n = users.shape[0]
    ones = torch.ones(n, 1, device=DEV)
    common = dict(seed=1, negatives=k, observed=observed, grouped=True)
    loaders = {"a_uniform": DeviceLoader.pairs(users, items, ones, batch, **common)}
    tries = {"a_uniform": float((1.0 / (1.0 - rows[users].double() / a.items)).mean())}
    if not a.uniform_only:
        from deeplearningrecommendationsystem_amd.data import ItemSampler
        sampler = ItemSampler.popularity(observed, a.alpha)
        loaders["b_weighted"] = DeviceLoader.pairs(users, items, ones, batch, item_sampler=sampler, **common)
        q = torch.from_numpy(sampler.q).to(DEV)
        mass = torch.zeros(a.users, dtype=torch.float64, device=DEV).index_add_(0, users, q[items])     # Q_u
        tries["b_weighted"] = float((1.0 / (1.0 - mass[users])).mean())
    loss_fn = BCELoss()

    def fed_step(loader):
        torch.manual_seed(1234)
        with torch.device(DEV):
            model = zoo.NeuralCF(a.users, a.items, 64, [128, 64, 32, 16, 8])
        args, rating = loader.static_batch()
        for _ in loader.epoch(0):
            break
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

    legs = {name: fed_step(loader) for name, loader in loaders.items()}

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6

    for leg in legs.values():
        leg(a.warmup)
    if a.only_loader_leg:
        for leg in legs.values():
            leg(a.warmup)
        torch.cuda.synchronize()
        return None
    steps = max(a.warmup, int(a.seconds * 1e6 / timed(legs["a_uniform"], a.warmup)))
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, leg in legs.items():
            times[name].append(timed(leg, steps))
    for loader in loaders.values():
        loader.check_bad_index()
    out = {"batch": batch, "negatives": k, "alpha": a.alpha, "users": a.users, "items": a.items, "positives": n,
           "positions_per_epoch": loaders["a_uniform"].num_samples, "steps_per_window": steps,
           "alias_table_bytes": 8 * a.items}
    for name, ts in times.items():
        out[name] = {"step": {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)},
                     "expected_tries_per_draw": tries[name]}
    if "b_weighted" in times:
        out["b_minus_a_us"] = statistics.median(times["b_weighted"]) - statistics.median(times["a_uniform"])
        out["per_round_b_minus_a_us"] = [b - x for x, b in zip(times["a_uniform"], times["b_weighted"])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="length of one timed window")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only-loader-leg", action="store_true", help="run the legs untimed: the profiler's run")
    ap.add_argument("--uniform-only", action="store_true", help="leg (a) alone (docstring)")
    ap.add_argument("--stats-csv", help="rocprofv3 --stats kernel CSV of an --only-loader-leg run, merged into the result")
    ap.add_argument("--neg-stats-csv", help="the same of `dev/loader_bench.py --neg-leg --only-loader-leg`")
    ap.add_argument("--parent-stats-csv", help="--stats-csv of the parent commit's build (--uniform-only)")
    ap.add_argument("--parent-neg-stats-csv", help="--neg-stats-csv of the parent commit's build")
    ap.add_argument("--merge-only", action="store_true", help="no run: merge the CSVs into the JSON of --into")
    ap.add_argument("--into", help="--merge-only: the JSON line to extend")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--negatives", type=int, default=4)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263)
    a = ap.parse_args()
    if a.merge_only:
        with open(a.into) as f:
            res = json.loads(f.readline())
    else:
        if not torch.cuda.is_available():
            raise SystemExit("loader_pop_bench.py needs the GPU: there is nothing to measure without one")
        res = {"metric": "weighted_grouped_loader_step_vs_uniform_grouped_loader_step", "argv": sys.argv[1:],
               "device": torch.cuda.get_device_name(0), "window_seconds": a.seconds, "rounds": a.rounds}
        out = run(a)
        if out is not None:
            res["neuralcf"] = out
    for key, path in (("this_build_pop_legs", a.stats_csv), ("this_build_neg_leg", a.neg_stats_csv),
                      ("parent_build_uniform_leg", a.parent_stats_csv), ("parent_build_neg_leg", a.parent_neg_stats_csv)):
        if path:
            res.setdefault("loader_kernels_rocprofv3", {})[key] = loader_kernel_times(path)
    if not a.only_loader_leg:
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
