#!/usr/bin/env python3
"""What the device-side loader adds to a training step; prints one JSON line.

Two legs per workload (NeuralCF of BASELINE configs[1] at batch 65536, DIN of configs[4] at batch 32768, the models
and the fixed batch exactly as bench.py builds them):

  (a) the step as ``GraphedStep`` replays it on one fixed batch -- what ``bench.py`` times;
  (b) the same captured step over the loader's static buffers, every replay preceded by one ``ctr_load_batch``
      launch that draws the next shuffled batch of a sample set of ``--batches`` (>= 64) batches.

The legs alternate inside every round and each leg of a round is timed by a host clock around ``--seconds`` worth of
steps that end in a device synchronise; the result quotes the median and the spread (min, max) over ``--rounds`` rounds.  The
loader kernel's own time comes from a separate run under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_ncf -- \
        python dev/loader_bench.py --only-loader-leg --workloads neuralcf        (and the same for din)
    python dev/loader_bench.py --stats-csv neuralcf=out/prof_ncf/<...>_kernel_stats.csv --stats-csv din=<...> \
        --out profiles/loader_bench.json

``--neg-leg`` is a leg of its own: the NeuralCF step (ml-20m table sizes, batch 65536) fed by (a) the plain loader over a
materialised set of every positive and ``--negatives`` fixed negatives per positive, and (b) the loader that is given
the positives alone and draws the negatives inside its launch (``negatives=``, ``observed=``), on a synthetic
ml-20m-shaped observed set built as dev/cf_bench.py builds it.  Same alternating rounds; the two loader kernels' times
come from a profiler run of the same leg:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_neg -- \
        python dev/loader_bench.py --neg-leg --only-loader-leg
    python dev/loader_bench.py --neg-leg --stats-csv neg=out/prof_neg/<...>_kernel_stats.csv \
        --out profiles/loader_neg_bench.json

Payload bytes per sample (``payload_bytes_per_sample``): what the kernel must read and write, counted from the shapes --
pairs: 8 + 8 + 4 read, the same written; sequences: user id 8, history row 8 L, target 8, rating 4 read, all but the
user id written.  The id and rating reads are random 4- and 8-byte accesses, each of which costs a whole 64-byte sector.
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
import bench  # noqa: E402  (make_model / make_inputs: the benchmark's own workloads)
from deeplearningrecommendationsystem_amd.data import DeviceLoader, ObservedPairs  # noqa: E402
from deeplearningrecommendationsystem_amd.graph import GraphedStep  # noqa: E402
from deeplearningrecommendationsystem_amd.loss import BCELoss  # noqa: E402

DEV = "cuda:0"
HIST_USERS = 138_493      # ml-20m's user count: one history row per user


def sample_set(name, batch, batches):
    """a loader over ``batches`` x ``batch`` samples drawn like the benchmark's batch"""
    gen = torch.Generator().manual_seed(99)
    n = batch * batches
    rating = (torch.rand(n, generator=gen) < 0.5).float().view(-1, 1).to(DEV)
    if name == "neuralcf":
        users = torch.randint(0, 943, (n,), generator=gen).to(DEV)
        items = torch.randint(0, 1682, (n,), generator=gen).to(DEV)
        return DeviceLoader.pairs(users, items, rating, batch, seed=1), 2 * (8 + 8 + 4)
    hist_len = 100
    history = torch.randint(0, 10_000_000, (HIST_USERS, hist_len), generator=gen).to(DEV)
    users = torch.randint(0, HIST_USERS, (n,), generator=gen).to(DEV)
    targets = torch.randint(0, 10_000_000, (n,), generator=gen).to(DEV)
    return DeviceLoader.sequences(history, users, targets, rating, batch, seed=1), 8 + 2 * (8 * hist_len + 8 + 4)


def legs(name, a):
    batch = bench.batch_of(name)
    loss_fn = BCELoss()
    with torch.device(DEV):
        model_a, model_b = bench.make_model(name), bench.make_model(name)
    inputs, y = bench.make_inputs(name, 0, batch)
    fixed = GraphedStep(model_a.to(DEV), loss_fn, [t.to(DEV) for t in inputs], y.to(DEV))
    loader, payload = sample_set(name, batch, a.batches)
    args, rating = loader.static_batch()
    for _ in loader.epoch(0):
        break                                    # the static buffers hold a valid batch before the capture reads them
    fed = GraphedStep(model_b.to(DEV), loss_fn, list(args), rating)

    def leg_a(steps):
        for _ in range(steps):
            fixed()

    def draws():
        epoch = 0
        while True:
            for _ in loader.epoch(epoch):        # one ctr_load_batch launch per batch
                yield
            epoch += 1

    feed = draws()

    def leg_b(steps):
        for _ in range(steps):
            next(feed)
            fed()

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6

    if a.only_loader_leg:
        leg_b(a.warmup)
        leg_b(4 * a.batches)
        torch.cuda.synchronize()
        return None
    leg_a(a.warmup)
    leg_b(a.warmup)
    # every timed window lasts about --seconds: a window of a few milliseconds would time the clock
    steps = max(a.warmup, int(a.seconds * 1e6 / timed(leg_b, a.warmup)))
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed(leg_a, steps))
        tb.append(timed(leg_b, steps))
    loader.check_bad_index()

    def stats(ts):
        return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}

    return {"batch": batch, "steps_per_window": steps, "samples": loader.num_samples, "batches_per_epoch": len(loader),
            "payload_bytes_per_sample": payload, "a_fixed_batch_step": stats(ta), "b_loader_fed_step": stats(tb),
            "b_minus_a_us": statistics.median(tb) - statistics.median(ta),
            "per_round_b_minus_a_us": [b - x for x, b in zip(ta, tb)]}


def neg_leg(a):
    """(a) plain loader over a materialised N * (1 + k) set against (b) the loader that draws, under one NeuralCF step"""
    import numpy as np
    from deeplearningrecommendationsystem_amd import model as zoo
    batch, k = bench.batch_of("neuralcf"), a.negatives
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
    drawing = DeviceLoader.pairs(users, items, ones, batch, seed=1, negatives=k, observed=observed)
    # (a): what a caller without the feature holds -- each positive followed by k negatives drawn once
    gen = torch.Generator(device=DEV).manual_seed(99)
    all_users = users.repeat_interleave(1 + k)
    all_items = torch.randint(0, a.items, (n * (1 + k),), generator=gen, device=DEV)
    all_items[::1 + k] = items
    all_rating = torch.zeros(n * (1 + k), 1, device=DEV)
    all_rating[::1 + k] = 1.0
    materialised = DeviceLoader.pairs(all_users, all_items, all_rating, batch, seed=1)
    assert materialised.num_samples == drawing.num_samples
    # a draw of user u is rejected with probability rows[u] / items: the mean number of tries over the positives
    tries = float((1.0 / (1.0 - rows[users].double() / a.items)).mean())

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

    leg_a, leg_b = fed_step(materialised), fed_step(drawing)

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6

    leg_a(a.warmup)
    leg_b(a.warmup)
    if a.only_loader_leg:
        leg_a(a.warmup)
        leg_b(a.warmup)
        torch.cuda.synchronize()
        return None
    steps = max(a.warmup, int(a.seconds * 1e6 / timed(leg_b, a.warmup)))
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed(leg_a, steps))
        tb.append(timed(leg_b, steps))
    for loader in (materialised, drawing):
        loader.check_bad_index()

    def stats(ts):
        return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}

    return {"batch": batch, "negatives": k, "users": a.users, "items": a.items, "positives": n,
            "positions_per_epoch": drawing.num_samples, "steps_per_window": steps,
            "sample_bytes_on_device": {"a_materialised": 20 * n * (1 + k), "b_positives_and_csr": 20 * n + 4 * n + 8 * (a.users + 1)},
            "expected_tries_per_draw_from_row_lengths": tries,
            "a_materialised_set_step": stats(ta), "b_drawn_negatives_step": stats(tb),
            "b_minus_a_us": statistics.median(tb) - statistics.median(ta),
            "per_round_b_minus_a_us": [b - x for x, b in zip(ta, tb)]}


def loader_kernel_times(path):
    """{kernel name: {calls, average_us, min_us, max_us}} of the loader kernels in a rocprofv3 --stats CSV"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if any(k in row["Name"] for k in ("load_batch_kernel", "load_batch_neg_kernel", "loader_indices_kernel")):
                out[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                    "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="neuralcf,din")
    ap.add_argument("--batches", type=int, default=64, help="batches in the loader's sample set (>= 64)")
    ap.add_argument("--seconds", type=float, default=0.5, help="length of one timed window")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only-loader-leg", action="store_true", help="run leg (b) alone: the profiler's run")
    ap.add_argument("--stats-csv", action="append", default=[], metavar="WORKLOAD=CSV",
                    help="rocprofv3 --stats kernel CSV of an --only-loader-leg run of one workload, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--neg-leg", action="store_true", help="the drawn-negatives leg instead of the workloads (docstring)")
    ap.add_argument("--negatives", type=int, default=4)
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench.py needs the GPU: there is nothing to measure without one")
    res = {"metric": "loader_fed_step_vs_fixed_batch_step", "argv": sys.argv[1:],
           "device": torch.cuda.get_device_name(0), "window_seconds": a.seconds, "rounds": a.rounds}
    if a.neg_leg:
        res["metric"] = "drawn_negatives_step_vs_materialised_set_step"
        out = neg_leg(a)
        if out is not None:
            res["neuralcf"] = out
    for name in [] if a.neg_leg else a.workloads.split(","):
        out = legs(name, a)
        if out is not None:
            res[name] = out
    for item in a.stats_csv:
        name, path = item.split("=", 1)
        res.setdefault("loader_kernels_rocprofv3", {})[name] = loader_kernel_times(path)
    if not a.only_loader_leg:
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
