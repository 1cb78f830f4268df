#!/usr/bin/env python3
"""What the sampled leave-one-out evaluation costs at ml-20m shape; prints one JSON line.

The observed set is the synthetic ml-20m-shaped one of dev/cf_bench.py (138 493 users x 26 744 items, 20 M drawn pairs);
one observed item per user is held out and ranked against k = 99 distinct unobserved items.  Three things are measured:

  draw    ``ctr_eval_candidates`` over the 138 493 groups against a plain-PyTorch composition of the same stage:
          per chunk of users ``rand`` (users x items), the observed pairs and the positive masked out, ``topk`` k;
  rank    ``ctr_group_rank`` over the (groups, 1 + k) scores against ``(~(s[:, 1:] < s[:, :1])).sum(1)`` + ``bincount``;
  pass    the wall time of ``Trainer.rank_epoch`` with NeuralCF-64 over the 13.8 M candidate pairs.

The legs of draw and rank alternate inside every round, each timed by a host clock around calls that end in a device
synchronise; the result quotes the median and the spread over ``--rounds`` rounds.  The kernels' own times come from a
separate run under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_loo -- python dev/loo_bench.py --only-kernels
    python dev/loo_bench.py --stats-csv out/prof_loo/<...>_kernel_stats.csv --out profiles/loo_bench_ml20m.json
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
from deeplearningrecommendationsystem_amd import model as zoo  # noqa: E402
from deeplearningrecommendationsystem_amd import ops  # noqa: E402
from deeplearningrecommendationsystem_amd.data import LeaveOneOut  # noqa: E402
from deeplearningrecommendationsystem_amd.loss import BCELoss  # noqa: E402
from deeplearningrecommendationsystem_amd.trainer import Trainer  # noqa: E402
from _bench import observed_set  # noqa: E402

DEV = "cuda:0"


def torch_draw(users, items, observed, k, chunk, gen):
    """the same stage from library calls: k distinct unobserved items per group by random keys and topk"""
    out = torch.empty((users.shape[0], 1 + k), dtype=torch.int64, device=DEV)
    out[:, 0] = items
    indptr, indices = observed.indptr, observed.indices.long()
    for lo in range(0, users.shape[0], chunk):
        u = users[lo:lo + chunk]
        keys = torch.rand((u.shape[0], observed.num_items), device=DEV, generator=gen)
        start, stop = indptr[u], indptr[u + 1]
        rows = torch.repeat_interleave(torch.arange(u.shape[0], device=DEV), stop - start)
        offs = torch.arange(rows.shape[0], device=DEV) - torch.repeat_interleave((stop - start).cumsum(0) - (stop - start), stop - start)
        keys[rows, indices[torch.repeat_interleave(start, stop - start) + offs]] = -1.0
        keys[torch.arange(u.shape[0], device=DEV), items[lo:lo + chunk]] = -1.0
        out[lo:lo + chunk, 1:] = torch.topk(keys, k, dim=1).indices
    return out


def torch_rank(scores, k):
    rank = (~(scores[:, 1:] < scores[:, :1])).sum(1)
    return torch.bincount(rank, minlength=k + 1)


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
            if any(name in row["Name"] for name in ("eval_candidates_kernel", "group_rank_kernel")):
                out[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                    "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263)
    ap.add_argument("--negatives", type=int, default=99)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--chunk", type=int, default=4096, help="users per chunk of the PyTorch draw (chunk x items floats)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="kernel calls per timed window")
    ap.add_argument("--only-kernels", action="store_true", help="run the two kernels alone: the profiler's run")
    ap.add_argument("--stats-csv", help="rocprofv3 --stats kernel CSV of an --only-kernels run, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loo_bench.py needs the GPU: there is nothing to measure without one")
    k = a.negatives
    observed = observed_set(a)
    lengths = observed.indptr.diff()
    users = torch.nonzero(lengths > 0).flatten()                     # one held-out positive per user: its first item
    items = observed.indices[observed.indptr[users]].long()
    n = users.shape[0]
    err, fail = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    cand = torch.empty((n, 1 + k), dtype=torch.int64, device=DEV)
    scores = torch.rand((n, 1 + k), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    hist = torch.zeros(k + 1, dtype=torch.int64, device=DEV)

    def hip_draw():
        ops.eval_candidates(users, items, observed.indptr, observed.indices, a.users, a.items, k, 1, err, fail, out=cand)

    def hip_rank():
        ops.group_rank(scores, k, hist)

    if a.only_kernels:
        for _ in range(a.calls):
            hip_draw()
            hip_rank()
        torch.cuda.synchronize()
        return
    gen = torch.Generator(device=DEV).manual_seed(9)
    for fn in (hip_draw, hip_rank, lambda: torch_draw(users, items, observed, k, a.chunk, gen), lambda: torch_rank(scores, k)):
        fn()
    res = {"metric": "sampled_leave_one_out_evaluation", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "users": a.users, "items": a.items, "observed_pairs": len(observed), "groups": n, "negatives": k,
           "rounds": a.rounds, "calls_per_window": a.calls,
           "bytes": {"candidates_written": 8 * n * (1 + k), "scores_read_by_rank": 4 * n * (1 + k)}}
    td, tpd, tr, tpr = [], [], [], []
    for _ in range(a.rounds):
        td.append(timed(hip_draw, a.calls))
        tpd.append(timed(lambda: torch_draw(users, items, observed, k, a.chunk, gen), 1))
        tr.append(timed(hip_rank, a.calls))
        tpr.append(timed(lambda: torch_rank(scores, k), a.calls))
    assert int(err.item()) == 0 and int(fail.item()) == 0
    assert torch.equal(torch_rank(scores, k) * (hist.sum() // n), hist)
    res["draw"] = {"ctr_eval_candidates_call": stats(td), "pytorch_rand_mask_topk": stats(tpd)}
    res["rank"] = {"ctr_group_rank_call": stats(tr), "pytorch_compare_sum_bincount": stats(tpr)}
    # the scoring pass: NeuralCF-64 over every candidate pair, then the rank launch
    held_out = LeaveOneOut(users, items, observed, negatives=k, seed=1)
    torch.manual_seed(1234)
    with torch.device(DEV):
        net = zoo.NeuralCF(a.users, a.items, 64, [128, 64, 32, 16, 8])
    trainer = Trainer(net, BCELoss(), torch.optim.Adam(net.parameters(), lr=0.001))
    loader = held_out.pairs(a.batch)
    trainer.rank_epoch(loader, negatives=k)
    tp = [timed(lambda: trainer.rank_epoch(loader, negatives=k), 1) for _ in range(3)]
    held_out.check()
    res["pass"] = {"pairs": held_out.num_samples, "batch": a.batch, "batches": len(loader),
                   "rank_epoch_wall": stats(tp), "sample_bytes_on_device": 20 * held_out.num_samples}
    if a.stats_csv:
        res["kernels_rocprofv3"] = kernel_times(a.stats_csv)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
