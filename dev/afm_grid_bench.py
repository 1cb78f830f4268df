#!/usr/bin/env python3
"""AFM over the user x item grid at ml-20m table sizes (138 493 users x 26 744 items, attention_dim 64) at E = 16 (the
small end of what the kernel admits) and E = 128 (the reference script's shape); prints one JSON line.

Two ways to score a slice of ``--rows`` users against every item (4096 x 26 744 = 1.1e8 pairs), on one model:

  (a) grid     ``scorer.score_rows(0, rows)``: the user-side and item-side table rows (ctr_embed_fwd, ctr_pairprod_fwd,
               three ctr_linear_fwd a pass, the softmax summaries), then ``ctr_afm_grid_scores``;
  (b) forward  the chunked forward path every feature model gets: ``assembler.feature`` and ``model.forward`` under
               ``no_grad``, 2^18 pairs a call (``FeatureModel.catalogue_scorer``'s scorer on the same model).

The two legs alternate inside every round, each timed by a host clock around calls that end in a device synchronise;
the result quotes the median and the spread over ``--rounds`` rounds, pairs per second for both and their ratio, and
the time of the table rows alone (``scorer._shared()``), hence their share of leg (a).  With ``--recommend`` it also
reports the wall time of ``recommend(n=20)`` for EVERY user with the observed set of dev/cf_bench.py left out.  The
kernel's own time, and with it its share of the 155 TF fp32 matrix-core rate (counting the attention map alone, 2 x 8 x
E x 64 flop a pair: the bound is 1.18e9 pairs/s at E = 128), comes from a separate run under the
profiler, of leg (a) alone:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_afm_grid -- python dev/afm_grid_bench.py --only-kernels --embed 128
    python dev/afm_grid_bench.py --stats-csv 128=out/prof_afm_grid/<...>_kernel_stats.csv --out profiles/afm_grid_bench.json
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
from deeplearningrecommendationsystem_amd import model as zoo  # noqa: E402
from deeplearningrecommendationsystem_amd import synth  # noqa: E402
from deeplearningrecommendationsystem_amd.data import FeatureAssembler, ObservedPairs  # noqa: E402
from deeplearningrecommendationsystem_amd.model._base import CatalogueScorer  # noqa: E402

DEV = "cuda:0"
F32_MFMA_PEAK = 155e12
ATTENTION = 64


def map_flop_per_pair(embed):
    return 2 * 8 * embed * ATTENTION                                 # the attention map of the eight cross products


def flop_per_pair(embed):
    # per cross product: the product itself, the map, bias + relu + the dot with h, the dot with o, the softmax merge
    return 8 * (embed + 2 * embed * ATTENTION + 4 * ATTENTION + 2 * embed + 8)


def observed_set(a):
    rng = np.random.default_rng(0)                                   # the observed set of dev/cf_bench.py
    pop = 1.0 / np.arange(1, a.items + 1)
    pop = pop[rng.permutation(a.items)]
    u = torch.from_numpy(rng.integers(0, a.users, a.pairs)).to(DEV)
    i = torch.from_numpy(rng.choice(a.items, size=a.pairs, p=pop / pop.sum())).to(DEV)
    return ObservedPairs(u, i, a.users, a.items)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def kernel_times(path):
    """the library's kernels of an --only-kernels run"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "(anonymous namespace)::" in row["Name"] and "at::native" not in row["Name"]:
                name = row["Name"].split("(anonymous namespace)::")[1].split("(")[0].split("<")[0]
                prev = out.get(name, {"calls": 0, "total_ms": 0.0})
                calls, total = prev["calls"] + int(row["Calls"]), prev["total_ms"] + float(row["TotalDurationNs"]) / 1e6
                out[name] = {"calls": calls, "total_ms": total, "average_us": total * 1e3 / calls}
    return out


def build(a, embed):
    torch.manual_seed(1234)
    with torch.device(DEV):
        net = zoo.AFM(a.users, a.items, embed, ATTENTION).eval()
    users = synth.feature_batch(a.users, gen=synth.generator(11))[:, 2:26]
    items = synth.feature_batch(a.items, gen=synth.generator(12))[:, 26:45]
    asm = FeatureAssembler(users.to(DEV), items.to(DEV))
    return net, asm


def measure(a, embed, observed):
    net, asm = build(a, embed)
    grid_scorer, forward_scorer = net.catalogue_scorer(asm), CatalogueScorer(net, asm)
    assert grid_scorer.path == "grid" and forward_scorer.path == "forward"
    rows, pairs = a.rows, a.rows * a.items
    got = grid_scorer.score_rows(0, rows)
    want = forward_scorer.score_rows(0, rows)
    worst = float((got - want).abs().max())
    assert worst <= 1e-5, worst                                      # the two legs score the same function
    del got, want
    res = {"embedding_dim": embed, "flop_per_pair": flop_per_pair(embed), "map_flop_per_pair": map_flop_per_pair(embed),
           "max_abs_difference_between_legs": worst}
    ta, tb, tr = [], [], []
    for _ in range(a.rounds):
        ta.append(timed(lambda: grid_scorer.score_rows(0, rows)))
        tb.append(timed(lambda: forward_scorer.score_rows(0, rows)))
        with torch.no_grad():
            tr.append(timed(grid_scorer._shared))
    ma, mb, mr = statistics.median(ta), statistics.median(tb), statistics.median(tr)
    res["grid"] = dict(stats(ta), pairs_per_s=pairs / ma)
    res["forward"] = dict(stats(tb), pairs_per_s=pairs / mb)
    res["grid_over_forward_pairs_per_s"] = mb / ma
    res["table_rows"] = dict(stats(tr), share_of_grid_leg=mr / ma)
    if observed is not None:
        grid_scorer.recommend(users=list(range(64)), n=20, exclude=observed)
        t = timed(lambda: grid_scorer.recommend(n=20, exclude=observed))
        res["recommend_all_users_n20"] = {"wall_s": t, "observed_pairs": len(observed), "pairs_scored": a.users * a.items,
                                          "pairs_per_s": a.users * a.items / t}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263, help="drawn pairs of the observed set (distinct ones are fewer)")
    ap.add_argument("--rows", type=int, default=4096, help="users of the timed slice")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--embed", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--only-kernels", action="store_true", help="a few calls of leg (a) alone: the profiler's run")
    ap.add_argument("--recommend", action="store_true", help="also time recommend(n=20) for every user")
    ap.add_argument("--stats-csv", action="append", default=[], metavar="E=PATH",
                    help="rocprofv3 --stats kernel CSV of an --only-kernels --embed E run, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("afm_grid_bench.py needs the GPU: there is nothing to measure without one")
    if a.only_kernels:
        for embed in a.embed:
            net, asm = build(a, embed)
            scorer = net.catalogue_scorer(asm)
            for _ in range(5):
                scorer.score_rows(0, a.rows)
        torch.cuda.synchronize()
        return
    pairs = a.rows * a.items
    res = {"metric": "afm_grid_scores_ml20m_tables", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "users": a.users, "items": a.items, "attention_dim": ATTENTION, "slice_rows": a.rows, "slice_pairs": pairs,
           "rounds": a.rounds, "forward_pairs_per_call": 1 << 18, "shapes": []}
    observed = observed_set(a) if a.recommend else None
    csvs = dict(s.split("=", 1) for s in a.stats_csv)
    for embed in a.embed:
        r = measure(a, embed, observed)
        if str(embed) in csvs:
            k = kernel_times(csvs[str(embed)])
            r["kernels_rocprofv3"] = k
            for name, v in k.items():
                if "afm_grid_scores_kernel" in name:
                    flops = map_flop_per_pair(embed) * pairs / (v["average_us"] * 1e-6)
                    r["grid_kernel"] = {"average_us": v["average_us"], "map_tflops": flops / 1e12,
                                        "share_of_fp32_mfma_peak": flops / F32_MFMA_PEAK,
                                        "pairs_per_s": pairs / (v["average_us"] * 1e-6)}
        res["shapes"].append(r)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
