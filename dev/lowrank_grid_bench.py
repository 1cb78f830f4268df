#!/usr/bin/env python3
"""MatrixFactorization, FFM, LogisticRegression and Wide & Deep over the user x item grid at ml-20m table sizes
(138 493 users x 26 744 items); prints one JSON line.  The timed slice is ``--rows`` users against every item (4096 x
26 744 = 1.1e8 pairs, 438 MB of scores).

  (a) MF grid     ``MatrixFactorization(U, I, 64).score_rows(0, rows)``: ``ctr_lowrank_grid_scores`` over the two weight
                  tables as they are;
  (b) MF before   what the library offered for the same scores before the grid interface: ``ops.linear_fwd(P[0:rows], Q)``
                  into a score matrix, then ``sigmoid_()`` over it;
  (c) FFM k = 32, LogisticRegression and Wide & Deep E = 128: the model's grid scorer (``catalogue_scorer``) against the
                  chunked forward path every feature model gets (``CatalogueScorer`` on the same model: ``assembler.
                  feature`` and ``model.forward`` under ``no_grad``, 2^18 pairs a call);
  (d) store floor a ``fill_`` of the same (rows, items) score buffer: what this machine takes to write 438 MB once.

The legs alternate inside every round; a window is ``--calls`` back-to-back calls of a short leg (one call of a forward
leg, which runs for a second), timed by a host clock around work that ends in a device synchronise, and the result
quotes the median and the spread over ``--rounds`` windows.  (a)'s score bytes per second are reported as a fraction of
(d)'s.  With ``--recommend`` it also reports the wall time of ``recommend(n=20)`` for EVERY user, with the observed set of
dev/cf_bench.py left out, for MF and Wide & Deep.  Kernel times come from a separate run under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_lowrank_grid -- python dev/lowrank_grid_bench.py --only-kernels
    python dev/lowrank_grid_bench.py --recommend --stats-csv out/prof_lowrank_grid/<...>_kernel_stats.csv --out profiles/lowrank_grid_bench.json
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
from deeplearningrecommendationsystem_amd import ops, synth  # noqa: E402
from deeplearningrecommendationsystem_amd.data import FeatureAssembler, ObservedPairs  # noqa: E402
from deeplearningrecommendationsystem_amd.model._base import CatalogueScorer  # noqa: E402

DEV = "cuda:0"
F32_MFMA_PEAK = 155e12
STORE_PEAK = 6.0e12          # plain stores, MI355X_MICROARCH.md
MF_RANK, FFM_RANK, WD_EMBED, WD_HIDDEN = 64, 32, 128, [512, 256, 128, 1]


def observed_set(a):
    rng = np.random.default_rng(0)                                   # the observed set of dev/cf_bench.py
    pop = 1.0 / np.arange(1, a.items + 1)
    pop = pop[rng.permutation(a.items)]
    u = torch.from_numpy(rng.integers(0, a.users, a.pairs)).to(DEV)
    i = torch.from_numpy(rng.choice(a.items, size=a.pairs, p=pop / pop.sum())).to(DEV)
    return ObservedPairs(u, i, a.users, a.items)


def timed(fn, calls=1):
    """seconds per call of ``calls`` back-to-back calls that end in one device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def kernel_times(path):
    """the kernels of an --only-kernels run: the library's by name (template arguments kept), torch's fill and sigmoid"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "(anonymous namespace)::" in name and "at::native" not in name:
                name = name.split("(anonymous namespace)::")[1].split("(")[0]
            elif "FillFunctor" in name:
                name = "torch_fill"
            elif "sigmoid" in name.lower():
                name = "torch_sigmoid_"
            else:
                continue
            prev = out.get(name, {"calls": 0, "total_ms": 0.0})
            calls, total = prev["calls"] + int(row["Calls"]), prev["total_ms"] + float(row["TotalDurationNs"]) / 1e6
            out[name] = {"calls": calls, "total_ms": total, "average_us": total * 1e3 / calls}
    return out


def build(a):
    """the four models and the assembler, on the device"""
    torch.manual_seed(1234)
    with torch.device(DEV):
        nets = {"mf": zoo.MatrixFactorization(a.users, a.items, MF_RANK).eval(),
                "ffm": zoo.FFM(43, FFM_RANK, num_users=a.users, num_items=a.items).eval(),
                "lr": zoo.LogisticRegression(a.users, a.items, 43).eval(),
                "widedeep": zoo.WideDeep(a.users, a.items, WD_HIDDEN, WD_EMBED).eval()}
    users = synth.feature_batch(a.users, gen=synth.generator(11))[:, 2:26]
    items = synth.feature_batch(a.items, gen=synth.generator(12))[:, 26:45]
    return nets, FeatureAssembler(users.to(DEV), items.to(DEV))


def mf_before(net, rows):
    """leg (b): the score matrix of the first ``rows`` users as ``recommendation()`` makes it, then the sigmoid"""
    with torch.no_grad():
        return ops.linear_fwd(net.user_embeddings.weight[:rows], net.item_embeddings.weight, None).sigmoid_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263, help="drawn pairs of the observed set (distinct ones are fewer)")
    ap.add_argument("--rows", type=int, default=4096, help="users of the timed slice")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="calls per window of a short leg")
    ap.add_argument("--only-kernels", action="store_true", help="a few calls of every grid leg, (b) and (d): the profiler's run")
    ap.add_argument("--recommend", action="store_true", help="also time recommend(n=20) for every user (MF, Wide & Deep)")
    ap.add_argument("--stats-csv", help="rocprofv3 --stats kernel CSV of an --only-kernels run, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lowrank_grid_bench.py needs the GPU: there is nothing to measure without one")
    nets, asm = build(a)
    rows, pairs = a.rows, a.rows * a.items
    score_bytes = 4 * pairs
    grid = {"mf": nets["mf"].score_rows}
    forward = {}
    for name in ("ffm", "lr", "widedeep"):
        scorer = nets[name].catalogue_scorer(asm)
        assert scorer.path == "grid", name
        grid[name], forward[name] = scorer, CatalogueScorer(nets[name], asm)
    floor = torch.empty((rows, a.items), dtype=torch.float32, device=DEV)
    if a.only_kernels:
        for _ in range(5):
            for scorer in grid.values():
                scorer(0, rows)
            mf_before(nets["mf"], rows)
            floor.fill_(0.5)
        torch.cuda.synchronize()
        return
    res = {"metric": "lowrank_grid_scores_ml20m_tables", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "users": a.users, "items": a.items, "slice_rows": rows, "slice_pairs": pairs, "slice_score_bytes": score_bytes,
           "rounds": a.rounds, "calls_per_window": a.calls, "forward_pairs_per_call": 1 << 18,
           "shapes": {"mf": MF_RANK, "ffm": FFM_RANK, "widedeep": [WD_EMBED, WD_HIDDEN]}}
    # the legs score the same function (and every shape is warm before it is timed)
    worst = {"mf": float((grid["mf"](0, rows) - mf_before(nets["mf"], rows)).abs().max())}
    for name, scorer in forward.items():
        worst[name] = float((grid[name](0, rows) - scorer(0, rows)).abs().max())
    assert max(worst.values()) <= 1e-5, worst
    res["max_abs_difference_between_legs"] = worst
    floor.fill_(0.5)
    t = {"mf_grid": [], "mf_before": [], "store_floor": []}
    t.update({f"{name}_{leg}": [] for name in forward for leg in ("grid", "forward", "table_rows")})
    for _ in range(a.rounds):
        t["mf_grid"].append(timed(lambda: grid["mf"](0, rows), a.calls))
        t["mf_before"].append(timed(lambda: mf_before(nets["mf"], rows), a.calls))
        t["store_floor"].append(timed(lambda: floor.fill_(0.5), a.calls))
        for name in forward:
            calls = a.calls if name != "widedeep" else max(1, a.calls // 10)
            t[f"{name}_grid"].append(timed(lambda: grid[name](0, rows), calls))
            t[f"{name}_forward"].append(timed(lambda: forward[name](0, rows)))
            with torch.no_grad():
                t[f"{name}_table_rows"].append(timed(grid[name]._shared, max(1, a.calls // 10)))
    med = {k: statistics.median(v) for k, v in t.items()}
    res["legs"] = {k: dict(stats(v), pairs_per_s=pairs / med[k]) for k, v in t.items() if not k.endswith("table_rows")}
    for name in forward:
        res["legs"][f"{name}_grid"]["table_rows"] = dict(stats(t[f"{name}_table_rows"]),
                                                         share_of_grid_leg=med[f"{name}_table_rows"] / med[f"{name}_grid"])
        res["legs"][f"{name}_grid"]["over_forward_pairs_per_s"] = med[f"{name}_forward"] / med[f"{name}_grid"]
    res["legs"]["mf_grid"]["over_before_pairs_per_s"] = med["mf_before"] / med["mf_grid"]
    res["legs"]["store_floor"]["bytes_per_s"] = score_bytes / med["store_floor"]
    res["legs"]["mf_grid"]["score_bytes_per_s"] = score_bytes / med["mf_grid"]
    res["legs"]["mf_grid"]["share_of_store_floor"] = med["store_floor"] / med["mf_grid"]
    if a.recommend:
        observed = observed_set(a)
        res["recommend_all_users_n20"] = {"observed_pairs": len(observed), "pairs_scored": a.users * a.items}
        for name, scorer in (("mf", nets["mf"]), ("widedeep", grid["widedeep"])):
            scorer.recommend(users=list(range(64)), n=20, exclude=observed)
            wall = timed(lambda: scorer.recommend(n=20, exclude=observed))
            res["recommend_all_users_n20"][name] = {"wall_s": wall, "pairs_per_s": a.users * a.items / wall}
    if a.stats_csv:
        k = kernel_times(a.stats_csv)
        res["kernels_rocprofv3"] = k
        for name, v in k.items():
            if name.startswith("lowrank_grid_scores_kernel"):
                rank = 16 * int(name.split("<")[1].split(">")[0])
                sec = v["average_us"] * 1e-6
                entry = {"rank": rank, "average_us": v["average_us"], "pairs_per_s": pairs / sec,
                         "score_bytes_per_s": score_bytes / sec, "share_of_plain_store_peak": score_bytes / sec / STORE_PEAK,
                         "mfma_tflops": 2 * rank * pairs / sec / 1e12,
                         "share_of_fp32_mfma_peak": 2 * rank * pairs / sec / F32_MFMA_PEAK}
                entry["share_of_store_floor_window"] = med["store_floor"] / sec
                res.setdefault("grid_kernels", {})[name] = entry
            elif name.startswith("deepfm_grid_scores_kernel"):
                sec = v["average_us"] * 1e-6
                res.setdefault("grid_kernels", {})[name] = {
                    "average_us": v["average_us"], "pairs_per_s": pairs / sec,
                    "share_of_fp32_mfma_peak": 2 * 256 * 128 * pairs / sec / F32_MFMA_PEAK}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
