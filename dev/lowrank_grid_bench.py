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
import statistics
import sys

import torch

from _bench import DEV, F32_MFMA_PEAK, STORE_PEAK, emit, need_gpu, observed_set, stats, timed  # first: it puts the repository root on sys.path
from _bench import lowrank_kernel_sums as kernel_times
from deeplearningrecommendationsystem_amd import model as zoo
from deeplearningrecommendationsystem_amd import ops, synth
from deeplearningrecommendationsystem_amd.data import FeatureAssembler
from deeplearningrecommendationsystem_amd.model._base import CatalogueScorer

MF_RANK, FFM_RANK, WD_EMBED, WD_HIDDEN = 64, 32, 128, [512, 256, 128, 1]


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


def grid_kernels(pairs, store_floor_s, kernels):
    """the ``grid_kernels`` entries from ``kernels_rocprofv3``; ``store_floor_s`` is the median window of leg (d), seconds a call"""
    out, score_bytes = {}, 4 * pairs
    for name, v in kernels.items():
        sec = v["average_us"] * 1e-6
        if name.startswith("lowrank_grid_scores_kernel"):
            rank = 16 * int(name.split("<")[1].split(">")[0])
            out[name] = {"rank": rank, "average_us": v["average_us"], "pairs_per_s": pairs / sec,
                         "score_bytes_per_s": score_bytes / sec, "share_of_plain_store_peak": score_bytes / sec / STORE_PEAK,
                         "mfma_tflops": 2 * rank * pairs / sec / 1e12,
                         "share_of_fp32_mfma_peak": 2 * rank * pairs / sec / F32_MFMA_PEAK,
                         "share_of_store_floor_window": store_floor_s / sec}
        elif name.startswith("deepfm_grid_scores_kernel"):
            out[name] = {"average_us": v["average_us"], "pairs_per_s": pairs / sec,
                         "share_of_fp32_mfma_peak": 2 * 256 * 128 * pairs / sec / F32_MFMA_PEAK}
    return out


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
    need_gpu("lowrank_grid_bench.py")
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
        res["kernels_rocprofv3"] = kernel_times(a.stats_csv)
        entries = grid_kernels(pairs, med["store_floor"], res["kernels_rocprofv3"])
        if entries:
            res["grid_kernels"] = entries
    emit(res, a.out)


if __name__ == "__main__":
    main()
