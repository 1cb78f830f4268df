#!/usr/bin/env python3
"""NeuralCF over the user x item grid at ml-20m table sizes (138 493 users x 26 744 items, NeuralCF 64 /
[128, 64, 32, 16, 8]); prints one JSON line.

Two ways to score a slice of ``--rows`` users against every item (4096 x 26 744 = 1.1e8 pairs):

  (a) grid     ``model.score_rows(0, rows)``: two projections over the table rows, the head fold, ``ctr_ncf_grid_scores``;
  (b) forward  what the model offered before: ``model(user_ids, item_ids)`` under ``no_grad`` over the slice's pairs,
               ``--chunk`` pairs per call, the int64 ids of the slice generated OUTSIDE the timed window.

The two legs alternate inside every round, each timed by a host clock around calls that end in a device synchronise;
the result quotes the median and the spread over ``--rounds`` rounds, pairs per second for both and their ratio.  It
also reports the wall time of ``recommend(n=20)`` for EVERY user with the observed set of dev/cf_bench.py left out
(138 493 x 26 744 = 3.7e9 pairs, which (b) cannot hold: 59 GB of ids).  The kernel's own time, and with it its share of
the 155 TF fp32 matrix-core rate, comes from a separate run under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_ncf_grid -- python dev/ncf_grid_bench.py --only-kernels
    python dev/ncf_grid_bench.py --stats-csv out/prof_ncf_grid/<...>_kernel_stats.csv --out profiles/ncf_grid_bench.json
"""
import argparse
import statistics
import sys

import torch

from _bench import DEV, F32_MFMA_PEAK, emit, need_gpu, observed_set, stats, timed  # first: it puts the repository root on sys.path
from _bench import library_kernel_rows as kernel_times
from deeplearningrecommendationsystem_amd import model as zoo

TOWER_FLOP_PER_PAIR = 2 * (64 * 32 + 32 * 16 + 16 * 8)      # 5376: the three layers the kernel runs per pair


def grid_kernel(pairs, kernels):
    """the ``grid_kernel`` entry from ``kernels_rocprofv3``; None where the grid kernel is not in it"""
    entry = None
    for name, v in kernels.items():
        if "ncf_grid_scores_kernel" in name:
            flops = TOWER_FLOP_PER_PAIR * pairs / (v["average_us"] * 1e-6)
            entry = {"average_us": v["average_us"], "tower_tflops": flops / 1e12,
                     "share_of_fp32_mfma_peak": flops / F32_MFMA_PEAK, "pairs_per_s": pairs / (v["average_us"] * 1e-6)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263, help="drawn pairs of the observed set (distinct ones are fewer)")
    ap.add_argument("--rows", type=int, default=4096, help="users of the timed slice")
    ap.add_argument("--chunk", type=int, default=1 << 20, help="pairs per forward call of leg (b)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only-kernels", action="store_true", help="a few calls of each leg alone: the profiler's run")
    ap.add_argument("--skip-recommend", action="store_true")
    ap.add_argument("--stats-csv", help="rocprofv3 --stats kernel CSV of an --only-kernels run, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    need_gpu("ncf_grid_bench.py")
    torch.manual_seed(1234)
    with torch.device(DEV):
        net = zoo.NeuralCF(a.users, a.items, 64, [128, 64, 32, 16, 8]).eval()
    rows, ni = a.rows, a.items
    pairs = rows * ni
    users = torch.arange(rows, device=DEV).repeat_interleave(ni)
    items = torch.arange(ni, device=DEV).repeat(rows)
    scores_b = torch.empty(pairs, dtype=torch.float32, device=DEV)

    def grid():
        return net.score_rows(0, rows)

    def forward():
        with torch.no_grad():
            for lo in range(0, pairs, a.chunk):
                scores_b[lo:lo + a.chunk] = net(users[lo:lo + a.chunk], items[lo:lo + a.chunk]).view(-1)

    if a.only_kernels:
        for _ in range(5):
            grid()
            forward()
        torch.cuda.synchronize()
        return
    got = grid()
    forward()
    worst = float((got.view(-1) - scores_b).abs().max())
    assert worst <= 1e-5, worst                                      # the two legs score the same function
    res = {"metric": "neuralcf_grid_scores_ml20m_tables", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "users": a.users, "items": a.items, "slice_rows": rows, "slice_pairs": pairs, "rounds": a.rounds,
           "forward_chunk_pairs": a.chunk, "max_abs_difference_between_legs": worst,
           "bytes": {"scores_written": 4 * pairs, "ids_read_by_forward": 16 * pairs}}
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed(grid))
        tb.append(timed(forward))
    ma, mb = statistics.median(ta), statistics.median(tb)
    res["grid"] = dict(stats(ta), pairs_per_s=pairs / ma)
    res["forward"] = dict(stats(tb), pairs_per_s=pairs / mb)
    res["grid_over_forward_pairs_per_s"] = mb / ma
    del users, items, scores_b, got
    if not a.skip_recommend:
        observed = observed_set(a)
        net.recommend(users=list(range(64)), n=20, exclude=observed)
        t = timed(lambda: net.recommend(n=20, exclude=observed))
        res["recommend_all_users_n20"] = {"wall_s": t, "observed_pairs": len(observed), "pairs_scored": a.users * ni,
                                          "pairs_per_s": a.users * ni / t}
    if a.stats_csv:
        res["kernels_rocprofv3"] = kernel_times(a.stats_csv)
        entry = grid_kernel(pairs, res["kernels_rocprofv3"])
        if entry:
            res["grid_kernel"] = entry
    emit(res, a.out)


if __name__ == "__main__":
    main()
