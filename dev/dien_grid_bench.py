#!/usr/bin/env python3
"""DIEN over the history x item grid at the ml-20m item count (26 744 items, DIEN at E = 16); prints one JSON line.

Two ways to score a slice of history rows against every item, at L = 10 (``--rows`` rows) and at L = 100
(``--rows-long`` rows):

  (a) grid     ``model.score_histories(hist)``: the split first attention layer and the GRU's input projection on the
               table rows, ``ctr_dien_grid_hidden``, the fc stack per chunk of pairs;
  (b) forward  what the model offered before (``SequenceModel._rank_histories``): ``model(hist_ids, item_ids)`` under
               ``no_grad`` over the slice's pairs, 2^22 history positions per call, the int64 ids of the slice generated
               OUTSIDE the timed window.

The two legs alternate inside every round, each timed by a host clock around calls that end in a device synchronise;
the result quotes the median and the spread over ``--rounds`` rounds, pairs per second for both and their ratio.  The
kernels' own times -- the new kernel's share of the 155 TF fp32 matrix-core rate on its L * (2 * 64 * 32 + 2 * 16 * 48)
flop per pair, and how leg (a) splits between it, the fc stage and the table broadcast -- come from a separate run of
leg (a) alone under the profiler, at ``--profile-length`` 10 or 100:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_dien_grid -- python dev/dien_grid_bench.py --only-kernels
    python dev/dien_grid_bench.py --stats-csv out/prof_dien_grid/<...>_kernel_stats.csv --out profiles/dien_grid_bench.json
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

DEV = "cuda:0"
F32_MFMA_PEAK = 155e12
FLOP_PER_POSITION = 2 * 64 * 32 + 2 * 16 * 48                # the 64 -> 32 layer and the recurrent product per (pair, position)
MAX_POSITIONS = 1 << 22                                      # per forward call of leg (b): _rank_histories' bound
PROFILED_CALLS = 5                                           # score_histories calls of an --only-kernels run


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def kernel_times(path):
    """every kernel of an --only-kernels run, the library's by their short names"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "(anonymous namespace)::" in name and "at::native" not in name:
                name = name.split("(anonymous namespace)::")[1].split("(")[0].split("<")[0]
            else:
                name = name.split("(")[0][:80]
            e = out.setdefault(name, {"calls": 0, "total_ms": 0.0})
            e["calls"] += int(row["Calls"])
            e["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    return out


def legs(net, rows, length, ni):
    hist = torch.randint(0, ni, (rows, length), device=DEV, generator=torch.Generator(DEV).manual_seed(length))
    pairs = rows * ni
    hist_ids = hist.repeat_interleave(ni, 0)
    item_ids = torch.arange(ni, device=DEV).repeat(rows)
    scores_b = torch.empty(pairs, dtype=torch.float32, device=DEV)
    chunk = max(1, MAX_POSITIONS // length)

    def grid():
        return net.score_histories(hist)

    def forward():
        with torch.no_grad():
            for lo in range(0, pairs, chunk):
                scores_b[lo:lo + chunk] = net(hist_ids[lo:lo + chunk], item_ids[lo:lo + chunk]).view(-1)

    return hist, pairs, chunk, scores_b, grid, forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--rows", type=int, default=64, help="history rows of the timed slice at L = 10")
    ap.add_argument("--rows-long", type=int, default=8, help="history rows of the timed slice at L = 100")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only-kernels", action="store_true", help="five calls of leg (a) alone: the profiler's run")
    ap.add_argument("--profile-length", type=int, default=10, choices=(10, 100),
                    help="history length of the --only-kernels run and of the --stats-csv it produced")
    ap.add_argument("--stats-csv", help="rocprofv3 --stats kernel CSV of an --only-kernels run, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dien_grid_bench.py needs the GPU: there is nothing to measure without one")
    torch.manual_seed(1234)
    with torch.device(DEV):
        net = zoo.DIEN(a.items, 16).eval()
    ni = a.items
    profiled_rows = a.rows if a.profile_length == 10 else a.rows_long
    if a.only_kernels:
        grid = legs(net, profiled_rows, a.profile_length, ni)[4]
        for _ in range(PROFILED_CALLS):
            grid()
        torch.cuda.synchronize()
        return
    res = {"metric": "dien_grid_scores_ml20m_items", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "items": ni, "embed": 16, "rounds": a.rounds, "forward_positions_per_call": MAX_POSITIONS}
    for length, rows in ((10, a.rows), (100, a.rows_long)):
        hist, pairs, chunk, scores_b, grid, forward = legs(net, rows, length, ni)
        got = grid()
        forward()
        worst = float((got.view(-1) - scores_b).abs().max())
        assert worst <= 1e-5, worst                                  # the two legs score the same function
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(timed(grid))
            tb.append(timed(forward))
        ma, mb = statistics.median(ta), statistics.median(tb)
        res[f"L{length}"] = {"slice_rows": rows, "slice_pairs": pairs, "forward_chunk_pairs": chunk,
                             "max_abs_difference_between_legs": worst,
                             "bytes": {"scores_written": 4 * pairs, "ids_read_by_forward": 8 * (length + 1) * pairs},
                             "grid": dict(stats(ta), pairs_per_s=pairs / ma),
                             "forward": dict(stats(tb), pairs_per_s=pairs / mb),
                             "grid_over_forward_pairs_per_s": mb / ma}
        del hist, scores_b, got, grid, forward
    if a.stats_csv:
        k = kernel_times(a.stats_csv)
        tag = f"L{a.profile_length}"
        res[f"kernels_rocprofv3_{tag}_grid_leg"] = k
        total = sum(v["total_ms"] for v in k.values())
        hidden = k.get("dien_grid_hidden_kernel")
        if hidden:
            pairs = profiled_rows * ni
            flops = FLOP_PER_POSITION * a.profile_length * pairs * PROFILED_CALLS / (hidden["total_ms"] * 1e-3)
            res[f"grid_kernel_{tag}"] = {"launches": hidden["calls"], "total_ms": hidden["total_ms"],
                                         "tflops": flops / 1e12, "share_of_fp32_mfma_peak": flops / F32_MFMA_PEAK,
                                         "share_of_leg_kernel_time": hidden["total_ms"] / total,
                                         "rest_of_leg_share": 1.0 - hidden["total_ms"] / total}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
