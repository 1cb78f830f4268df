#!/usr/bin/env python3
"""DIN over the history x item grid at the ml-20m item count (26 744 items, DIN at E = 64); prints one JSON line.

Two ways to score a slice of history rows against every item, at L = 10 (``--rows`` rows) and at L = 100
(``--rows-long`` rows):

  (a) grid     ``model.score_histories(hist)``: the split first attention layer on the table rows, ``ctr_din_grid_pool``,
               the fc stack per chunk of pairs;
  (b) forward  what the model offered before (``SequenceModel._rank_histories``): ``model(hist_ids, item_ids)`` under
               ``no_grad`` over the slice's pairs, 2^22 history positions per call, the int64 ids of the slice generated
               OUTSIDE the timed window.

The two legs alternate inside every round, each timed by a host clock around calls that end in a device synchronise;
the result quotes the median and the spread over ``--rounds`` rounds, pairs per second for both and their ratio.  The
kernels' own times -- the new kernel's share of the 155 TF fp32 matrix-core rate on its L * 2 * 128 * 64 flop per pair,
and how leg (a) splits between it and the fc stage -- come from a separate run of leg (a) alone under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_din_grid -- python dev/din_grid_bench.py --only-kernels
    python dev/din_grid_bench.py --stats-csv out/prof_din_grid/<...>_kernel_stats.csv --out profiles/din_grid_bench.json
"""
from _grid_bench import HistorySpec, history_bench  # first: it puts the repository root on sys.path
from deeplearningrecommendationsystem_amd import model as zoo

LAYER_FLOP_PER_POSITION = 2 * 128 * 64                       # the 128 -> 64 layer the kernel runs per (pair, position)

SPEC = HistorySpec(script="din_grid_bench.py", metric="din_grid_scores_ml20m_items", model=lambda items: zoo.DIN(items, 64),
                   embed=64, flop_per_position=LAYER_FLOP_PER_POSITION, kernel="din_grid_pool_kernel",
                   rate_key="layer_tflops", profile_length=False)

if __name__ == "__main__":
    history_bench(SPEC)
