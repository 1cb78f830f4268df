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
from _grid_bench import HistorySpec, history_bench  # first: it puts the repository root on sys.path
from deeplearningrecommendationsystem_amd import model as zoo

FLOP_PER_POSITION = 2 * 64 * 32 + 2 * 16 * 48                # the 64 -> 32 layer and the recurrent product per (pair, position)

SPEC = HistorySpec(script="dien_grid_bench.py", metric="dien_grid_scores_ml20m_items", model=lambda items: zoo.DIEN(items, 16),
                   embed=16, flop_per_position=FLOP_PER_POSITION, kernel="dien_grid_hidden_kernel",
                   rate_key="tflops", profile_length=True)

if __name__ == "__main__":
    history_bench(SPEC)
