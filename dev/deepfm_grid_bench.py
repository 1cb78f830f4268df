#!/usr/bin/env python3
"""DeepFM over the user x item grid at ml-20m table sizes (138 493 users x 26 744 items, hidden_units
[512, 256, 128, 1]) at E = 16 (the bench shape) and E = 128 (the reference script's shape); prints one JSON line.

Two ways to score a slice of ``--rows`` users against every item (4096 x 26 744 = 1.1e8 pairs), on one model:

  (a) grid     ``scorer.score_rows(0, rows)``: the user-side and item-side table rows (ctr_embed_fwd, four
               ctr_linear_fwd, a few torch expressions), then ``ctr_deepfm_grid_scores``;
  (b) forward  the chunked forward path every feature model gets: ``assembler.feature`` and ``model.forward`` under
               ``no_grad``, 2^18 pairs a call (``FeatureModel.catalogue_scorer``'s scorer on the same model).

The two legs alternate inside every round, each timed by a host clock around calls that end in a device synchronise;
the result quotes the median and the spread over ``--rounds`` rounds, pairs per second for both and their ratio, and
the time of the table rows alone (``scorer._shared()``), hence their share of leg (a).  It also reports the wall time of
``recommend(n=20)`` for EVERY user with the observed set of dev/cf_bench.py left out.  The kernel's own time, and with
it its share of the 155 TF fp32 matrix-core rate, comes from a separate run under the profiler, of leg (a) alone:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_deepfm_grid -- python dev/deepfm_grid_bench.py --only-kernels --embed 16
    python dev/deepfm_grid_bench.py --stats-csv 16=out/prof_deepfm_grid/<...>_kernel_stats.csv --out profiles/deepfm_grid_bench.json
"""
import torch

from _grid_bench import DEV, SixFieldSpec, assembler, six_field_bench  # first: it puts the repository root on sys.path
from deeplearningrecommendationsystem_amd import model as zoo

HIDDEN = [512, 256, 128, 1]
NCF_GRID_SHARE = 0.58                            # what ncf_grid_scores_kernel reaches (README, NeuralCF over the grid)


def flop_per_pair(embed):
    return 2 * 256 * 128 + 256 + 2 * 128 + 2 * embed      # the 256 -> 128 layer, the relu'd sum, the w3 and FM dots


def build(a, embed):
    torch.manual_seed(1234)
    with torch.device(DEV):
        net = zoo.DeepFM(a.users, a.items, HIDDEN, embed).eval()
    return net, assembler(a)


SPEC = SixFieldSpec(script="deepfm_grid_bench.py", metric="deepfm_grid_scores_ml20m_tables", build=build,
                    flop_per_pair=flop_per_pair, embed=[16, 128], kernel="deepfm_grid_scores_kernel",
                    recommend_flag="--skip-recommend", model_entries={"hidden_units": HIDDEN},
                    closing_entries={"ncf_grid_share_of_fp32_mfma_peak": NCF_GRID_SHARE})

if __name__ == "__main__":
    six_field_bench(SPEC)
