#!/usr/bin/env python3
"""PNN (inner mode) over the user x item grid at ml-20m table sizes (138 493 users x 26 744 items, hidden_units
[256, 128, 64, 32]) at E = 16 (the bench shape) and E = 256 (the reference script's shape); prints one JSON line.

Two ways to score a slice of ``--rows`` users against every item (4096 x 26 744 = 1.1e8 pairs), on one model:

  (a) grid     ``scorer.score_rows(0, rows)``: the user-side and item-side table rows (ctr_embed_fwd, ctr_allpairs_fwd,
               three ctr_linear_fwd a pass, G), then ``ctr_pnn_grid_scores``;
  (b) forward  the chunked forward path every feature model gets: ``assembler.feature`` and ``model.forward`` under
               ``no_grad``, 2^18 pairs a call (``FeatureModel.catalogue_scorer``'s scorer on the same model).

The two legs alternate inside every round, each timed by a host clock around calls that end in a device synchronise;
the result quotes the median and the spread over ``--rounds`` rounds, pairs per second for both and their ratio, and
the time of the table rows alone (``scorer._shared()``), hence their share of leg (a).  With ``--recommend`` it also
reports the wall time of ``recommend(n=20)`` for EVERY user with the observed set of dev/cf_bench.py left out.  The
kernel's own time, and with it its share of the 155 TF fp32 matrix-core rate, comes from a separate run under the
profiler, of leg (a) alone:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/prof_pnn_grid -- python dev/pnn_grid_bench.py --only-kernels --embed 16
    python dev/pnn_grid_bench.py --stats-csv 16=out/prof_pnn_grid/<...>_kernel_stats.csv --out profiles/pnn_grid_bench.json
"""
import torch

from _grid_bench import DEV, SixFieldSpec, assembler, six_field_bench  # first: it puts the repository root on sys.path
from deeplearningrecommendationsystem_amd import model as zoo

HIDDEN = [256, 128, 64, 32]


def flop_per_pair(embed):
    return 2 * (8 * embed + 128 * 8 + 128 * 64 + 64 * 32 + 32)      # the dots, G d, the two layers, the output dot


def build(a, embed):
    torch.manual_seed(1234)
    with torch.device(DEV):
        net = zoo.PNN(embed, HIDDEN, num_users=a.users, num_items=a.items).eval()
    return net, assembler(a)


SPEC = SixFieldSpec(script="pnn_grid_bench.py", metric="pnn_grid_scores_ml20m_tables", build=build,
                    flop_per_pair=flop_per_pair, embed=[16, 256], kernel="pnn_grid_scores_kernel",
                    recommend_flag="--recommend", model_entries={"hidden_units": HIDDEN})

if __name__ == "__main__":
    six_field_bench(SPEC)
