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
import torch

from _grid_bench import DEV, SixFieldSpec, assembler, six_field_bench  # first: it puts the repository root on sys.path
from deeplearningrecommendationsystem_amd import model as zoo

ATTENTION = 64


def map_flop_per_pair(embed):
    return 2 * 8 * embed * ATTENTION                                 # the attention map of the eight cross products


def flop_per_pair(embed):
    # per cross product: the product itself, the map, bias + relu + the dot with h, the dot with o, the softmax merge
    return 8 * (embed + 2 * embed * ATTENTION + 4 * ATTENTION + 2 * embed + 8)


def build(a, embed):
    torch.manual_seed(1234)
    with torch.device(DEV):
        net = zoo.AFM(a.users, a.items, embed, ATTENTION).eval()
    return net, assembler(a)


SPEC = SixFieldSpec(script="afm_grid_bench.py", metric="afm_grid_scores_ml20m_tables", build=build,
                    flop_per_pair=flop_per_pair, embed=[16, 128], kernel="afm_grid_scores_kernel",
                    recommend_flag="--recommend", model_entries={"attention_dim": ATTENTION},
                    shape_entries=lambda embed: {"map_flop_per_pair": map_flop_per_pair(embed)},
                    rate=("map_tflops", map_flop_per_pair))

if __name__ == "__main__":
    six_field_bench(SPEC)
