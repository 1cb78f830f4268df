"""The two frames of the grid-scorer benchmarks: ``six_field_bench`` (dev/deepfm_grid_bench.py, pnn_grid_bench.py,
afm_grid_bench.py) and ``history_bench`` (dev/din_grid_bench.py, dien_grid_bench.py).  A script keeps its docstring, its
constants and a spec; the frame owns the argument parser, the --only-kernels run, the timed legs, the recommend leg,
the fold of the profiler's CSV and the output.  Windows, medians and the CSV readers are dev/_bench.py's.

In both frames the legs alternate inside every round, each window timed by a host clock around calls that end in a device
synchronise.  The folds (``six_field_grid_kernel``, ``history_grid_kernel``) are pure functions of the reader's dictionary
and the shape: tests/test_dev_bench_cpu.py recomputes the recorded entries of profiles/ with them, without a GPU.
"""
import argparse
import statistics
import sys
from dataclasses import dataclass, field
from typing import Callable

import torch

from _bench import DEV, F32_MFMA_PEAK, emit, every_kernel_totals, library_kernel_sums, need_gpu, observed_set, stats, timed
from deeplearningrecommendationsystem_amd import synth
from deeplearningrecommendationsystem_amd.data import FeatureAssembler
from deeplearningrecommendationsystem_amd.model._base import CatalogueScorer

MAX_POSITIONS = 1 << 22                                      # per forward call of a history leg (b): _rank_histories' bound
PROFILED_CALLS = 5                                           # calls of leg (a) in an --only-kernels run


# ---------------------------------------------------------------------------------- six-field models: user x item grid
@dataclass
class SixFieldSpec:
    script: str                                  # the file's name, for the no-GPU sentence
    metric: str
    build: Callable                              # (a, embed) -> (net, assembler)
    flop_per_pair: Callable                      # embed -> flop the kernel runs per pair
    embed: list                                  # default of --embed
    kernel: str                                  # the grid kernel's short name in the profiler's CSV
    recommend_flag: str                          # "--skip-recommend" (the leg runs by default) or "--recommend"
    model_entries: dict = field(default_factory=dict)        # of the result, after "items"
    closing_entries: dict = field(default_factory=dict)      # of the result, in front of "shapes"
    shape_entries: Callable = lambda embed: {}               # of a shape, after "flop_per_pair"
    rate: tuple = None                                       # (key, embed -> flop) of the kernel's rate figure
    kernel_times = staticmethod(library_kernel_sums)

    def __post_init__(self):
        self.rate = self.rate or ("tflops", self.flop_per_pair)


def assembler(a):
    """the synthetic user and item feature tables of every six-field benchmark, on the device"""
    users = synth.feature_batch(a.users, gen=synth.generator(11))[:, 2:26]
    items = synth.feature_batch(a.items, gen=synth.generator(12))[:, 26:45]
    return FeatureAssembler(users.to(DEV), items.to(DEV))


def six_field_grid_kernel(spec, embed, pairs, kernels):
    """a shape's ``grid_kernel`` entry from its ``kernels_rocprofv3``; None where the grid kernel is not in it"""
    entry = None
    key, flop = spec.rate
    for name, v in kernels.items():
        if spec.kernel in name:
            flops = flop(embed) * pairs / (v["average_us"] * 1e-6)
            entry = {"average_us": v["average_us"], key: flops / 1e12, "share_of_fp32_mfma_peak": flops / F32_MFMA_PEAK,
                     "pairs_per_s": pairs / (v["average_us"] * 1e-6)}
    return entry


def _six_field_measure(spec, a, embed, observed):
    net, asm = spec.build(a, embed)
    grid_scorer, forward_scorer = net.catalogue_scorer(asm), CatalogueScorer(net, asm)
    assert grid_scorer.path == "grid" and forward_scorer.path == "forward"
    rows, pairs = a.rows, a.rows * a.items
    got = grid_scorer.score_rows(0, rows)
    want = forward_scorer.score_rows(0, rows)
    worst = float((got - want).abs().max())
    assert worst <= 1e-5, worst                                      # the two legs score the same function
    del got, want
    res = {"embedding_dim": embed, "flop_per_pair": spec.flop_per_pair(embed), **spec.shape_entries(embed),
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


def six_field_bench(spec):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263, help="drawn pairs of the observed set (distinct ones are fewer)")
    ap.add_argument("--rows", type=int, default=4096, help="users of the timed slice")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--embed", type=int, nargs="+", default=spec.embed)
    ap.add_argument("--only-kernels", action="store_true", help="a few calls of leg (a) alone: the profiler's run")
    if spec.recommend_flag == "--skip-recommend":
        ap.add_argument("--skip-recommend", action="store_true")
    else:
        ap.add_argument("--recommend", action="store_true", help="also time recommend(n=20) for every user")
    ap.add_argument("--stats-csv", action="append", default=[], metavar="E=PATH",
                    help="rocprofv3 --stats kernel CSV of an --only-kernels --embed E run, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    need_gpu(spec.script)
    if a.only_kernels:
        for embed in a.embed:
            net, asm = spec.build(a, embed)
            scorer = net.catalogue_scorer(asm)
            for _ in range(PROFILED_CALLS):
                scorer.score_rows(0, a.rows)
        torch.cuda.synchronize()
        return
    pairs = a.rows * a.items
    res = {"metric": spec.metric, "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "users": a.users, "items": a.items, **spec.model_entries, "slice_rows": a.rows, "slice_pairs": pairs,
           "rounds": a.rounds, "forward_pairs_per_call": 1 << 18, **spec.closing_entries, "shapes": []}
    recommend = not a.skip_recommend if spec.recommend_flag == "--skip-recommend" else a.recommend
    observed = observed_set(a) if recommend else None
    csvs = dict(s.split("=", 1) for s in a.stats_csv)
    for embed in a.embed:
        r = _six_field_measure(spec, a, embed, observed)
        if str(embed) in csvs:
            r["kernels_rocprofv3"] = spec.kernel_times(csvs[str(embed)])
            entry = six_field_grid_kernel(spec, embed, pairs, r["kernels_rocprofv3"])
            if entry:
                r["grid_kernel"] = entry
        res["shapes"].append(r)
    emit(res, a.out)


# ------------------------------------------------------------------------------- sequence models: history x item grid
@dataclass
class HistorySpec:
    script: str                                  # the file's name, for the no-GPU sentence
    metric: str
    model: Callable                              # items -> the model, built on the device
    embed: int
    flop_per_position: int                       # what the kernel runs per (pair, position)
    kernel: str                                  # the grid kernel's short name in the profiler's CSV
    rate_key: str                                # the key of the kernel's rate figure
    profile_length: bool                         # --profile-length exists; without it the profiled leg is L = 10
    kernel_times = staticmethod(every_kernel_totals)


def _history_legs(net, rows, length, ni):
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


def history_grid_kernel(spec, length, pairs, kernels):
    """the ``grid_kernel_L<length>`` entry from the profiled leg's kernels; None where the grid kernel is not among them"""
    total = sum(v["total_ms"] for v in kernels.values())
    own = kernels.get(spec.kernel)
    if not own:
        return None
    flops = spec.flop_per_position * length * pairs * PROFILED_CALLS / (own["total_ms"] * 1e-3)
    return {"launches": own["calls"], "total_ms": own["total_ms"],
            spec.rate_key: flops / 1e12, "share_of_fp32_mfma_peak": flops / F32_MFMA_PEAK,
            "share_of_leg_kernel_time": own["total_ms"] / total, "rest_of_leg_share": 1.0 - own["total_ms"] / total}


def history_bench(spec):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--rows", type=int, default=64, help="history rows of the timed slice at L = 10")
    ap.add_argument("--rows-long", type=int, default=8, help="history rows of the timed slice at L = 100")
    ap.add_argument("--rounds", type=int, default=7)
    if spec.profile_length:
        ap.add_argument("--only-kernels", action="store_true", help="five calls of leg (a) alone: the profiler's run")
        ap.add_argument("--profile-length", type=int, default=10, choices=(10, 100),
                        help="history length of the --only-kernels run and of the --stats-csv it produced")
    else:
        ap.add_argument("--only-kernels", action="store_true", help="five calls of leg (a) at L = 10 alone: the profiler's run")
    ap.add_argument("--stats-csv", help="rocprofv3 --stats kernel CSV of an --only-kernels run, merged into the result")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    need_gpu(spec.script)
    torch.manual_seed(1234)
    with torch.device(DEV):
        net = spec.model(a.items).eval()
    ni = a.items
    profiled_length = a.profile_length if spec.profile_length else 10
    profiled_rows = a.rows if profiled_length == 10 else a.rows_long
    if a.only_kernels:
        grid = _history_legs(net, profiled_rows, profiled_length, ni)[4]
        for _ in range(PROFILED_CALLS):
            grid()
        torch.cuda.synchronize()
        return
    res = {"metric": spec.metric, "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "items": ni, "embed": spec.embed, "rounds": a.rounds, "forward_positions_per_call": MAX_POSITIONS}
    for length, rows in ((10, a.rows), (100, a.rows_long)):
        hist, pairs, chunk, scores_b, grid, forward = _history_legs(net, rows, length, ni)
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
        k = spec.kernel_times(a.stats_csv)
        res[f"kernels_rocprofv3_L{profiled_length}_grid_leg"] = k
        entry = history_grid_kernel(spec, profiled_length, profiled_rows * ni, k)
        if entry:
            res[f"grid_kernel_L{profiled_length}"] = entry
    emit(res, a.out)
