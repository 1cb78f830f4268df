"""CPU: the readers and folds of the seven dev/*_grid_bench.py scripts against what profiles/ recorded with them.  For each
of the ten profiler CSVs kept there the script's reader must give, with ``==``, the dictionary in the script's JSON, and
the fold of that dictionary must give the recorded ``grid_kernel*`` entry -- the same rates, shares and pairs per second,
recomputed from the recorded shape.  No tolerance: the recorded entries came out of these expressions."""
import importlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(ROOT, "profiles")
sys.path.insert(0, os.path.join(ROOT, "dev"))                # where the scripts find their own modules when they are run


def _script(name):
    return importlib.import_module(f"{name}_grid_bench")


def _recorded(name):
    with open(os.path.join(PROFILES, f"{name}_grid_bench.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name,embed", [("deepfm", 16), ("deepfm", 128), ("pnn", 16), ("pnn", 256), ("afm", 16), ("afm", 128)])
def test_six_field_reader_and_fold(name, embed):
    from _grid_bench import six_field_grid_kernel
    spec, rec = _script(name).SPEC, _recorded(name)
    shape = next(s for s in rec["shapes"] if s["embedding_dim"] == embed)
    kernels = spec.kernel_times(os.path.join(PROFILES, f"{name}_grid_bench_kernel_stats_E{embed}.csv"))
    assert kernels == shape["kernels_rocprofv3"]
    assert spec.flop_per_pair(embed) == shape["flop_per_pair"]
    assert spec.shape_entries(embed) == {k: shape[k] for k in ("map_flop_per_pair",) if k in shape}
    assert six_field_grid_kernel(spec, embed, rec["slice_pairs"], kernels) == shape["grid_kernel"]


@pytest.mark.parametrize("name,csv", [("din", "din_grid_bench_kernel_stats.csv"), ("dien", "dien_grid_bench_kernel_stats_L10.csv")])
def test_history_reader_and_fold(name, csv):
    from _grid_bench import history_grid_kernel
    spec, rec = _script(name).SPEC, _recorded(name)
    kernels = spec.kernel_times(os.path.join(PROFILES, csv))
    assert kernels == rec["kernels_rocprofv3_L10_grid_leg"]
    pairs = rec["L10"]["slice_rows"] * rec["items"]
    assert history_grid_kernel(spec, 10, pairs, kernels) == rec["grid_kernel_L10"]


def test_neuralcf_reader_and_fold():
    mod, rec = _script("ncf"), _recorded("ncf")
    kernels = mod.kernel_times(os.path.join(PROFILES, "ncf_grid_bench_kernel_stats.csv"))
    assert kernels == rec["kernels_rocprofv3"]
    assert mod.grid_kernel(rec["slice_pairs"], kernels) == rec["grid_kernel"]


def test_lowrank_reader_and_fold():
    mod, rec = _script("lowrank"), _recorded("lowrank")
    kernels = mod.kernel_times(os.path.join(PROFILES, "lowrank_grid_bench_kernel_stats.csv"))
    assert kernels == rec["kernels_rocprofv3"]
    store_floor_s = rec["legs"]["store_floor"]["median_ms"] / 1e3           # the fold's one input that is a measured time
    assert mod.grid_kernels(rec["slice_pairs"], store_floor_s, kernels) == rec["grid_kernels"]


def test_one_call_window_is_the_plain_clock_difference(monkeypatch):
    import _bench
    ticks = iter([10.0, 10.7])
    monkeypatch.setattr(_bench.torch.cuda, "synchronize", lambda: None)
    monkeypatch.setattr(_bench.time, "perf_counter", lambda: next(ticks))
    calls = []
    assert _bench.timed(lambda: calls.append(1)) == 10.7 - 10.0 and calls == [1]
    assert _bench.stats([0.003, 0.001, 0.002]) == {"median_ms": 0.002 * 1e3, "min_ms": 0.001 * 1e3, "max_ms": 0.003 * 1e3}
