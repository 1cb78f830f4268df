"""GPU: each of the seven dev/*_grid_bench.py scripts runs end to end, in a process of its own, at a shape of a few
seconds: 520 items (no multiple of the kernels' 128-item tile), 300 users (more than the 64 the recommend warm-up ranks),
two rounds.  The run ends with status 0 and one JSON line that carries the script's metric, and every pair of legs agrees
to the 1e-5 the scripts themselves demand.  What the readers and folds make of a profiler CSV is
tests/test_dev_bench_cpu.py's."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ["--users", "300", "--items", "520", "--pairs", "4000", "--rows", "64", "--rounds", "2"]
HISTORIES = ["--items", "520", "--rows", "4", "--rows-long", "2", "--rounds", "2"]
SCRIPTS = {
    "deepfm": ("deepfm_grid_scores_ml20m_tables", TABLES + ["--embed", "16"]),
    "pnn": ("pnn_grid_scores_ml20m_tables", TABLES + ["--embed", "16", "--recommend"]),
    "afm": ("afm_grid_scores_ml20m_tables", TABLES + ["--embed", "16", "--recommend"]),
    "ncf": ("neuralcf_grid_scores_ml20m_tables", TABLES + ["--chunk", "8192"]),
    "lowrank": ("lowrank_grid_scores_ml20m_tables", TABLES + ["--calls", "3", "--recommend"]),
    "din": ("din_grid_scores_ml20m_items", HISTORIES),
    "dien": ("dien_grid_scores_ml20m_items", HISTORIES),
}


def _leg_differences(node):
    """every figure recorded under a ``max_abs_difference_between_legs`` key, at any depth (the low-rank script keeps one a model)"""
    if isinstance(node, list):
        return [x for v in node for x in _leg_differences(v)]
    if not isinstance(node, dict):
        return []
    found = []
    for key, v in node.items():
        if key == "max_abs_difference_between_legs":
            found += list(v.values()) if isinstance(v, dict) else [v]
        else:
            found += _leg_differences(v)
    return found


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_script_runs(name):
    metric, args = SCRIPTS[name]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "dev", f"{name}_grid_bench.py"), *args],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["metric"] == metric
    worst = _leg_differences(res)
    assert worst and all(w <= 1e-5 for w in worst), worst
