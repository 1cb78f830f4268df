"""What the dev/*_grid_bench.py scripts share: the timing method (a window, a spread), the observed set of the
recommend legs, the reader of a ``rocprofv3 --kernel-trace --stats`` kernel CSV and the output line.  A module, not a
script; importing it needs no GPU (tests/test_dev_bench_cpu.py reads the recorded CSVs of profiles/ with it).

A window is ``calls`` back-to-back calls between two device synchronises, timed by the host clock; a leg's figure is the
median of its windows, quoted with their minimum and maximum.  dev/_grid_bench.py holds the two frames built on this.
"""
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)                                     # the scripts import the package after this module
from deeplearningrecommendationsystem_amd.data import ObservedPairs  # noqa: E402

DEV = "cuda:0"
F32_MFMA_PEAK = 155e12
STORE_PEAK = 6.0e12          # plain stores, MI355X_MICROARCH.md


def need_gpu(script):
    if not torch.cuda.is_available():
        raise SystemExit(f"{script} needs the GPU: there is nothing to measure without one")


def timed(fn, calls=1):
    """seconds per call of ``calls`` back-to-back calls that end in one device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def observed_set(a):
    rng = np.random.default_rng(0)                                   # the observed set of dev/cf_bench.py
    pop = 1.0 / np.arange(1, a.items + 1)
    pop = pop[rng.permutation(a.items)]
    u = torch.from_numpy(rng.integers(0, a.users, a.pairs)).to(DEV)
    i = torch.from_numpy(rng.choice(a.items, size=a.pairs, p=pop / pop.sum())).to(DEV)
    return ObservedPairs(u, i, a.users, a.items)


def emit(res, out):
    """the JSON line: printed, and written to ``out`` if that is given"""
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------- the profiler's kernel CSV, four readers
def library_name(name, template_args=False):
    """a library kernel's short name out of ``... (anonymous namespace)::name<...>(...)``; None for any other kernel"""
    if "(anonymous namespace)::" not in name or "at::native" in name:
        return None
    name = name.split("(anonymous namespace)::")[1].split("(")[0]
    return name if template_args else name.split("<")[0]


def _summed(path, short, average):
    """calls and total_ms per ``short(Name)`` over the rows of the CSV; rows that ``short`` answers with None are left out"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = short(row["Name"])
            if name is None:
                continue
            prev = out.get(name, {"calls": 0, "total_ms": 0.0})
            calls, total = prev["calls"] + int(row["Calls"]), prev["total_ms"] + float(row["TotalDurationNs"]) / 1e6
            out[name] = {"calls": calls, "total_ms": total}
            if average:
                out[name]["average_us"] = total * 1e3 / calls
    return out


def library_kernel_sums(path):
    """the library's kernels of an --only-kernels run, summed per short name (DeepFM, PNN, AFM)"""
    return _summed(path, library_name, average=True)


def library_kernel_rows(path):
    """the library's kernels of an --only-kernels run with the row's own average, minimum and maximum (NeuralCF)"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = library_name(row["Name"])
            if name is not None:
                out[name] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6,
                             "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                             "max_us": float(row["MaxNs"]) / 1e3}
    return out


def every_kernel_totals(path):
    """every kernel of an --only-kernels run, the library's by their short names (DIN, DIEN)"""
    def short(name):
        lib = library_name(name)
        return name.split("(")[0][:80] if lib is None else lib
    return _summed(path, short, average=False)


def lowrank_kernel_sums(path):
    """the kernels of an --only-kernels run: the library's by name (template arguments kept), torch's fill and sigmoid"""
    def short(name):
        lib = library_name(name, template_args=True)
        if lib is not None:
            return lib
        return "torch_fill" if "FillFunctor" in name else "torch_sigmoid_" if "sigmoid" in name.lower() else None
    return _summed(path, short, average=True)
