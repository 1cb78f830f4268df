#!/usr/bin/env python3
"""The three arms of the ALS row solves at the ml-20m shape of dev/als_bench.py (138 493 users x 26 744 items, the
~14.8 M distinct synthetic pairs of its Zipf draw, one seeded integer value 1..5 per pair), k = 64 and k = 128,
hipEvent-timed after warm-up; prints one JSON line and writes it to ``profiles/als_weighted_bench_ml20m.json``
(``--out``).

  unit        ``ops.als_gram`` + ``ops.als_solve_rows``: the pairs as a set, one confidence 1 + alpha
  confidence  ``ops.als_gram`` + ``ops.als_solve_rows_weighted``: c = 1 + alpha v, w = (0, alpha), t = (1, alpha)
  explicit    ``ops.als_solve_rows_weighted`` alone: no Gram, w = (1, 0), t = (0, 1), reg times the list length

User and item half-sweeps of each.  Every leg is judged on its own against float64 (``numpy.linalg.solve`` of its
normal equations built from the fp32 inputs) on ``--sample`` rows spread over the launch order: the worst
``max|x - x64| / max|x64|`` and the worst residual ``max|A x - b| / (|A|_inf max|x| + max|b|)``, and the guard bits of
the launch.  The legs alternate in one process; each figure is the median of 7 windows of ``--reps`` half-sweeps.  No
threshold is attached.

``--parent-lib PATH``: a libctrhip.so built from the parent commit.  Its ``ctr_als_solve_rows`` is then timed on the
same operands in the same windows beside this build's (the solve launch alone, the Gram given), and the two outputs are
compared bitwise.

Kernel times are not taken here: run

    rocprofv3 --kernel-trace --stats -d <dir> -- python dev/als_weighted_bench.py --trace

in a run of its own (``--trace``: three half-sweeps per leg, nothing timed, nothing written).

    python dev/als_weighted_bench.py [--reps 1] [--parent-lib PATH] [--out profiles/als_weighted_bench_ml20m.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dev"))
from als_bench import ALPHA, DRAWS, ITEMS, KS, REG, USERS, WINDOWS, Side, window  # noqa: E402
from deeplearningrecommendationsystem_amd import _lib, ops  # noqa: E402
from deeplearningrecommendationsystem_amd.data import Interactions, ObservedPairs  # noqa: E402

ARMS = {      # name: (dense part, (w0, w1), (t0, t1), reg, reg_per_entry)
    "unit": (True, (ALPHA, 0.0), (1.0 + ALPHA, 0.0), REG, 0.0),          # as the float64 judge states it
    "confidence": (True, (0.0, ALPHA), (1.0, ALPHA), REG, 0.0),
    "explicit": (False, (1.0, 0.0), (0.0, 1.0), 0.0, REG),
}


def half(arm, side, values, fixed, flag):
    pairs = side.pairs
    if arm == "unit":
        return ops.als_solve_rows(fixed, ops.als_gram(fixed), pairs.indptr, pairs.indices, REG, ALPHA, rows=side.plan,
                                  err_flag=flag)
    dense, w, t, reg, per_entry = ARMS[arm]
    return ops.als_solve_rows_weighted(fixed, ops.als_gram(fixed) if dense else None, pairs.indptr, pairs.indices,
                                       values, w, t, reg, per_entry, rows=side.plan, err_flag=flag)


class Judge:
    """float64 solutions of ``sample`` rows of one (arm, side, table), made once on the host"""

    def __init__(self, arm, side, values, fixed, sample):
        dense, (w0, w1), (t0, t1), reg, per_entry = ARMS[arm]
        y = fixed.double().cpu().numpy()
        k = y.shape[1]
        gram = y.T @ y if dense else np.zeros((k, k))
        indptr, indices = side.pairs.indptr.cpu().numpy(), side.pairs.indices.cpu().numpy()
        vals = np.ones(indices.size) if arm == "unit" else values.double().cpu().numpy()
        plan = side.plan.cpu().numpy()
        self.at = np.unique(np.linspace(0, plan.size - 1, sample).astype(np.int64))     # first and last row included
        self.a, self.b, self.x = [], [], []
        for j in self.at:
            span = slice(indptr[plan[j]], indptr[plan[j] + 1])
            x, v = y[indices[span]], vals[span]
            a = gram + (x * (w0 + w1 * v)[:, None]).T @ x + (reg + per_entry * len(v)) * np.eye(k)
            b = (x * (t0 + t1 * v)[:, None]).sum(0)
            self.a.append(a)
            self.b.append(b)
            self.x.append(np.linalg.solve(a, b) if len(v) else np.zeros(k))

    def of(self, out, bits):
        got = out[torch.from_numpy(self.at).to(out.device)].double().cpu().numpy()
        diff = resid = 0.0
        zero_rows = 0
        for g, a, b, x in zip(got, self.a, self.b, self.x):
            scale = np.abs(x).max()
            if scale == 0.0:                                  # an empty list
                diff = max(diff, float(np.abs(g).max()))
                continue
            zero_rows += int(not g.any())
            diff = max(diff, float(np.abs(g - x).max() / scale))
            resid = max(resid, float(np.abs(a @ g - b).max() / (np.abs(a).sum(1).max() * np.abs(g).max()
                                                                 + np.abs(b).max())))
        return dict(rows=int(self.at.size), max_rel_diff_vs_float64=diff, max_scaled_residual=resid,
                    zeroed_rows=zero_rows, finite=bool(torch.isfinite(out).all()), err_flag_bits=bits)


def unit_solver(path):
    """``ctr_als_solve_rows`` of one build of the library, called through ctypes with nothing else on the host path, so
    that two builds are timed alike"""
    fn = ctypes.CDLL(path).ctr_als_solve_rows
    fn.restype, fn.argtypes = _lib.SIGNATURES["ctr_als_solve_rows"]

    def solve(side, fixed, gram, out):
        k = fixed.shape[1]
        _lib.check(fn(fixed.data_ptr(), fixed.shape[0], k, gram.data_ptr(), side.pairs.indptr.data_ptr(),
                      side.pairs.indices.data_ptr(), side.pairs.indptr.numel() - 1, side.plan.data_ptr(),
                      side.plan.numel(), REG, ALPHA, out.data_ptr(), k, None, _lib.stream_ptr()), "parent solve")
        return out
    return solve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1, help="half-sweeps per timed window")
    ap.add_argument("--sample", type=int, default=300, help="rows of each half-sweep judged against float64")
    ap.add_argument("--parent-lib", default=None, help="a libctrhip.so of the parent commit, for the unit solve A/B")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_weighted_bench_ml20m.json"))
    ap.add_argument("--trace", action="store_true", help="three untimed half-sweeps per leg, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("als_weighted_bench needs the GPU: nothing is measured without one")
    rng = np.random.default_rng(0)                            # the draw of dev/als_bench.py
    pop = 1.0 / np.arange(1, ITEMS + 1)
    pop = pop[rng.permutation(ITEMS)]
    u = torch.from_numpy(rng.integers(0, USERS, DRAWS)).cuda()
    i = torch.from_numpy(rng.choice(ITEMS, size=DRAWS, p=pop / pop.sum())).cuda()
    by_user = ObservedPairs(u, i, USERS, ITEMS)
    del u, i
    gen = torch.Generator(device="cuda").manual_seed(0)
    users = torch.repeat_interleave(torch.arange(USERS, device="cuda"), by_user.indptr.diff())
    vals = torch.randint(1, 6, (len(by_user),), device="cuda", generator=gen).float()
    inter = Interactions(users, by_user.indices.long(), vals, USERS, ITEMS, duplicates="error")
    assert torch.equal(inter.pairs.indices, by_user.indices) and torch.equal(inter.values, vals)
    del users, by_user
    sides = {"user": (Side(inter.pairs), inter.values)}
    t = inter.transpose()
    sides["item"] = (Side(t.pairs), t.values)
    pairs = len(inter)
    tables = {k: {"user": (torch.randn(ITEMS, k, device="cuda", generator=gen) * 0.1).contiguous(),     # the FIXED table
                  "item": (torch.randn(USERS, k, device="cuda", generator=gen) * 0.1).contiguous()} for k in KS}
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    legs = {}
    for k in KS:
        for name, (side, values) in sides.items():
            for arm in ARMS:
                legs[f"{arm}_{name}_k{k}"] = (lambda arm=arm, side=side, values=values, y=tables[k][name]:
                                              half(arm, side, values, y, flag))
    if a.trace:
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        return

    judged = {}
    for k in KS:
        for name, (side, values) in sides.items():
            for arm in ARMS:
                flag.zero_()
                out = legs[f"{arm}_{name}_k{k}"]()
                judged[f"{arm}_{name}_k{k}"] = Judge(arm, side, values, tables[k][name], a.sample).of(out, int(flag.item()))
                del out

    # the unit solve launch alone, this build beside the parent's, on the same operands
    ab, same_bits = {}, {}
    if a.parent_lib:
        this, parent = unit_solver(_lib.LIB_PATH), unit_solver(a.parent_lib)
        for k in KS:
            for name, (side, _) in sides.items():
                y = tables[k][name]
                gram = ops.als_gram(y)
                outs = [torch.empty((side.plan.numel(), k), device="cuda") for _ in range(2)]
                ab[f"unit_solve_{name}_k{k}"] = (lambda side=side, y=y, gram=gram, out=outs[0]:
                                                 this(side, y, gram, out))
                ab[f"parent_unit_solve_{name}_k{k}"] = (lambda side=side, y=y, gram=gram, out=outs[1]:
                                                        parent(side, y, gram, out))
                same_bits[f"{name}_k{k}"] = bool(torch.equal(ab[f"unit_solve_{name}_k{k}"](),
                                                             ab[f"parent_unit_solve_{name}_k{k}"]()))
    timed = {**legs, **ab}
    for fn in timed.values():                                 # warm up every shape the timed windows use
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in timed}
    for _ in range(WINDOWS):                                  # alternating, so drift hits every leg alike
        for name, fn in timed.items():
            if name in ab:                                    # the two builds of a pair run back to back on the same
                fn()                                          # operands: each timed launch follows an untimed one of
            times[name].append(window(fn, a.reps))            # its own, so neither finds the caches warmer
    res = dict(metric="als_weighted_half_sweep_ml20m_shape", argv=sys.argv[1:], users=USERS, items=ITEMS, pairs=pairs,
               reg=REG, alpha=ALPHA, values="seeded integers 1..5", windows=WINDOWS, reps=a.reps,
               device=torch.cuda.get_device_name(0),
               longest_list={name: int(side.lengths.max()) for name, (side, _) in sides.items()},
               judged_against_float64=judged, unit_solve_bitwise_equal_to_parent=same_bits, legs={})
    for name in timed:
        k = int(name.split("_k")[1])
        med = statistics.median(times[name])
        rows = USERS if "_user_" in name else ITEMS
        flop = 2 * k * k * pairs + rows * k ** 3 // 3
        res["legs"][name] = dict(k=k, s_median=med, s_min=min(times[name]), s_max=max(times[name]), rows=rows,
                                 flop=flop, tflops=flop / med / 1e12)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
