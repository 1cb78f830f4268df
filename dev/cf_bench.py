#!/usr/bin/env python3
"""Neighbourhood-CF stages at ml-20m shape (138 493 users x 26 744 items, ~20 M synthetic pairs, Zipf item
popularity), hipEvent-timed after warm-up; prints one JSON line.

Stages: user kNN (ctr_cf_knn over the rows), item kNN (over the columns), recommend-all-users at n = 20.  Each kNN
stage reports its i8 op rate 2 * q * rows * cols_pad against the i8 MFMA peak (2x the 2.5 PF bf16 dense peak).
Baseline: the same kNN composed from plain PyTorch on the same GPU (chunked fp32 normalised matmul + torch.topk).
By default every stage, the baseline included, is the full self-join.  ``--query-rows Q`` / ``--torch-query-rows Q``
time Q query rows against all rows instead and scale by rows / Q; the JSON records Q.  That scaling is only sound
when Q covers whole device rounds: ctr_cf_knn runs one 128-row workgroup per CU (LDS-bound occupancy), so a grid of
fewer than 256 workgroups leaves CUs idle and the scaled time overstates the speed.

    python dev/cf_bench.py [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeplearningrecommendationsystem_amd import cf, ops  # noqa: E402

I8_PEAK = 5.0e15


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / 1e3)
    return best


def torch_knn(x, kk, q0, q):
    """plain PyTorch: normalised fp32 rows, chunked matmul against all rows, torch.topk"""
    xf = x.float()
    xf = xf / xf.norm(dim=1, keepdim=True).clamp_min(1e-30)
    out = []
    for s in range(q0, q0 + q, 2048):
        sim = xf[s:min(s + 2048, q0 + q)] @ xf.t()
        out.append(torch.topk(sim, kk, dim=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263)
    ap.add_argument("--query-rows", type=int, default=0)
    ap.add_argument("--torch-query-rows", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    pop = 1.0 / np.arange(1, a.items + 1)
    pop = pop[rng.permutation(a.items)]
    u = rng.integers(0, a.users, a.pairs)
    i = rng.choice(a.items, size=a.pairs, p=pop / pop.sum())
    mat = cf.implicit_matrix(u, i, a.users, a.items)
    res = dict(metric="cf_stages_ml20m_shape", argv=sys.argv[1:], users=a.users, items=a.items, pairs=int(mat.counts.sum()))
    for name, x in (("user_knn", mat.data), ("item_knn", mat.transposed())):
        rows, cols = x.shape
        counts = x.sum(1, dtype=torch.int32)
        q = rows if a.query_rows <= 0 else min(rows, a.query_rows)
        t = timed(lambda: ops.cf_knn(x, counts, 11, 0, q), a.reps) * rows / q
        ops_ = 2.0 * rows * rows * cols
        res[name + "_s"] = t
        res[name + "_i8_frac_peak"] = ops_ / t / I8_PEAK
        tq = rows if a.torch_query_rows <= 0 else min(rows, a.torch_query_rows)
        tt = timed(lambda: torch_knn(x, 11, 0, tq), 1) * rows / tq
        res[name + "_torch_s"] = tt
        res[name + "_speedup_vs_torch"] = tt / t
        res[name + "_query_rows_timed"] = q
        res[name + "_torch_query_rows_timed"] = tq
    model = cf.UserCF(10).fit(mat)
    torch.cuda.synchronize()
    res["recommend_all_users_s"] = timed(lambda: model.recommend(n=20), a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
