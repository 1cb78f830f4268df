#!/usr/bin/env python3
"""ALS half-sweeps at the ml-20m shape (138 493 users x 26 744 items, the ~14.8 M distinct synthetic pairs of
dev/gdcf_bench.py's Zipf draw), k = 64 and k = 128, hipEvent-timed after warm-up; prints one JSON line and writes it to
``profiles/als_bench_ml20m.json`` (``--out``).

  leg (a): ``ops.als_gram`` + ``ops.als_solve_rows`` -- the user half-sweep, the item half-sweep and the Gram launch
           alone (of the item table, the one the user half-sweep takes)
  leg (b): a plain-PyTorch composition of the same half-sweep on the same GPU: rows longest list first, in chunks of
           at most ``--torch-entries`` padded list entries and ``--torch-rows`` systems, padded gather, ``bmm`` for sum q q^T, ``torch.linalg.cholesky``
           and ``torch.cholesky_solve``

Neither leg is the other's yardstick: each is judged on its own against float64 (``numpy.linalg.solve`` of the
normal equations built from the fp32 inputs) on ``--sample`` rows spread over the launch order -- the worst
``max|x - x64| / max|x64|`` and the worst residual ``max|A x - b| / (|A|_inf max|x| + max|b|)`` -- once cold (the first
call of each leg in the process, fused first) and once after warm-up in the reverse order (PyTorch first).  The fused
leg passes an ``err_flag`` and the line records its bits.

The legs alternate in one process; each figure is the median of 7 windows of ``--reps`` half-sweeps; the peak device
memory of one half-sweep of each leg is taken beyond what was allocated before it.  A half-sweep is 2 k^2 FLOP per pair
plus k^3 / 3 per row.  No threshold is attached.  Kernel times are not taken here: run

    rocprofv3 --kernel-trace --stats -d <dir> -- python dev/als_bench.py --trace

in a run of its own (``--trace``: three half-sweeps of leg (a) per side and k, nothing timed, nothing written).

    python dev/als_bench.py [--reps 1] [--out profiles/als_bench_ml20m.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeplearningrecommendationsystem_amd import ops  # noqa: E402
from deeplearningrecommendationsystem_amd.data import ObservedPairs  # noqa: E402

USERS, ITEMS, DRAWS, KS, WINDOWS = 138_493, 26_744, 20_000_263, (64, 128), 7
REG, ALPHA = 0.1, 40.0


class Side:
    def __init__(self, pairs):
        self.pairs = pairs
        self.lengths = pairs.indptr.diff()
        self.plan = torch.argsort(self.lengths, descending=True, stable=True).contiguous()


FLAG = None      # device int32 the fused leg ORs its guard bits into; read outside the timed windows


def fused_half(side, fixed):
    gram = ops.als_gram(fixed)
    return ops.als_solve_rows(fixed, gram, side.pairs.indptr, side.pairs.indices, REG, ALPHA, rows=side.plan,
                              err_flag=FLAG)


class Judge:
    """float64 solutions of ``sample`` rows of one (side, table), made once on the host; ``of(out)`` judges a leg's
    (rows in plan order, k) output against them"""

    def __init__(self, side, fixed, sample):
        y = fixed.double().cpu().numpy()
        gram = y.T @ y
        k = y.shape[1]
        indptr, indices = side.pairs.indptr.cpu().numpy(), side.pairs.indices.cpu().numpy()
        plan = side.plan.cpu().numpy()
        self.at = np.unique(np.linspace(0, plan.size - 1, sample).astype(np.int64))     # first and last row included
        self.a, self.b, self.x = [], [], []
        for j in self.at:
            x = y[indices[indptr[plan[j]]:indptr[plan[j] + 1]]]
            a = gram + ALPHA * (x.T @ x) + REG * np.eye(k)
            b = (1.0 + ALPHA) * x.sum(0)
            self.a.append(a)
            self.b.append(b)
            self.x.append(np.linalg.solve(a, b))

    def of(self, out):
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
                    zeroed_rows=zero_rows, finite=bool(torch.isfinite(out).all()))


def torch_half(side, fixed, entries, max_rows):
    """the same rows in the same order from library calls alone"""
    k = fixed.shape[1]
    gram = fixed.T @ fixed
    eye = torch.eye(k, device=fixed.device) * REG
    out = torch.empty((side.plan.numel(), k), device=fixed.device)
    lengths = side.lengths[side.plan]
    host = lengths.cpu().tolist()
    indptr, indices = side.pairs.indptr, side.pairs.indices
    s = 0
    while s < len(host):
        width = max(host[s], 1)                               # the longest list of the chunk: rows are sorted
        e = min(len(host), s + max(1, min(max_rows, entries // width)))
        rows = side.plan[s:e]
        col = torch.arange(width, device=fixed.device)
        live = col[None, :] < lengths[s:e, None]
        at = (indptr[rows][:, None] + col[None, :]).clamp_(max=max(indices.numel() - 1, 0))
        x = fixed[indices[at].long()] * live[:, :, None]     # (rows, width, k), zeros past a list's end
        a = gram + ALPHA * torch.bmm(x.transpose(1, 2), x) + eye
        b = (1.0 + ALPHA) * x.sum(1)
        out[s:e] = torch.cholesky_solve(b[:, :, None], torch.linalg.cholesky(a))[:, :, 0]
        s = e
    return out


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def peak_of(fn):
    """peak bytes allocated during fn beyond what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1, help="half-sweeps per timed window")
    ap.add_argument("--torch-entries", type=int, default=1 << 21, help="padded list entries per chunk of leg (b)")
    ap.add_argument("--torch-rows", type=int, default=2048, help="systems per chunk of leg (b) at the most")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--sample", type=int, default=300, help="rows of each half-sweep judged against float64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_bench_ml20m.json"))
    ap.add_argument("--trace", action="store_true", help="three untimed half-sweeps of leg (a), for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("als_bench needs the GPU: nothing is measured without one")
    rng = np.random.default_rng(0)
    pop = 1.0 / np.arange(1, ITEMS + 1)
    pop = pop[rng.permutation(ITEMS)]
    u = torch.from_numpy(rng.integers(0, USERS, DRAWS)).cuda()
    i = torch.from_numpy(rng.choice(ITEMS, size=DRAWS, p=pop / pop.sum())).cuda()
    by_user = ObservedPairs(u, i, USERS, ITEMS)
    users = torch.repeat_interleave(torch.arange(USERS, device="cuda"), by_user.indptr.diff())
    by_item = ObservedPairs(by_user.indices.long(), users, ITEMS, USERS)
    del u, i, users
    global FLAG
    FLAG = torch.zeros(1, dtype=torch.int32, device="cuda")
    sides = {"user": Side(by_user), "item": Side(by_item)}
    pairs = len(by_user)
    gen = torch.Generator(device="cuda").manual_seed(0)
    tables = {k: {"user": (torch.randn(ITEMS, k, device="cuda", generator=gen) * 0.1).contiguous(),     # the FIXED table
                  "item": (torch.randn(USERS, k, device="cuda", generator=gen) * 0.1).contiguous()} for k in KS}

    legs = {}
    for k in KS:
        for name, side in sides.items():
            legs[f"fused_{name}_k{k}"] = lambda side=side, y=tables[k][name]: fused_half(side, y)
        legs[f"gram_k{k}"] = lambda y=tables[k]["user"]: ops.als_gram(y)
    if a.trace:
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        return
    if not a.skip_torch:
        for k in KS:
            for name, side in sides.items():
                legs[f"torch_{name}_k{k}"] = lambda side=side, y=tables[k][name]: torch_half(side, y, a.torch_entries, a.torch_rows)

    # each leg against float64, on its own: cold (the first call of the process, fused first) ...
    judges = {(name, k): Judge(sides[name], tables[k][name], a.sample) for k in KS for name in sides}
    kinds = ("fused",) if a.skip_torch else ("fused", "torch")
    judged = {}
    for (name, k), judge in judges.items():
        for kind in kinds:
            judged[f"{kind}_{name}_k{k}"] = dict(cold=judge.of(legs[f"{kind}_{name}_k{k}"]()))
    for fn in legs.values():                                  # warm up every shape the timed windows use
        fn()
    torch.cuda.synchronize()
    # ... and warm, in the reverse order (PyTorch first); the two legs against each other on every row, warm
    agree = {}
    for (name, k), judge in reversed(list(judges.items())):
        outs = {kind: legs[f"{kind}_{name}_k{k}"]() for kind in reversed(kinds)}
        for kind, out in outs.items():
            judged[f"{kind}_{name}_k{k}"]["warm"] = judge.of(out)
        if not a.skip_torch:
            agree[f"{name}_k{k}"] = float((outs["fused"] - outs["torch"]).abs().max() / outs["torch"].abs().max())
        del outs
    del judges
    times = {name: [] for name in legs}
    for _ in range(WINDOWS):                                  # alternating, so drift hits every leg alike
        for name, fn in legs.items():
            times[name].append(window(fn, a.reps))
    longest = {name: int(side.lengths.max()) for name, side in sides.items()}
    res = dict(metric="als_half_sweep_ml20m_shape", argv=sys.argv[1:], users=USERS, items=ITEMS, pairs=pairs,
               reg=REG, alpha=ALPHA, windows=WINDOWS, reps=a.reps, device=torch.cuda.get_device_name(0),
               longest_list=longest, fused_err_flag_bits=int(FLAG.item()), judged_against_float64=judged,
               max_rel_diff_fused_vs_torch_warm=agree, legs={})
    for name, fn in legs.items():
        k = int(name.split("_k")[1])
        med = statistics.median(times[name])
        leg = dict(k=k, s_median=med, s_min=min(times[name]), s_max=max(times[name]), peak_bytes=peak_of(fn))
        if not name.startswith("gram"):
            rows = USERS if "_user_" in name else ITEMS
            flop = 2 * k * k * pairs + rows * k ** 3 // 3
            leg.update(rows=rows, flop=flop, tflops=flop / med / 1e12)
        res["legs"][name] = leg
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
