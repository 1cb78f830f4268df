#!/usr/bin/env python3
"""GDCF epoch stages at ml-20m shape (138 493 users x 26 744 items, ~20 M synthetic pairs with the Zipf item
popularity of dev/cf_bench.py), k = 100, hipEvent-timed after warm-up; prints one JSON line.

Stages: the row pass (loss + dP), the column pass (dQ), the Adam step (optim.Adam, one launch per tensor), one whole
epoch (forward, backward, step) and recommend(n=50) for every user.  Each pass reports 4 m n k FLOP (two products of
2 m n k) over its time against the 155 TF fp32 MFMA rate.  Peak device memory is taken over one epoch.
Baseline: the same epoch as a plain PyTorch fp32 composition on the same GPU (P @ Q.T, BCEWithLogitsLoss against the
float32 0/1 matrix, backward, torch.optim.Adam), with its time and peak memory; its target matrix is built outside the
timed window, as the reference builds it once.

    python dev/gdcf_bench.py [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeplearningrecommendationsystem_amd import GDCF, cf, ops, optim  # noqa: E402

F32_MFMA_PEAK = 155e12


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


def peak_of(fn):
    """peak bytes allocated during fn beyond what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--pairs", type=int, default=20_000_263)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    m, n, k = a.users, a.items, a.k
    rng = np.random.default_rng(0)
    pop = 1.0 / np.arange(1, a.items + 1)
    pop = pop[rng.permutation(a.items)]
    u = rng.integers(0, a.users, a.pairs)
    i = rng.choice(a.items, size=a.pairs, p=pop / pop.sum())
    mat = cf.implicit_matrix(u, i, m, n)
    mat.transposed()
    res = dict(metric="gdcf_epoch_ml20m_shape", argv=sys.argv[1:], users=m, items=n, k=k,
               pairs=int(mat.counts.sum()), device=torch.cuda.get_device_name(0))

    model = GDCF(m, n, k, seed=0)
    opt = optim.Adam(model.parameters(), lr=0.01)
    P, Q = model.P.detach(), model.Q.detach()
    one = torch.ones((), device="cuda")
    flops_pass = 4.0 * m * n * k

    def epoch():
        loss = model(mat)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=False)

    epoch()
    t_rows = timed(lambda: ops.gdcf_rows(P, Q, mat.data), a.reps)
    t_loss = timed(lambda: ops.gdcf_rows(P, Q, mat.data, grad=False), a.reps)
    t_cols = timed(lambda: ops.gdcf_cols(P, Q, mat.transposed(), one), a.reps)
    model(mat).backward()
    t_adam = timed(opt.step, a.reps)
    t_epoch = timed(epoch, a.reps)
    t_rec = timed(lambda: model.recommend(n=50), 1)
    extra, peak = peak_of(epoch)
    res.update(row_pass_ms=t_rows * 1e3, row_pass_tflops=flops_pass / t_rows / 1e12,
               row_pass_share_of_fp32_mfma_peak=flops_pass / t_rows / F32_MFMA_PEAK,
               loss_only_ms=t_loss * 1e3, column_pass_ms=t_cols * 1e3,
               column_pass_tflops=flops_pass / t_cols / 1e12,
               column_pass_share_of_fp32_mfma_peak=flops_pass / t_cols / F32_MFMA_PEAK,
               adam_step_ms=t_adam * 1e3, epoch_ms=t_epoch * 1e3,
               epoch_tflops=2 * flops_pass / t_epoch / 1e12, recommend_all_n50_ms=t_rec * 1e3,
               epoch_peak_extra_bytes=extra, epoch_peak_allocated_bytes=peak,
               score_matrix_fp32_bytes=4 * m * n)
    del model, opt, P, Q

    if not a.skip_torch:
        y = torch.zeros((m, n), dtype=torch.float32, device="cuda")
        y[torch.from_numpy(u).cuda(), torch.from_numpy(i).cuda()] = 1.0
        del mat
        rs = np.random.RandomState(0)
        tp = torch.from_numpy(rs.rand(m, k)).float().cuda().requires_grad_()
        tq = torch.from_numpy(rs.rand(n, k).T.copy()).float().cuda().requires_grad_()
        topt = torch.optim.Adam([tp, tq], lr=0.01)
        loss_fn = torch.nn.BCEWithLogitsLoss()

        def torch_epoch():
            loss = loss_fn(tp @ tq, y)
            loss.backward()
            topt.step()
            topt.zero_grad()

        t_torch = timed(torch_epoch, a.reps)
        textra, tpeak = peak_of(torch_epoch)
        res.update(torch_epoch_ms=t_torch * 1e3, torch_epoch_peak_extra_bytes=textra,
                   torch_epoch_peak_allocated_bytes=tpeak, speedup_vs_torch=t_torch / t_epoch)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
