#!/usr/bin/env python3
"""The full softmax over the catalogue at the ml-20m catalogue (I = 26 744 items, k = 64), batches of 8192 and 65 536
query rows: forward (row pass) and backward (scaling dX, column pass) of ``ops.softmax_full_rows`` /
``ops.softmax_full_cols``, hipEvent-timed after warm-up; prints one JSON line and writes it to
``profiles/softmax_full_bench.json`` (``--out``).

  leg (a): this op, forward and backward, at both batch sizes
  leg (b): ``F.cross_entropy(x @ q.T, t, reduction="none")`` with its backward on the same GPU, at B = 8192 only (the
           logits alone are 876 MB there and 7 GB at 65 536)

The legs alternate in one process; each figure is the median of 7 windows of ``--reps`` steps; the peak device memory
of a step of each leg is taken beyond what was allocated before it.  A step is four 2 B I k products; the share of the
155 TF fp32 matrix rate is that count over the step time (an end-to-end figure: it includes the merge launches and the
dX scaling).  No threshold is attached.  Kernel times are not taken here: run

    rocprofv3 --kernel-trace --stats -d <dir> -- python dev/softmax_full_bench.py --trace

in a run of its own (``--trace``: three steps of leg (a) per shape, nothing timed, nothing written).

    python dev/softmax_full_bench.py [--reps 5] [--out profiles/softmax_full_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeplearningrecommendationsystem_amd import ops  # noqa: E402

F32_MFMA_PEAK = 155e12
ITEMS, K, BATCHES, TORCH_BATCH, WINDOWS = 26_744, 64, (8192, 65_536), 8192, 7


def inputs(batch, gen):
    x = (torch.randn(batch, K, device="cuda", generator=gen) * 0.1).contiguous()
    t = torch.randint(0, ITEMS, (batch,), device="cuda", generator=gen)
    g = torch.full((batch,), 1.0 / batch, device="cuda")
    return x, t, g


def fused_step(x, q, t, g):
    nll, lse, gx = ops.softmax_full_rows(x, q, t)
    dx = gx * g.unsqueeze(1)
    dq = ops.softmax_full_cols(x, q, t, lse, g, nll=nll)
    return nll, dx, dq


def torch_step(x, q, t, g):
    x, q = x.detach().requires_grad_(True), q.detach().requires_grad_(True)
    nll = torch.nn.functional.cross_entropy(x @ q.T, t, reduction="none")
    nll.backward(g)
    return nll.detach(), x.grad, q.grad


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
    ap.add_argument("--reps", type=int, default=5, help="steps per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_full_bench.json"))
    ap.add_argument("--trace", action="store_true", help="three untimed steps of leg (a) per shape, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_full_bench needs the GPU: nothing is measured without one")
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = (torch.randn(ITEMS, K, device="cuda", generator=gen) * 0.1).contiguous()
    data = {b: inputs(b, gen) for b in BATCHES}
    legs = {f"fused_b{b}": (lambda b=b: fused_step(data[b][0], q, data[b][1], data[b][2])) for b in BATCHES}
    if a.trace:
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        return
    legs[f"torch_b{TORCH_BATCH}"] = lambda: torch_step(data[TORCH_BATCH][0], q, data[TORCH_BATCH][1], data[TORCH_BATCH][2])

    # the two legs at B = 8192 compute the same thing
    mine, theirs = legs[f"fused_b{TORCH_BATCH}"](), legs[f"torch_b{TORCH_BATCH}"]()
    agree = {name: float((u - v).abs().max() / v.abs().max()) for name, u, v in zip(("nll", "dx", "dq"), mine, theirs)}
    del mine, theirs

    for fn in legs.values():                                # warm up every shape the timed windows use
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(WINDOWS):                                # alternating, so drift hits every leg alike
        for name, fn in legs.items():
            times[name].append(window(fn, a.reps))
    res = dict(metric="softmax_full_step", argv=sys.argv[1:], items=ITEMS, k=K, windows=WINDOWS, reps=a.reps,
               device=torch.cuda.get_device_name(0), max_rel_diff_vs_torch_b8192=agree, legs={})
    for name, fn in legs.items():
        batch = int(name.split("_b")[1])
        med = statistics.median(times[name])
        flop = 8 * batch * ITEMS * K                        # four products of 2 B I k
        res["legs"][name] = dict(batch=batch, step_s_median=med, step_s_min=min(times[name]), step_s_max=max(times[name]),
                                 step_flop=flop, tflops=flop / med / 1e12, share_of_f32_mfma_peak=flop / med / F32_MFMA_PEAK,
                                 peak_step_bytes=peak_of(fn))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
