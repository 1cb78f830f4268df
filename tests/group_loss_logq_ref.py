"""Float64 reference and bounds for the logQ-corrected sampled softmax (csrc/group_loss.hip,
ctr_group_loss_logq_fwd / _bwd; ``loss.SampledSoftmaxLoss(log_q=...)``): the sibling of group_loss_ref.py, whose
constants, grid rule, input builders and comparison helpers it imports.

The definition is the kernel file's header comment: with c_i = logq[i], the softmax of group_loss_ref runs over
    z'_i = z_i - c_i                every slot, the positive's included
in place of z_i; dL/dz' keeps its form, dz'/dz = 1, dL/dp = dz / max(p (1 - p), 1e-12).

Bounds.  c is an input, the same float32 number on both sides; the only new rounding is the subtraction, so in
group_loss_ref's algebra
    ez'_i = ez_i + u |z'_i|
and every later line carries over with z' for z and ez' for ez (a_j = z'_j - m', E = max_j ez'_j, ...).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from group_loss_ref import TINY, U, den_of, fwd_grid, lanes

KS = (1, 4, 63, 64, 99)
NS = (1, 3, 257)
CASES = [(n, k) for k in KS for n in NS]
TIE_CASES = [(n, k) for k in KS for n in (3, 257)]
SAT_CASES = [(8 if k < 4 else 3, k) for k in KS] + [(257, k) for k in KS]


def heavy_tail_log_q(count, seed, items=1682):
    """``count`` values of float32(log q) at random items of a Pareto-tailed q over ``items`` items"""
    rng = np.random.default_rng(seed)
    w = rng.pareto(1.1, items) + 0.01
    q = w / w.sum()
    return torch.from_numpy(np.log(q[rng.integers(0, items, count)]).astype(np.float32))


def reference(p, c, k):
    """float64 reference from the flat fp32 probabilities ``p`` and corrections ``c`` (n (1 + k) of each) -> dict:
    loss, loss_bound (floats), dz, dz_bound, den, gprob (float64 tensors, flat, for an upstream gradient of 1)"""
    p = p.detach().reshape(-1).cpu()
    c = c.detach().reshape(-1).cpu()
    w = 1 + k
    n = p.numel() // w
    assert n * w == p.numel() == c.numel() and n >= 1
    lp = torch.log(p.double()).clamp_min(-100.0)
    l1p = torch.log((1.0 - p).double()).clamp_min(-100.0)        # 1 - p formed in fp32
    z0 = lp - l1p
    z = (z0 - c.double()).view(n, w)
    ez = (2 * U * (lp.abs() + l1p.abs()) + U * z0.abs()).view(n, w) + U * z.abs()
    depth_g = math.log2(lanes(k)) + -(-w // lanes(k))
    depth = depth_g + fwd_grid(n, k)[1] + 34
    scale = 1.0 / n
    m = z.max(1, keepdim=True)
    a = z - m.values
    big = ez.max(1, keepdim=True).values
    sm = torch.softmax(z, 1)
    r = 2 * big + U * a.abs() + 2 * U
    r_s = (sm * r).sum(1, keepdim=True) + U * depth_g
    hot = torch.zeros_like(z)
    hot[:, 0] = 1.0
    dz = (sm - hot) * scale
    bound = (sm * (r + r_s + U) + 4 * U * (sm - hot).abs()) * scale
    log_s = torch.log(torch.exp(a).sum(1))
    terms = m.values[:, 0] + log_s - z[:, 0]
    ez_m = ez.gather(1, m.indices)[:, 0]
    term_bound = ez_m + ez[:, 0] + r_s[:, 0] + 2 * U * log_s.abs() + 2 * U * ((m.values[:, 0] + log_s).abs() + terms.abs())
    loss = float(terms.sum() * scale)
    loss_bound = 4.0 * float(scale * term_bound.sum() + U * depth * scale * terms.abs().sum())
    dz_bound = 4.0 * (bound + 2 * U * dz.abs()) + TINY
    den = den_of(p)
    dz = dz.reshape(-1)
    return dict(loss=loss, loss_bound=loss_bound, dz=dz, dz_bound=dz_bound.reshape(-1), den=den, gprob=dz / den)
