"""Float64 reference, bounds and input builders for the group losses (csrc/group_loss.hip; ``loss.BPRLoss``,
``loss.SampledSoftmaxLoss``).  Imported by test_gpu_group_loss.py (the HIP kernels) and by test_group_loss_cpu.py
(torch's own fp32 on the same inputs, and deliberately wrong rules), so the two cannot drift.

The definition is the kernel file's header comment.  n groups of w = 1 + k probabilities, slot 0 the positive:
    z   = max(log p, -100) - max(log(1 - p), -100)
    BPR      L = 1/(n k) sum_g sum_{j>=1} softplus(z_gj - z_g0);    dz_gj = sigmoid(z_gj - z_g0)/(n k), dz_g0 = -sum_j dz_gj
    softmax  L = 1/n sum_g [logsumexp_j z_gj - z_g0];                dz_gj = (softmax_j - [j == 0])/n
    dL/dp = dz / max(p (1 - p), 1e-12)
The reference forms 1 - p and p (1 - p) in float32 first, as the kernel does (and as step_tail_ref does for BCE),
then takes logs, clamps, and computes softplus / log-sum-exp in float64: it measures the kernel's log, exp and sums,
not the rounding the two share.

What is compared.  den = max(p (1 - p), 1e-12) is the same float32 number on both sides, and near p = 0 or 1 it is
tiny: dz/dp is huge there and the gradient w.r.t. p is ill-conditioned in p.  Every gradient comparison is therefore
made on  gprob * den,  i.e. on dz, for every input and not only for the saturated ones; a wrong den (another floor,
p (1 - p) formed differently) still shows, because the reference's den multiplies the kernel's quotient.

Bounds, by counting roundings (u = 2^-24; a correctly rounded operation loses u relative, logf / expf / log1pf one
ulp <= 2u relative; the factor 4 in front is the project's margin for fused multiply-add and operation order):
    ez_i  = 2u (|log p_i| + |log(1 - p_i)|) + u |z_i|                   the two logs and the subtraction
  BPR, x = z_j - z_0:
    ex_j  = ez_j + ez_0 + u |x_j|
    softplus term:  ex_j (softplus is 1-Lipschitz) + 3u softplus(x_j)    (log1p and the sum)
    dz_j (j >= 1):  relative  ex_j (d log sigmoid / dx <= 1) + 8u         (exp, 1 + e, the divide, the product with
                                                                          1/(n k) and that constant's three roundings)
    dz_0:           sum_j bound_j + u depth_g |dz_0|                      depth_g = log2 G + ceil(w / G)
  softmax, a_j = z_j - m, E = max_j ez_j:
    r_j   = 2E + u |a_j| + 2u                                            relative error of exp(a_j)
    r_S   = sum_j softmax_j r_j + u depth_g                              of the sum
    dz_j:  [softmax_j (r_j + r_S + u) + 4u |softmax_j - [j == 0]|] / n
    term:  ez_m + ez_0 + r_S + 2u |log S| + 2u (|m + log S| + |term|)
  both:
    every dz bound + 2^-126 (below it fp32 has no relative precision: exp(-200) is 0 in fp32, 1.4e-87 in the reference)
    and + 2u |dz| for the divide by den and the product with the upstream gradient
    loss:  scale * sum term bounds + u depth |L_abs|,  depth = depth_g + passes + 34
           (L_abs = scale * sum |term|; 34: the wave tree 6, the four wave sums, the last workgroup's trees 8 + 4,
           the products with the scale and the tail)
    passes = tiles a workgroup of the capped forward grid takes, from the kernel's grid rule (``fwd_grid``).

Measured on the CPU by test_group_loss_cpu.py on the very inputs the GPU tests use, a correct fp32 implementation
in torch ops (worst element over the bound, over every case of CASES, TIE_CASES and SAT_CASES):
    BPR      loss 0.014   dz 0.11
    softmax  loss 0.009   dz 0.07
(the loss bound counts every sum as if its roundings lined up; they do not).  Against the same bounds the float64
rule with one thing changed lands outside on every case of CASES (smallest worst ratio over the cases, loss / dz):
1/n for 1/(n k) (BPR, k >= 2): 4.6e4 / 2.0e5;  the positive's gradient with the wrong sign: dz 1.1e5;  slot 1 taken
as the positive: 5.4e2 / 1.8e5;  max not subtracted is only wrong in fp32 and only on saturated groups, where
exp(100) overflows: NaN on every case of SAT_CASES.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
FLOOR = float(torch.tensor(1e-12, dtype=torch.float32))
BPR, SOFTMAX = 0, 1

KS = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 99)
NS = (1, 3, 257)
SATURATED = (0.0, 1.0, 2.0 ** -149, 1.0 - 2.0 ** -24)


def lanes(k):
    """G of the kernel: the smallest power of two >= 1 + k, capped at 64"""
    g = 2
    while g < 1 + k and g < 64:
        g *= 2
    return g


def fwd_grid(n, k):
    """(workgroups, tiles per workgroup) of the forward launch: 256 / G groups per tile, a workgroup per four tiles,
    at most 256 workgroups"""
    tiles = -(-n // (256 // lanes(k)))
    grid = min(-(-tiles // 4), 256)
    return grid, -(-tiles // grid)


# the smallest n at k = 1 whose capped grid takes more than the four tiles per workgroup it is sized for
N_CAPPED = 256 * 4 * (256 // lanes(1)) + 129
assert fwd_grid(N_CAPPED, 1) == (256, 5) and fwd_grid(N_CAPPED - 129, 1) == (256, 4)

CASES = [(n, k) for k in KS for n in NS] + [(N_CAPPED, 1)]
TIE_CASES = [(3, 1), (3, 4), (5, 63), (3, 99)]
SAT_CASES = [(8, 1), (3, 4), (5, 7), (3, 64), (3, 99)]


def random_inputs(n, k):
    """n groups of 1 + k probabilities, logits of scale 2"""
    g = torch.Generator().manual_seed(9000 + 131 * n + k)
    return torch.sigmoid(torch.randn(n * (1 + k), generator=g) * 2.0)


def tied_inputs(n, k):
    """group 0: every slot the same number; group 1: one negative equal to the positive; the rest: two values only"""
    g = torch.Generator().manual_seed(9100 + 131 * n + k)
    two = torch.sigmoid(torch.randn(n, 2, generator=g) * 2.0)
    p = two.gather(1, torch.randint(0, 2, (n, 1 + k), generator=g))
    p[0, :] = 0.625
    if n > 1:
        p[1, 1] = p[1, 0]
    return p.reshape(-1).contiguous()


def saturated_inputs(n, k):
    """every slot one of p = 0, 1, 2^-149, 1 - 2^-24 or 0.5 / 0.9; group 0 has the positive at 0 against a negative
    at 1 (z = -100 against +100), group 1 the reverse, and every saturated value appears as a positive and as a
    negative"""
    g = torch.Generator().manual_seed(9200 + 131 * n + k)
    values = torch.tensor(SATURATED + (0.5, 0.9), dtype=torch.float64).float()
    p = values[torch.randint(0, values.numel(), (n, 1 + k), generator=g)]
    p[0, 0], p[0, 1] = 0.0, 1.0
    if n > 1:
        p[1, 0], p[1, 1] = 1.0, 0.0
    for at, v in enumerate(values[:4]):      # as positives (slot 0 of groups 2..) and as negatives
        if 2 + at < n:
            p[2 + at, 0] = v
        if k >= 4:
            p[n - 1, 1 + at] = v
        else:
            p[n - 1 - at, 1] = v
    return p.reshape(-1).contiguous()


def ratio(got, want, tol):
    """worst |got - want| / tol over the elements; nan if anything is nan"""
    err = (got.detach().cpu().double().reshape(-1) - want.reshape(-1)).abs()
    r = err / tol.reshape(-1)
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def den_of(p):
    """max(p (1 - p), 1e-12) formed in float32, as float64"""
    p = p.detach().reshape(-1).cpu()
    return ((1.0 - p) * p).clamp_min(FLOOR).double()


def reference(p, k, kind):
    """float64 reference from the flat fp32 probabilities ``p`` (n (1 + k) of them) -> dict:
    loss, loss_bound (floats), dz, dz_bound, den, gprob (float64 tensors, flat, for an upstream gradient of 1)"""
    p = p.detach().reshape(-1).cpu()
    w = 1 + k
    n = p.numel() // w
    assert n * w == p.numel() and n >= 1
    lp = torch.log(p.double()).clamp_min(-100.0)
    l1p = torch.log((1.0 - p).double()).clamp_min(-100.0)        # 1 - p formed in fp32
    z = (lp - l1p).view(n, w)
    ez = (2 * U * (lp.abs() + l1p.abs())).view(n, w) + U * z.abs()
    depth_g = math.log2(lanes(k)) + -(-w // lanes(k))
    depth = depth_g + fwd_grid(n, k)[1] + 34
    if kind == BPR:
        scale = 1.0 / (n * k)
        x = z[:, 1:] - z[:, :1]
        ex = ez[:, 1:] + ez[:, :1] + U * x.abs()
        term = torch.nn.functional.softplus(x, threshold=1e9)
        term_bound = (ex + 3 * U * term).sum(1)
        dz = torch.empty_like(z)
        dz[:, 1:] = torch.sigmoid(x) * scale
        dz[:, 0] = -dz[:, 1:].sum(1)
        bound = torch.empty_like(z)
        bound[:, 1:] = (ex + 8 * U) * dz[:, 1:]
        bound[:, 0] = bound[:, 1:].sum(1) + U * depth_g * dz[:, 0].abs()
        terms = term.sum(1)
    else:
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


def loss_ratio(got, ref):
    got = float(got.detach()) if torch.is_tensor(got) else float(got)
    return float("nan") if math.isnan(got) else abs(got - ref["loss"]) / ref["loss_bound"]


def dz_ratio(gprob, ref, gloss=1.0):
    """worst error of ``gprob * den`` against ``gloss * dz`` over its bound (module docstring: what is compared)"""
    got = gprob.detach().cpu().double().reshape(-1) * ref["den"]
    return ratio(got, ref["dz"] * gloss, ref["dz_bound"] * abs(gloss))
