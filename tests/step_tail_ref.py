"""References, bounds and input builders for the tail of every training step: ``loss.BCELoss``, ``optim.Adam`` and
the row-wise Adam of the sparse mode.  Imported by test_gpu_step_tail.py (the HIP kernels) and by
test_step_tail_cpu.py (torch's own fp32 on the same inputs, and deliberately wrong rules), so the two cannot drift.

Adam.  The reference is ``oracle.ctr_oracle.adam_update`` on float64 copies of the same fp32 inputs, with and without
``rows=``.  The tolerance on ``p`` is per element and accumulates over the steps of a trajectory:

    tol_p += 4 * 2^-24 * (|p_before| + 8 * |p_after - p_before|)          (both from the float64 trajectory)

The inner expression is what a correct fp32 Adam can lose on inputs that are the same fp32 numbers: one rounding each
in gr, m and v, then sqrt, two divides and a multiply (sqrt and divide correctly rounded), plus the rounding of p
itself; the 4 is the margin for fused multiply-add and a different but equivalent operation order.
Measured on the CPU by test_step_tail_cpu.py, on the very inputs the GPU tests use, ``torch.optim.Adam(foreach=False)``
in fp32, worst element over the bound (x 4 for the share of the inner expression):
    set 0  lr 1e-3, betas (0.9, 0.999), eps 1e-8, wd 1e-5
    set 1  lr 1e-2, betas (0.9, 0.999), eps 1e-8, wd 0
    set 2  lr 1e-2, betas (0.5, 0.9),   eps 1e-3, wd 1e-2
    set 3  lr 3e-2, betas (0, 0),       eps 1e-8, wd 1e-3          (gradient scale 1 only)
    six steps + two at step 2001/2002, 200 003 elements, gradients of scale 1 and 1e-3:   p 0.15 .. 0.19
    three steps at up to 4 197 379 elements and with 63 .. 129 tensors:                   p 0.22 .. 0.23
    exp_avg <= 0.07, exp_avg_sq <= 0.57 of their bounds (below)
    a correct fp32 row-wise rule, dims 1 .. 64, three steps, betas (0.9, 0.999), (0.5, 0.9), (0, 0):   p 0.16 .. 0.25
i.e. a correct fp32 Adam uses 0.6 .. 1.0 of the inner expression.  Set 3 with gradients of scale 1e-3 is left out:
g + wd*p cancels, the update is sign(gr), and torch's own fp32 lands ~1100 x outside -- ill-conditioned, not a kernel
property.  Against the same bound the float64 rule with one thing changed lands far outside at every set where the
change applies (worst element, smallest over the sets): (1 - beta2) raised by 1 %: 1300 x; lr raised by 0.1 %:
430 x; eps x 10: 57 x; the step count off by one: 29 000 x; weight decay dropped: 2100 x.

The moments have bounds of their own, from the same kind of count (u = 2^-24, gr = g + wd*p):
    m' = m + (1-b1)(gr - m):  roundings of gr, of gr - m, of the fp32 constant 1-b1 and of the result:
         <= u (|gr| + 2 |gr - m| + |m'|) <= u (3 |gr| + 2 |m| + |m'|)             tol_m += 4u (|m| + |m'| + |gr|)
    v' = b2 v + ((1-b2) gr) gr:  the fp32 constants b2 and 1-b2, three products, gr twice, the sum:
         <= u (2 b2 v + 5 (1-b2) gr^2 + v') <= u (2 v + 6 v')                      tol_v += 4u (v + 2 v')
gr itself cancels when g is about -wd*p; the fp32 constant wd and the product wd*p then leave an absolute error
e = 4u * 2 wd |p| + wd * tol_p (the second term: what the error already allowed on p contributes) that the relative
terms above do not see.  It enters m' as (1-b1) e and v' as (1-b2)(2 |gr| e + e^2); both are added.
A decay constant of one moment off by 2^-16 puts that moment 43 x (exp_avg) / 19 x (exp_avg_sq) outside.

BCE.  The float64 reference forms 1 - p and p*(1 - p) in float32 first, as ATen and the kernel both do, then takes
logs, clamps at -100, floors at float32(1e-12) and divides in float64: it measures the kernel's log and sum, not the
rounding the two share.
    gradient: |got - ref| <= 8 * 2^-24 * |ref| elementwise             (torch fp32: at most 1.98 * 2^-24)
    loss:     |got - ref| <= 2^-24 * mean|term| * (20 + passes)         (torch fp32: <= 0.07 of it, n = 1 .. 600 001)
with passes = ceil(n / (grid * 256)) the kernel's serial sum length, grid = min(ceil(n / 1024), 256); the 20 covers
the log error and the depth of the two trees."""
from __future__ import annotations

import numpy as np
import torch

from oracle import ctr_oracle as orc

U = 2.0 ** -24

ADAM_SETS = (
    dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5),
    dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=1e-2),
    dict(lr=3e-2, betas=(0.0, 0.0), eps=1e-8, weight_decay=1e-3),
)
# (set, gradient scale); betas (0, 0) with small gradients and decay is ill-conditioned (see above)
ADAM_HYPER_CASES = [(k, s) for k in range(4) for s in (1.0, 1e-3) if not (k == 3 and s != 1.0)]
ADAM_HYPER_SIZES = (200003, 1025, 7)
ADAM_JUMP = 2000      # state["step"] is set to this after the first steps: bias corrections ~1, a large pow

PASS = 2048 * 256 * 4  # elements one pass of adam_kernel's capped grid covers
ADAM_BIG_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, PASS, PASS + 1, 2 * PASS + 3 * 1024 + 3)
ADAM_COUNTS = (63, 64, 65, 129)


def adam_count_sizes(count):
    """distinct odd sizes (a pack slot read from the wrong index shows), some over one workgroup's 1024 elements;
    slot 64 -- the first of the second pack -- takes more than one pass, so that pack's grid is not the first's"""
    sizes = [2 * i + 1 + (2048 if i % 5 == 0 else 0) for i in range(count)]
    if count > 64:
        sizes[64] = PASS + 1
    return tuple(sizes)


def adam_params(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in sizes]


def adam_grads(sizes, seed, step, scale=1.0):
    g = torch.Generator().manual_seed(seed * 100003 + step)
    return [torch.randn(n, generator=g) * scale for n in sizes]


class AdamRef:
    """float64 trajectory of one tensor under ``oracle.adam_update`` and the tolerances it has earned so far"""

    def __init__(self, p, m=None, v=None):
        self.p = p.detach().double().clone()
        self.m = torch.zeros_like(self.p) if m is None else m.detach().double().clone()
        self.v = torch.zeros_like(self.p) if v is None else v.detach().double().clone()
        self.tol_p, self.tol_m, self.tol_v = (torch.zeros_like(self.p) for _ in range(3))

    def step(self, g, step, rows=None, **hyper):
        sel = slice(None) if rows is None else rows
        wd, (b1, b2) = hyper.get("weight_decay", 0.0), hyper.get("betas", (0.9, 0.999))
        pb, mb, vb = self.p[sel].clone(), self.m[sel].clone(), self.v[sel].clone()
        gr = (g.double()[sel] + wd * pb).abs()
        orc.adam_update(self.p, g.double(), self.m, self.v, step, rows=rows, **hyper)
        e = 8 * U * wd * pb.abs() + wd * self.tol_p[sel]
        self.tol_m[sel] += 4 * U * (mb.abs() + self.m[sel].abs() + gr) + (1.0 - b1) * e
        self.tol_v[sel] += 4 * U * (vb + 2 * self.v[sel]) + (1.0 - b2) * (2 * gr * e + e * e)
        self.tol_p[sel] += 4 * U * (pb.abs() + 8 * (self.p[sel] - pb).abs())


def ratio(got, want, tol):
    """worst |got - want| / tol over the elements (0 for an empty tensor, nan if anything is nan)"""
    if want.numel() == 0:
        return 0.0
    err = (got.detach().cpu().double() - want).abs()
    return float((err / tol.clamp_min(1e-300)).max())


def _set_step(state, value):
    if torch.is_tensor(state["step"]):
        state["step"].fill_(value)     # torch.optim.Adam keeps a tensor
    else:
        state["step"] = value


_ref_cache = {}


def adam_reference(sizes, seed, steps, hyper, scale=1.0, jump=None):
    """[AdamRef per tensor] after ``steps`` steps (and, with ``jump``, two more at step jump+1, jump+2); computed
    once per case and shared"""
    key = (sizes, seed, steps, repr(sorted(hyper.items())), scale, jump)
    if key not in _ref_cache:
        refs = [AdamRef(p) for p in adam_params(sizes, seed)]
        numbers = list(range(1, steps + 1)) + ([jump + 1, jump + 2] if jump else [])
        for k, number in enumerate(numbers, 1):
            for r, g in zip(refs, adam_grads(sizes, seed, k, scale)):
                r.step(g, number, **hyper)
        _ref_cache[key] = refs
    return _ref_cache[key]


def run_adam(make_opt, device, sizes, seed, steps, scale=1.0, jump=None):
    """the same trajectory under an optimizer: ``make_opt(params) -> optimizer``.  Returns (params, optimizer)."""
    params = [t.to(device).requires_grad_(True) for t in adam_params(sizes, seed)]
    opt = make_opt(params)
    k = 0
    for _ in range(steps):
        k += 1
        for p, g in zip(params, adam_grads(sizes, seed, k, scale)):
            p.grad = g.to(device)
        opt.step()
    if jump:
        for p in params:
            _set_step(opt.state[p], jump)
        for _ in range(2):
            k += 1
            for p, g in zip(params, adam_grads(sizes, seed, k, scale)):
                p.grad = g.to(device)
            opt.step()
    return params, opt


def adam_ratios(params, opt, refs):
    """worst ratio to the bound of p, exp_avg, exp_avg_sq over all tensors"""
    worst = [0.0, 0.0, 0.0]
    for p, r in zip(params, refs):
        st = opt.state[p]
        got = (ratio(p, r.p, r.tol_p), ratio(st["exp_avg"], r.m, r.tol_m), ratio(st["exp_avg_sq"], r.v, r.tol_v))
        worst = [w if w >= x else x for w, x in zip(worst, got)]   # a nan sticks
    return tuple(worst)


# ------------------------------------------------------------------------------------------------------------------
# row-wise Adam
# ------------------------------------------------------------------------------------------------------------------
ROWS_DIMS = (1, 3, 4, 12, 16, 20, 64)
ROWS_VOCAB = 997
ROWS_HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3)
# the row-wise kernel forms exp_avg from the nearer end like the dense one: beta1 = 0.5 sits exactly on the switch,
# beta1 = 0 is where the far-end form fails
ROWS_HYPERS = (ROWS_HYPER, ADAM_SETS[2], ADAM_SETS[3])


def rows_case(dim, vocab=ROWS_VOCAB, seed=0, steps=3, per_step=400):
    """(p, m, v) fp32 with non-trivial moments, and per step (ids with duplicates, one gradient row per id).
    Rows vocab-1 and 0 are touched in steps 1 and 3 but not in step 2: their bias corrections use the global step."""
    g = torch.Generator().manual_seed(7919 * dim + vocab + seed)
    p = torch.randn(vocab, dim, generator=g)
    m = torch.randn(vocab, dim, generator=g) * 0.01   # small beside the gradients: 0.9 m + 0.1 gr does not cancel
    v = (0.25 + torch.rand(vocab, dim, generator=g)) * 0.01   # away from 0: m / sqrt(v) stays well-conditioned
    batches = []
    for s in range(steps):
        ids = torch.randint(1, vocab - 1, (per_step,), generator=g)
        if s != 1:
            ids[:3] = torch.tensor([0, vocab - 1, 0])
        batches.append((ids, torch.randn(per_step, dim, generator=g)))
    return p, m, v, batches


# ------------------------------------------------------------------------------------------------------------------
# BCE
# ------------------------------------------------------------------------------------------------------------------
BCE_SIZES = (1, 255, 256, 257, 1025, 65536, 262144, 262145, 600001)
BCE_EDGES = (0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -126)
BCE_FLOOR = float(np.float32(1e-12))


def bce_inputs(n):
    """(p, y) fp32 of n elements: uniform p, hard labels with soft ones (0.3 and random) mixed in and, from 16
    elements on, p = 0, 1, 1 - 2^-24 and 2^-126 against y = 0 and y = 1"""
    g = torch.Generator().manual_seed(4000 + n)
    p = torch.rand(n, generator=g)
    y = (torch.rand(n, generator=g) < 0.5).float()
    soft = torch.rand(n, generator=g)
    at = torch.arange(n)
    y = torch.where(at % 6 == 1, torch.full_like(y, 0.3), y)
    y = torch.where(at % 6 == 4, soft, y)
    if n >= 16:
        p[:8] = torch.tensor(BCE_EDGES * 2, dtype=torch.float64).float()
        y[:8] = torch.tensor([0.0] * 4 + [1.0] * 4)
    return p, y


def bce_passes(n):
    grid = min((n + 1023) // 1024, 256)
    return (n + grid * 256 - 1) // (grid * 256)


def bce_reference(p, y, gloss=1.0):
    """(loss, d loss / d p, bound on the loss) in float64 from fp32 ``p`` and ``y`` of any (equal) shape"""
    p, y = p.detach().reshape(-1).cpu(), y.detach().reshape(-1).cpu()
    one_minus, prod = (1.0 - p).double(), ((1.0 - p) * p).double()       # formed in fp32, as ATen and the kernel do
    pd, yd = p.double(), y.double()
    term = -(yd * torch.log(pd).clamp_min(-100.0) + (1.0 - yd) * torch.log(one_minus).clamp_min(-100.0))
    n = p.numel()
    grad = (pd - yd) / prod.clamp_min(BCE_FLOOR) * (gloss / n)
    return float(term.mean()), grad, U * float(term.abs().mean()) * (20 + bce_passes(n))


def bce_grad_ratio(got, want):
    """worst |got - want| / (8 * 2^-24 * |want|)"""
    return ratio(got.reshape(-1), want, 8 * U * want.abs())
