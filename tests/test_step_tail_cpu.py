"""CPU: the bounds of step_tail_ref.py are neither loose nor flaky.  torch's own fp32 Adam / BCELoss stay inside them
on the exact inputs test_gpu_step_tail.py feeds the HIP kernels, and the float64 rule with one thing changed falls
outside.  Every ratio is printed before it is asserted (pytest -s shows them)."""
import pytest
import torch

import step_tail_ref as ref


def _torch_adam(hyper):
    return lambda params: torch.optim.Adam(params, foreach=False, **hyper)


@pytest.mark.parametrize("which,scale", ref.ADAM_HYPER_CASES)
def test_torch_fp32_adam_inside_bound_hyper_sets(which, scale):
    hyper = ref.ADAM_SETS[which]
    refs = ref.adam_reference(ref.ADAM_HYPER_SIZES, 11 + which, 6, hyper, scale, ref.ADAM_JUMP)
    params, opt = ref.run_adam(_torch_adam(hyper), "cpu", ref.ADAM_HYPER_SIZES, 11 + which, 6, scale, ref.ADAM_JUMP)
    rp, rm, rv = ref.adam_ratios(params, opt, refs)
    print(f"torch fp32 Adam set {which} scale {scale:g}: p {rp:.3f} m {rm:.3f} v {rv:.3f} of the bound")
    assert rp <= 1 and rm <= 1 and rv <= 1


def test_torch_fp32_adam_inside_bound_big_sizes():
    hyper = ref.ADAM_SETS[0]
    refs = ref.adam_reference(ref.ADAM_BIG_SIZES, 21, 3, hyper)
    params, opt = ref.run_adam(_torch_adam(hyper), "cpu", ref.ADAM_BIG_SIZES, 21, 3)
    rp, rm, rv = ref.adam_ratios(params, opt, refs)
    print(f"torch fp32 Adam big sizes: p {rp:.3f} m {rm:.3f} v {rv:.3f} of the bound")
    assert rp <= 1 and rm <= 1 and rv <= 1


@pytest.mark.parametrize("count", ref.ADAM_COUNTS)
def test_torch_fp32_adam_inside_bound_tensor_counts(count):
    hyper, sizes = ref.ADAM_SETS[0], ref.adam_count_sizes(count)
    assert len(set(sizes)) == count and all(n % 2 == 1 for n in sizes)
    refs = ref.adam_reference(sizes, 31 + count, 3, hyper)
    params, opt = ref.run_adam(_torch_adam(hyper), "cpu", sizes, 31 + count, 3)
    rp, rm, rv = ref.adam_ratios(params, opt, refs)
    print(f"torch fp32 Adam {count} tensors: p {rp:.3f} m {rm:.3f} v {rv:.3f} of the bound")
    assert rp <= 1 and rm <= 1 and rv <= 1


def _fp32_adam(p, g, m, v, step, rows, lr, betas, eps, weight_decay, far_end=False):
    """a correct fp32 row-wise Adam: exp_avg from the nearer end, as ATen's lerp and the kernels form it"""
    b1, b2 = betas
    gr = g[rows] + weight_decay * p[rows]
    if (1.0 - b1) >= 0.5 and not far_end:
        m[rows] = gr - (gr - m[rows]) * b1
    else:
        m[rows] = m[rows] + (gr - m[rows]) * (1.0 - b1)
    v[rows] = v[rows] * b2 + (1.0 - b2) * gr * gr
    p[rows] = p[rows] - (lr / (1.0 - b1 ** step)) * (m[rows] / (v[rows].sqrt() / (1.0 - b2 ** step) ** 0.5 + eps))


@pytest.mark.parametrize("which", range(len(ref.ROWS_HYPERS)))
@pytest.mark.parametrize("dim", ref.ROWS_DIMS)
def test_fp32_rowwise_rule_inside_bound(dim, which):
    """a correct fp32 row-wise Adam fits the float64 bound at every hyper-parameter set the GPU test runs"""
    hyper = ref.ROWS_HYPERS[which]
    p, m, v, batches = ref.rows_case(dim)
    r = ref.AdamRef(p, m, v)
    for step, (ids, vals) in enumerate(batches, 1):
        g = torch.zeros_like(p).index_add_(0, ids, vals)
        rows = torch.unique(ids)
        _fp32_adam(p, g, m, v, step, rows, **hyper)
        r.step(g, step, rows=rows, **hyper)
    got = (ref.ratio(p, r.p, r.tol_p), ref.ratio(m, r.m, r.tol_m), ref.ratio(v, r.v, r.tol_v))
    print(f"fp32 row-wise rule dim {dim} betas {hyper['betas']}: p {got[0]:.3f} m {got[1]:.3f} v {got[2]:.3f} of the bound")
    assert max(got) <= 1
    untouched = torch.ones(ref.ROWS_VOCAB, dtype=torch.bool)
    untouched[torch.cat([ids for ids, _ in batches])] = False
    assert untouched.any() and float(r.tol_p[untouched].max()) == 0.0            # rows no step touched earn nothing


def _mutated(p, g, m, v, step, lr, betas, eps, weight_decay, omb2_scale=1.0):
    """the float64 rule with (1 - beta2) as a separate knob"""
    b1, b2 = betas
    gr = g + weight_decay * p
    m += (1.0 - b1) * (gr - m)
    v.mul_(b2).add_(omb2_scale * (1.0 - b2) * gr * gr)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p -= (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps))


MUTATIONS = {
    "omb2 +1%": lambda h, s: (dict(h, omb2_scale=1.01), s),
    "lr +0.1%": lambda h, s: (dict(h, lr=h["lr"] * 1.001), s),
    "eps x10": lambda h, s: (dict(h, eps=h["eps"] * 10), s),
    "step +1": lambda h, s: (h, s + 1),
    "no decay": lambda h, s: (dict(h, weight_decay=0.0), s),
}


def _applies(name, hyper):
    if name == "no decay":
        return hyper["weight_decay"] > 0
    if name == "step +1":
        return hyper["betas"] != (0.0, 0.0)      # both bias corrections are exactly 1 at every step
    return True


@pytest.mark.parametrize("which,scale", ref.ADAM_HYPER_CASES)
def test_wrong_rules_fall_outside_bound(which, scale):
    hyper, sizes, seed = ref.ADAM_SETS[which], ref.ADAM_HYPER_SIZES[:1], 11 + which
    refs = ref.adam_reference(ref.ADAM_HYPER_SIZES, seed, 6, hyper, scale, ref.ADAM_JUMP)
    # the first six steps only: a fresh reference of the first tensor, stepped alongside the mutants
    good = ref.AdamRef(ref.adam_params(sizes, seed)[0])
    wrong = {k: ref.AdamRef(ref.adam_params(sizes, seed)[0]) for k in MUTATIONS if _applies(k, hyper)}
    for step in range(1, 7):
        g = ref.adam_grads(ref.ADAM_HYPER_SIZES, seed, step, scale)[0].double()
        good.step(g, step, **hyper)
        for k, w in wrong.items():
            h, s = MUTATIONS[k](hyper, step)
            _mutated(w.p, g, w.m, w.v, s, **h)
    assert refs[0].p.shape == good.p.shape
    for k, w in wrong.items():
        r = ref.ratio(w.p, good.p, good.tol_p)
        print(f"set {which} scale {scale:g} {k}: {r:.1f} x the bound")
        assert r > 1, k
    # and the knob-free restatement is the oracle's rule
    same = ref.AdamRef(ref.adam_params(sizes, seed)[0])
    for step in range(1, 7):
        _mutated(same.p, ref.adam_grads(ref.ADAM_HYPER_SIZES, seed, step, scale)[0].double(), same.m, same.v, step, **hyper)
    assert ref.ratio(same.p, good.p, good.tol_p) < 1e-6


@pytest.mark.parametrize("n", ref.BCE_SIZES)
def test_torch_fp32_bce_inside_bounds(n):
    p, y = ref.bce_inputs(n)
    a = p.view(n, 1).clone().requires_grad_(True)
    loss = torch.nn.BCELoss()(a, y.view(n, 1))
    loss.backward()
    want, grad, tol = ref.bce_reference(p, y)
    rl, rg = abs(float(loss.detach()) - want) / tol, ref.bce_grad_ratio(a.grad, grad)
    print(f"torch fp32 BCELoss n {n}: loss {rl:.3f} of the bound, gradient {rg:.3f} ({8 * rg:.2f} * 2^-24)")
    assert rl <= 1 and rg <= 1


def test_bce_bounds_notice_wrong_rules():
    n = 65536
    p, y = ref.bce_inputs(n)
    want, grad, tol = ref.bce_reference(p, y)
    dropped = ref.bce_reference(p[:-1], y[:-1])[0] * (n - 1) / n           # the last element never summed
    assert abs(dropped - want) > tol
    noclamp = ref.bce_reference(p[8:], y[8:])[0]                             # the -100 terms gone
    assert abs(noclamp - want) > tol
    assert ref.bce_grad_ratio(grad * (1 + 2.0 ** -20), grad) > 1             # 1/n formed for n + 4096 samples or so
    assert ref.bce_passes(262144) == 4 and ref.bce_passes(262145) == 5 and ref.bce_passes(1) == 1


@pytest.mark.parametrize("near_end,inside", [(True, True), (False, False)])
def test_lerp_from_the_far_end_falls_outside_at_beta1_zero(near_end, inside):
    """exp_avg.lerp_(gr, 1 - beta1) in fp32: ATen starts from the nearer end (weight >= 0.5: gr - (gr - m) beta1).
    m + (1 - beta1)(gr - m) at beta1 = 0 loses a small gr below ulp(m), and m / sqrt(v) = +-1 makes that a visible
    step.  The kernels must take ATen's form; the bound tells the two apart."""
    hyper, sizes, seed = ref.ADAM_SETS[3], ref.ADAM_HYPER_SIZES[:1], 14
    (b1, b2), lr, eps, wd = hyper["betas"], hyper["lr"], hyper["eps"], hyper["weight_decay"]
    good = ref.AdamRef(ref.adam_params(sizes, seed)[0])
    p = ref.adam_params(sizes, seed)[0]
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 7):
        g = ref.adam_grads(ref.ADAM_HYPER_SIZES, seed, step)[0]
        good.step(g, step, **hyper)
        gr = g + wd * p
        m = gr - (gr - m) * b1 if near_end else m + (gr - m) * (1.0 - b1)
        v = v * b2 + (1.0 - b2) * gr * gr
        p = p - (lr / (1.0 - b1 ** step)) * (m / (v.sqrt() / (1.0 - b2 ** step) ** 0.5 + eps))
    r = ref.ratio(p, good.p, good.tol_p)
    print(f"fp32 Adam at betas (0, 0), lerp from the {'near' if near_end else 'far'} end: {r:.3f} of the bound")
    assert (r <= 1) == inside


@pytest.mark.parametrize("broken", ["exp_avg", "exp_avg_sq"])
def test_moment_bounds_bite_on_their_own(broken):
    """the float64 rule with one moment's decay constant off by 2^-16 (a constant rounded to half precision, say):
    that moment leaves its bound while the other, which does not depend on it, stays exact"""
    hyper, sizes, seed = ref.ADAM_SETS[0], ref.ADAM_HYPER_SIZES[:1], 11
    (b1, b2), wd = hyper["betas"], hyper["weight_decay"]
    good = ref.AdamRef(ref.adam_params(sizes, seed)[0])
    p = ref.adam_params(sizes, seed)[0].double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    off = 1.0 + 2.0 ** -16
    for step in range(1, 7):
        g = ref.adam_grads(ref.ADAM_HYPER_SIZES, seed, step)[0].double()
        gr = g + wd * good.p                      # the good trajectory's p: only the moments are under test
        good.step(g, step, **hyper)
        m = m + (1.0 - b1 * (off if broken == "exp_avg" else 1.0)) * (gr - m)
        v = v * (b2 * (off if broken == "exp_avg_sq" else 1.0)) + (1.0 - b2) * gr * gr
    rm, rv = ref.ratio(m, good.m, good.tol_m), ref.ratio(v, good.v, good.tol_v)
    print(f"{broken} decay off by 2^-16: exp_avg {rm:.2f}, exp_avg_sq {rv:.2f} of their bounds")
    assert (rm > 1) == (broken == "exp_avg") and (rv > 1) == (broken == "exp_avg_sq")
    assert min(rm, rv) < 1e-6
