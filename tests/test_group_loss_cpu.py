"""CPU: the float64 reference of the group losses (group_loss_ref.py) against torch's own autograd on logits, its
bounds against a correct fp32 implementation and against deliberately wrong rules on the very inputs the GPU tests
use, and the entry points' argument validation."""
import ctypes
import math

import pytest
import torch

import group_loss_ref as ref

KINDS = (ref.BPR, ref.SOFTMAX)


def rule(p, k, kind, dtype=torch.float32, wrong=None):
    """the definition in torch ops of ``dtype`` (1 - p and p (1 - p) in float32 either way) -> (loss, gprob), the
    gradient w.r.t. z by autograd; ``wrong`` changes one thing"""
    p = p.detach().reshape(-1)
    w = 1 + k
    n = p.numel() // w
    den = ((1.0 - p) * p).clamp_min(ref.FLOOR).to(dtype)
    z = (torch.log(p.to(dtype)).clamp_min(-100.0) - torch.log((1.0 - p).to(dtype)).clamp_min(-100.0)).view(n, w)
    z.requires_grad_(True)
    zs = z
    if wrong == "slot1":
        order = [1, 0] + list(range(2, w))
        zs = z[:, order]
    if kind == ref.BPR:
        x = zs[:, 1:] - zs[:, :1]
        terms = -torch.nn.functional.logsigmoid(-x)       # softplus(x), stable, with the right derivative at 0
        loss = terms.sum() * (1.0 / n if wrong == "one_over_n" else 1.0 / (n * k))
    elif wrong == "no_max":
        loss = (torch.log(torch.exp(zs).sum(1)) - zs[:, 0]).sum() / n
    else:
        m = zs.max(1, keepdim=True).values.detach()
        loss = (m[:, 0] + torch.log(torch.exp(zs - m).sum(1)) - zs[:, 0]).sum() / n
    dz, = torch.autograd.grad(loss, z)
    if wrong == "positive_sign":
        dz = dz.clone()
        dz[:, 0] = -dz[:, 0]
    return loss.detach(), (dz.reshape(-1) / den).detach()


def _all_inputs():
    for n, k in ref.CASES:
        yield "random", n, k, ref.random_inputs(n, k)
    for n, k in ref.TIE_CASES:
        yield "tied", n, k, ref.tied_inputs(n, k)
    for n, k in ref.SAT_CASES:
        yield "saturated", n, k, ref.saturated_inputs(n, k)


_refs = {}


def _reference(name, n, k, kind, p):
    key = (name, n, k, kind)
    if key not in _refs:
        _refs[key] = ref.reference(p, k, kind)
    return _refs[key]


def test_reference_agrees_with_torch_autograd_on_logits():
    """p = m / 4096 has an exact 1 - p in float32, so the reference's z is logit(p) and the two must agree to
    float64 rounding"""
    g = torch.Generator().manual_seed(1)
    for n, k in ((1, 1), (7, 4), (33, 99)):
        p = (torch.randint(1, 4096, (n * (1 + k),), generator=g).double() / 4096.0).float()
        z = (torch.log(p.double()) - torch.log1p(-p.double())).view(n, 1 + k).requires_grad_(True)
        bpr = -torch.nn.functional.logsigmoid(z[:, :1] - z[:, 1:]).mean()
        ce = torch.nn.functional.cross_entropy(z, torch.zeros(n, dtype=torch.int64))
        for kind, loss in ((ref.BPR, bpr), (ref.SOFTMAX, ce)):
            dz, = torch.autograd.grad(loss, z)
            got = ref.reference(p, k, kind)
            assert abs(got["loss"] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
            torch.testing.assert_close(got["dz"], dz.reshape(-1), rtol=1e-10, atol=1e-15)
            torch.testing.assert_close(got["gprob"] * ref.den_of(p), dz.reshape(-1), rtol=1e-10, atol=1e-15)
            # the composition with the model's sigmoid backward: dL/dp * p (1 - p) = dz
            torch.testing.assert_close(got["gprob"] * (p.double() * (1 - p.double())), dz.reshape(-1), rtol=1e-6, atol=1e-15)


def test_the_input_sets_hold_what_they_promise():
    for n, k in ref.SAT_CASES:
        p = ref.saturated_inputs(n, k).view(n, 1 + k)
        assert p[0, 0] == 0.0 and p[0, 1] == 1.0 and p[1, 0] == 1.0 and p[1, 1] == 0.0
        for v in torch.tensor(ref.SATURATED, dtype=torch.float64).float():
            assert (p[:, 1:] == v).any(), (n, k, float(v))
    got = {float(v) for n, k in ref.SAT_CASES for v in ref.saturated_inputs(n, k).view(n, 1 + k)[:, 0]}
    assert {float(v) for v in torch.tensor(ref.SATURATED, dtype=torch.float64).float()} <= got
    for n, k in ref.TIE_CASES:
        p = ref.tied_inputs(n, k).view(n, 1 + k)
        assert (p[0] == p[0, 0]).all() and p[1, 1] == p[1, 0]
    assert ref.fwd_grid(ref.N_CAPPED, 1)[1] > 4


def test_a_correct_fp32_implementation_is_inside_the_bounds():
    worst = {kind: [0.0, 0.0] for kind in KINDS}
    for name, n, k, p in _all_inputs():
        for kind in KINDS:
            want = _reference(name, n, k, kind, p)
            loss, gprob = rule(p, k, kind)
            got = (ref.loss_ratio(loss, want), ref.dz_ratio(gprob, want))
            assert got[0] < 1.0 and got[1] < 1.0, (name, n, k, kind, got)
            worst[kind] = [max(a, b) for a, b in zip(worst[kind], got)]
    print("torch fp32 over the bounds (loss, dz): BPR", worst[ref.BPR], "softmax", worst[ref.SOFTMAX])


def _outside(x):
    return math.isnan(x) or x > 1.0


def test_wrong_rules_land_outside_the_bounds():
    least = {}
    for name, n, k, p in _all_inputs():
        if name != "random" or n == ref.N_CAPPED:
            continue
        for kind in KINDS:
            want = _reference(name, n, k, kind, p)
            wrongs = ["positive_sign", "slot1"] + (["one_over_n"] if kind == ref.BPR and k >= 2 else [])
            for wrong in wrongs:
                loss, gprob = rule(p, k, kind, torch.float64, wrong)
                got = (ref.loss_ratio(loss, want), ref.dz_ratio(gprob, want))
                if wrong == "positive_sign":
                    assert _outside(got[1]), (wrong, n, k, kind, got)
                    got = (math.inf, got[1])
                else:
                    assert _outside(got[0]) and _outside(got[1]), (wrong, n, k, kind, got)
                key = (wrong, kind)
                least[key] = tuple(min(a, b) for a, b in zip(least.get(key, (math.inf, math.inf)), got))
    for key, value in sorted(least.items()):
        print("wrong rule", key, "smallest worst ratio (loss, dz):", value)
    # max not subtracted: only fp32 and only saturated groups show it (exp(100) overflows)
    for n, k in ref.SAT_CASES:
        p = ref.saturated_inputs(n, k)
        want = _reference("saturated", n, k, ref.SOFTMAX, p)
        loss, gprob = rule(p, k, ref.SOFTMAX, torch.float32, "no_max")
        assert _outside(ref.loss_ratio(loss, want)) and _outside(ref.dz_ratio(gprob, want)), (n, k)


def test_a_nan_input_is_a_nan_reference():
    p = ref.random_inputs(3, 4)
    p[7] = float("nan")
    for kind in KINDS:
        assert math.isnan(ref.reference(p, 4, kind)["loss"]) and math.isnan(ref.loss_ratio(0.0, ref.reference(p, 4, kind)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def test_group_loss_entry_point_validation_without_gpu(lib):
    h = lib.load()
    buf = (ctypes.c_float * 512)()
    word = (ctypes.c_uint32 * 1)()
    a, t = ctypes.addressof(buf), ctypes.addressof(word)

    def fwd(prob=a, ldp=1, n=4, k=4, kind=0, loss=a, ws=a, ticket=t):
        return h.ctr_group_loss_fwd(prob, ldp, n, k, kind, loss, ws, 256, ticket, None, None)

    def bwd(prob=a, ldp=1, n=4, k=4, kind=0, gloss=a, gprob=a, ldg=1):
        return h.ctr_group_loss_bwd(prob, ldp, n, k, kind, gloss, gprob, ldg, None)

    # every refusal is the only thing wrong with an otherwise valid call (a valid one would launch: not made here)
    for call in (fwd, bwd):
        assert call(n=0) == -1                    # a mean over nothing
        assert call(n=-1) == -1
        assert call(k=0) == -1
        assert call(k=lib.CTR_GROUP_MAX_K + 1) == -1 and lib.CTR_GROUP_MAX_K + 1 == 4096
        assert call(kind=2) == -1 and call(kind=-1) == -1
        assert call(prob=None) == -1
        assert call(ldp=0) == -1 and call(ldp=-1) == -1
    assert fwd(loss=None) == -1 and fwd(ticket=None) == -1 and fwd(ws=None) == -1
    assert bwd(gloss=None) == -1 and bwd(gprob=None) == -1 and bwd(ldg=0) == -1
    # too little workspace for the grid: 1025 groups of 2 -> 3 workgroups
    assert h.ctr_group_loss_fwd(a, 1, 1025, 1, 0, a, a, 2, t, None, None) == -2


def test_group_loss_modules_validation_without_gpu(lib):
    from deeplearningrecommendationsystem_amd.loss import BCELoss, BPRLoss, SampledSoftmaxLoss
    for cls, kind in ((BPRLoss, 0), (SampledSoftmaxLoss, 1)):
        fn = cls(4)
        assert (fn.group_size, fn.negatives, fn.kind) == (5, 4, kind)
        with pytest.raises(lib.CtrHipError):
            fn(torch.rand(10), torch.zeros(10))                # a CPU tensor: no fallback, as BCELoss
        for bad in (0, -1, lib.CTR_GROUP_MAX_K + 1):
            with pytest.raises(ValueError):
                cls(bad)
    with pytest.raises(lib.CtrHipError):
        BCELoss()(torch.rand(10), torch.zeros(10))
