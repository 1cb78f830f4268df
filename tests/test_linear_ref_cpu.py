"""CPU only.  tests/linear_ref.py against autograd, its case table against the restated dispatch, and its comparisons
against small mutations of the reference: what tests/test_gpu_linear_arms.py trusts, checked without a GPU.

* linear_fwd_ref / linear_bwd_ref equal float64 autograd of torch.nn.functional.linear + activation;
* every table entry (arm, workspace extent) equals plan_bwd(), the entry points' arithmetic in Python, and every arm
  of the dispatch has a case;
* negative controls: each mutation of the float64 result, rounded to float32 like a kernel's output, must be rejected
  by the comparison the GPU test applies, at EVERY case of the table the mutation changes anything at
  (mutation_applies: "gb added twice" has no meaning for a call without gb, "the relu mask from gy" none without a
  relu); the unmutated result must pass.  Every mutation is applied at at least one case and every case meets at least
  one mutation."""
import pytest
import torch

import linear_ref as ref

TIGHT = dict(rtol=1e-11, atol=1e-12)
_cache = {}


def _case(c):
    """operands and the unmutated float64 result, computed once per case"""
    if c.name not in _cache:
        _cache.clear()                                   # (the 65536-row cases: keep one at a time)
        ops_ = ref.bwd_operands(c)
        _cache[c.name] = (ops_, ref.bwd_reference(c, ops_))
    return _cache[c.name]


@pytest.mark.parametrize("act", [0, 1, 2])
def test_the_references_equal_autograd(act):
    gen = torch.Generator().manual_seed(act)
    m, n, k = 37, 5, 7
    x, w, b, r, gy = (torch.randn(*s, generator=gen) for s in ((m, k), (n, k), (n,), (m, n), (m, n)))
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    z = torch.nn.functional.linear(xd, wd, bd) + r.double()
    y = [z, torch.relu(z), torch.sigmoid(z)][act]
    y.backward(gy.double())
    torch.testing.assert_close(ref.linear_fwd_ref(x, w, b, r, act), y.detach(), **TIGHT)
    gx0, gw0, gb0 = (torch.randn(*s, generator=gen) for s in ((m, k), (n, k), (n,)))
    out = ref.linear_bwd_ref(x, w, y.detach(), gy, act, gx0, gw0, gb0, True)
    torch.testing.assert_close(out["gx"], gx0.double() + xd.grad, **TIGHT)
    torch.testing.assert_close(out["gw"], gw0.double() + wd.grad, **TIGHT)
    torch.testing.assert_close(out["gb"], gb0.double() + bd.grad, **TIGHT)
    out = ref.linear_bwd_ref(x, w, y.detach(), gy, act, torch.full((m, k), float("nan")), None, None, False)
    torch.testing.assert_close(out["gx"], xd.grad, **TIGHT)
    assert out["gw"] is None and out["gb"] is None


@pytest.mark.parametrize("c", ref.BWD_CASES, ids=lambda c: c.name)
def test_the_table_follows_the_dispatch(c):
    assert c.arm in ref.ARMS
    assert ref.plan_bwd(c) == (c.arm, c.extent)
    assert c.ws is None or c.extent <= c.ws <= ref.AMPLE


def test_the_table_is_complete():
    names = [c.name for c in ref.BWD_CASES]
    assert len(set(names)) == len(names)
    assert {c.arm for c in ref.BWD_CASES} == set(ref.ARMS)
    for mutate in ref.BWD_MUTATIONS:
        assert any(ref.mutation_applies(c, mutate) for c in ref.BWD_CASES), mutate
    for c in ref.BWD_CASES:
        assert any(ref.mutation_applies(c, mutate) for mutate in ref.BWD_MUTATIONS), c.name


def _f32(d):
    return {k: (None if v is None else v.float()) for k, v in d.items()}


@pytest.mark.parametrize("c", ref.BWD_CASES, ids=lambda c: c.name)
def test_the_backward_comparison_passes_the_reference_and_rejects_every_mutation(c):
    ops_, want = _case(c)
    ref.check_bwd(c, _f32(want), want)
    gwv, gwbuf = ops_["gw"]
    ref.check_gaps(gwbuf, gwv, f"{c.name} gw buffer")
    applied = 0
    for mutate in ref.BWD_MUTATIONS:
        if not ref.mutation_applies(c, mutate):
            continue
        applied += 1
        if mutate == "write_gaps":                       # the slab's rows stored with the slab's own row stride
            buf = gwbuf.clone()
            buf[gwv.off:gwv.off + c.n * c.k] = 0.0
            assert ref.rejects(ref.check_gaps, buf, gwv, "mutated"), f"{c.name}: 'write_gaps' passed"
            continue
        wrong = _f32(ref.bwd_reference(c, ops_, mutate))
        assert ref.rejects(ref.check_bwd, c, wrong, want), f"{c.name}: '{mutate}' passed the comparison"
    assert applied > 0


@pytest.mark.parametrize("c", ref.FWD_CASES, ids=lambda c: c.name)
def test_the_forward_comparison_passes_the_reference_and_rejects_every_mutation(c):
    x, w, b, r, yv, ybuf = ref.fwd_operands(c)
    want = ref.linear_fwd_ref(x, w, b, r, c.act)
    ref.check_fwd(c, want.float(), want)
    ref.check_gaps(ybuf, yv, f"{c.name} y buffer")
    touched = ybuf.clone()
    touched[c.n] = 0.0                                   # the float behind row 0
    assert ref.rejects(ref.check_gaps, touched, yv, "mutated")
    if c.tail0 is None:                                  # a single column has no second launch
        assert c.n == 1
        return
    for mutate in ref.FWD_MUTATIONS:
        wrong = ref.linear_fwd_ref(x, w, b, r, c.act, c.tail0, mutate).float()
        assert ref.rejects(ref.check_fwd, c, wrong, want), f"{c.name}: '{mutate}' passed the comparison"
