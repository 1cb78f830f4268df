"""The group losses on the device (csrc/group_loss.hip; ``loss.BPRLoss`` / ``loss.SampledSoftmaxLoss``) against the
float64 reference of group_loss_ref.py, within the bounds derived and measured there.  Gradients are compared as
``gprob * den`` (= dz), see that module's docstring.  Shapes: every lane count G on both sides of each power of two and
the lane loop (k = 99), one to several workgroups, and one n whose capped grid takes more than its four tiles."""
import math

import pytest
import torch

import group_loss_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = [ref.BPR, ref.SOFTMAX]


def _lib():
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def _ticket():
    from deeplearningrecommendationsystem_amd.loss import _ticket
    return _ticket(torch.device(DEV))


def _strided(p, ldp):
    """the values of ``p`` at stride ``ldp`` behind one float of offset, NaN everywhere else -> (buffer, view)"""
    buf = torch.full((1 + p.numel() * ldp,), float("nan"), device=DEV)
    view = buf[1:][::ldp]
    view.copy_(p)
    assert view.data_ptr() == buf.data_ptr() + 4 and (view.numel() < 2 or view.stride(0) == ldp)
    return buf, view


def _fwd(view, ldp, n, k, kind, with_grad=True):
    lib = _lib()
    loss = torch.full((), float("nan"), device=DEV)
    ws = torch.empty(256, device=DEV)
    gp1 = torch.full((n * (1 + k),), float("nan"), device=DEV) if with_grad else None
    rc = lib.load().ctr_group_loss_fwd(view.data_ptr(), ldp, n, k, kind, loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _ticket().data_ptr(), lib.ptr(gp1), lib.stream_ptr())
    lib.check(rc, "ctr_group_loss_fwd")
    return loss, gp1


def _bwd(view, ldp, n, k, kind, gloss, ldg):
    lib = _lib()
    out = torch.full((n * (1 + k) * ldg,), float("nan"), device=DEV)
    up = torch.tensor(gloss, dtype=torch.float32, device=DEV)
    rc = lib.load().ctr_group_loss_bwd(view.data_ptr(), ldp, n, k, kind, up.data_ptr(), out.data_ptr(), ldg,
                                       lib.stream_ptr())
    lib.check(rc, "ctr_group_loss_bwd")
    return out


_refs = {}


def _reference(name, n, k, kind, p):
    key = (name, n, k, kind)
    if key not in _refs:
        _refs[key] = ref.reference(p, k, kind)
    return _refs[key]


def _check(name, n, k, kind, p):
    want = _reference(name, n, k, kind, p)
    _ticket().zero_()
    for ldp in (1, 2):
        buf, view = _strided(p.to(DEV), ldp)
        loss, gp1 = _fwd(view, ldp, n, k, kind)
        again, _ = _fwd(view, ldp, n, k, kind, with_grad=False)
        ratios = (ref.loss_ratio(loss, want), ref.dz_ratio(gp1, want))
        print(name, "n", n, "k", k, "kind", kind, "ldp", ldp, "loss", float(loss), "reference", want["loss"],
              "over the bounds (loss, dz):", ratios)
        assert ratios[0] < 1.0 and ratios[1] < 1.0, (name, n, k, kind, ldp, ratios)
        assert torch.equal(loss, again), "two runs give one loss, bit for bit"
        assert int(_ticket().item()) == 0, "the ticket is re-armed"
        unit = _bwd(view, ldp, n, k, kind, 1.0, 1)
        assert torch.equal(unit, gp1), "gprob_unit is the backward for an upstream of 1, bit for bit"
        scaled = _bwd(view, ldp, n, k, kind, -2.5, 2)
        assert ref.dz_ratio(scaled[::2], want, -2.5) < 1.0
        assert torch.isnan(scaled[1::2]).all(), "ldg = 2: the floats between are not written"
        assert torch.isnan(buf[0]) and (ldp == 1 or torch.isnan(buf[2::2]).all()), "the input is not written"


@pytest.mark.parametrize("n,k", ref.CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_loss_and_gradients_against_float64(kind, n, k):
    _check("random", n, k, kind, ref.random_inputs(n, k))


@pytest.mark.parametrize("n,k", ref.TIE_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_ties_within_a_group(kind, n, k):
    _check("tied", n, k, kind, ref.tied_inputs(n, k))


@pytest.mark.parametrize("n,k", ref.SAT_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_saturated_probabilities(kind, n, k):
    """p exactly 0, exactly 1, 2^-149 and 1 - 2^-24: the logs clamp at -100, z reaches +-100, den its floor"""
    _check("saturated", n, k, kind, ref.saturated_inputs(n, k))


@pytest.mark.parametrize("kind", KINDS)
def test_one_nan_input_is_a_nan_loss(kind):
    for n, k, at in ((3, 4, 7), (3, 4, 5), (2, 99, 150), (300, 1, 411)):      # a negative, a positive, the lane loop
        p = ref.random_inputs(n, k)
        p[at] = float("nan")
        loss, _ = _fwd(p.to(DEV), 1, n, k, kind)
        assert math.isnan(float(loss)), (n, k, at)
        assert int(_ticket().item()) == 0


def _modules():
    from deeplearningrecommendationsystem_amd.loss import BPRLoss, SampledSoftmaxLoss
    return {ref.BPR: BPRLoss, ref.SOFTMAX: SampledSoftmaxLoss}


@pytest.mark.parametrize("kind", KINDS)
def test_modules_and_the_unit_grad_shortcut(kind):
    from deeplearningrecommendationsystem_amd.loss import unit_grad
    n, k = 257, 4
    p = ref.random_inputs(n, k)
    want = _reference("random", n, k, kind, p)
    fn = _modules()[kind](k)
    target = torch.zeros(n * (1 + k), 1, device=DEV)
    # (B, 1) as the models return it; backward() with torch's own 1.0: the backward kernel
    prob = p.to(DEV).view(-1, 1).requires_grad_(True)
    loss = fn(prob, target)
    assert loss.shape == () and ref.loss_ratio(loss, want) < 1.0
    written = loss.grad_fn.gp1
    loss.backward()
    assert prob.grad.shape == prob.shape and prob.grad.data_ptr() != written.data_ptr()
    assert torch.equal(prob.grad.view(-1), written) and ref.dz_ratio(prob.grad, want) < 1.0
    # THE 1.0 of the device: the tensor the forward wrote comes back, no launch
    loss = fn(prob, target)
    got, = torch.autograd.grad(loss, prob, unit_grad(torch.device(DEV)))
    assert got.data_ptr() == loss.grad_fn.gp1.data_ptr() and got.shape == prob.shape
    assert ref.dz_ratio(got, want) < 1.0
    # another upstream gradient
    loss = fn(prob, target)
    got, = torch.autograd.grad(loss, prob, torch.tensor(3.0, device=DEV))
    assert ref.dz_ratio(got, want, 3.0) < 1.0
    # under no_grad nothing is kept for a backward
    with torch.no_grad():
        assert ref.loss_ratio(fn(prob, target), want) < 1.0
    # a strided input (a column of a wider matrix)
    wide = torch.full((n * (1 + k), 3), float("nan"), device=DEV)
    wide[:, 1] = p.to(DEV)
    assert ref.loss_ratio(fn(wide[:, 1], None), want) < 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_modules_refuse_what_bce_refuses(kind):
    fn = _modules()[kind](4)
    with pytest.raises(ValueError):
        fn(torch.rand(12, device=DEV), None)                             # not whole groups of 5
    with pytest.raises(ValueError):
        fn(torch.rand(10, device=DEV, dtype=torch.float64), None)
    with pytest.raises(ValueError):
        fn(torch.rand(0, device=DEV), None)
