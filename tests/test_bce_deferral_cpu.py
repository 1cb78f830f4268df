"""Host: the switch that lets a captured step defer ``BCELoss`` into NeuralCF's backward (``loss.deferred_bce``).
Outside a captured step ``BCELoss`` behaves as before; the state does not outlive its block, whatever ends it; and the
C ABI mirror carries the three new members at the end of ``ctr_ncf_proj_grad_t``."""
import ctypes

import pytest
import torch

from deeplearningrecommendationsystem_amd import _lib, loss
from deeplearningrecommendationsystem_amd._lib import CtrHipError


class _Run:
    deferred = None


def test_no_deferral_outside_a_captured_step():
    assert loss._deferral is None
    run, prob = _Run(), torch.rand(8, 1, requires_grad=True)
    loss.offer_deferral(run, prob)               # nobody listens
    assert loss._deferral is None and run.deferred is None
    # the eager loss takes its own launch, which has no CPU fallback: as before
    with pytest.raises(CtrHipError):
        loss.BCELoss()(prob, torch.rand(8, 1))


def test_the_state_does_not_survive_its_block():
    with loss.deferred_bce() as d:
        assert loss._deferral is d and d.run is None
        loss.offer_deferral(_Run(), torch.rand(4, 1))
        assert d.run is not None
    assert loss._deferral is None
    with pytest.raises(KeyError):
        with loss.deferred_bce():
            loss.offer_deferral(_Run(), torch.rand(4, 1))
            raise KeyError("as a failed capture would")
    assert loss._deferral is None
    with loss.deferred_bce():
        with pytest.raises(RuntimeError, match="nest"):
            with loss.deferred_bce():
                pass
        assert loss._deferral is not None        # the inner refusal leaves the outer block alone
    assert loss._deferral is None


def test_only_the_offered_prob_with_a_float32_target_defers():
    prob = torch.rand(6, 1, requires_grad=True)
    with loss.deferred_bce() as d:
        # nothing offered
        assert loss._deferrable(prob, torch.rand(6, 1)) is None
        loss.offer_deferral(_Run(), prob)
        # a host target, a float64 target, another size, another tensor than the offered one: today's path
        assert loss._deferrable(prob, torch.rand(6, 1)) is None
        assert loss._deferrable(prob, torch.rand(6, 1).double()) is None
        assert loss._deferrable(prob, torch.rand(5, 1)) is None
        assert loss._deferrable(prob * 1.0, torch.rand(6, 1)) is None
        assert loss._deferrable(prob.detach(), torch.rand(6, 1)) is None
        with pytest.raises(CtrHipError):
            loss.BCELoss()(prob, torch.rand(6, 1))
        assert d.run is not None                 # a call that did not defer consumes nothing

    class Sub(loss.BCELoss):
        pass
    with loss.deferred_bce():
        loss.offer_deferral(_Run(), prob)
        with pytest.raises(CtrHipError):
            Sub()(prob, torch.rand(6, 1))        # exactly BCELoss, not a subclass


def test_grad_struct_ends_in_target_stride_loss():
    names = [f[0] for f in _lib.NcfProjGrad._fields_]
    assert names[-5:] == ["phases", "reserved", "target", "ldtarget", "loss"]
    # gprob + stride, four layers, 13 pointers / int64, phases + reserved, then the three new members
    assert ctypes.sizeof(_lib.NcfProjGrad) == 2 * 8 + 4 * 64 + 13 * 8 + 8 + 3 * 8
    g = _lib.NcfProjGrad()
    assert g.target is None and g.loss is None and g.ldtarget == 0
