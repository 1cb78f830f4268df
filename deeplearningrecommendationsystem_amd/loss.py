"""``BCELoss`` -- drop-in for the ``torch.nn.BCELoss()`` every reference script builds
(e.g. scripts/pnn.py:54): mean reduction, log terms clamped at -100.  Forward is ONE launch: a pass
over the samples whose last workgroup sums the <= 256 partials in a fixed order (torch: elementwise
kernel + a single-workgroup mean), backward one pass.

``BPRLoss(negatives)`` / ``SampledSoftmaxLoss(negatives)`` -- ranking losses over groups of ``1 + negatives``
contiguous samples, the positive first: the batches of a ``data.DeviceLoader(..., grouped=True)``.  They take the
model's probabilities like ``BCELoss`` (every model of the package ends in a sigmoid) and go back to the logit; the
definitions stand in the header comment of csrc/group_loss.hip.  Same launch structure as ``BCELoss``: one forward
launch that also writes the gradient for an upstream of exactly 1, one backward pass otherwise.  The reference has
no loss over a group.  ``SampledSoftmaxLoss(negatives, log_q=...)`` is the logQ-corrected form for negatives that a
``DeviceLoader(item_sampler=...)`` does not draw uniformly (``ctr_group_loss_logq_fwd``, same header comment).

Inside a captured step (``graph.GraphedStep``) ``BCELoss`` on NeuralCF's table-row path launches nothing at all: the
model's backward launch forms the gradient from (prob, target) itself and its last launch stores the loss
(``deferred_bce`` below, csrc/ncf_proj.hip).  Eager code never takes that road: its loss has to be valid when
``loss_fn`` returns."""
from __future__ import annotations

import contextlib

import torch

from . import _lib


_tickets = {}


def _ticket(device: torch.device) -> torch.Tensor:
    """the zeroed device word ctr_bce_fwd finds its last workgroup with; the kernel leaves it zero.
    One per device: losses of one device are issued from one stream at a time here (the trainer's
    stream, or the hipGraph capture stream after its warm-up) -- a second stream computing a loss
    CONCURRENTLY would need its own word.  Created outside any capture (a tensor made during
    capture would add a fill to every replay)."""
    t = _tickets.get(device.index)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("BCELoss: run one step before capturing (GraphedStep does) so its ticket exists")
        t = _tickets[device.index] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


_units = {}


def unit_grad(device: torch.device) -> torch.Tensor:
    """THE scalar 1.0 of a device: pass it as ``loss.backward(unit_grad(dev))`` (GraphedStep does) and
    BCELoss' backward recognises it by address and returns the gradient its forward launch already
    wrote, instead of launching the scaling kernel.  Never write to it."""
    t = _units.get(device.index)
    if t is None:
        t = _units[device.index] = torch.ones((), dtype=torch.float32, device=device)
    return t


class _BCEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, target):
        _lib.require_device(prob, target)
        p, t = prob.reshape(-1), target.reshape(-1)
        if p.dtype != torch.float32 or t.dtype != torch.float32 or p.numel() != t.numel():
            raise ValueError("BCELoss expects float32 input and target of the same size")
        loss = torch.empty((), dtype=torch.float32, device=prob.device)
        ws = torch.empty(256, dtype=torch.float32, device=prob.device)
        # d loss / d prob for an upstream gradient of exactly 1, written by the same launch
        gp1 = torch.empty(p.numel(), dtype=torch.float32, device=prob.device) if ctx.needs_input_grad[0] else None
        rc = _lib.load().ctr_bce_fwd(p.data_ptr(), p.stride(0) if p.numel() > 1 else 1, t.data_ptr(),
                                     t.stride(0) if t.numel() > 1 else 1, p.numel(), loss.data_ptr(),
                                     ws.data_ptr(), ws.numel(), _ticket(prob.device).data_ptr(), _lib.ptr(gp1),
                                     _lib.stream_ptr())
        _lib.check(rc, "ctr_bce_fwd")
        ctx.save_for_backward(p, t)
        ctx.shape = prob.shape
        ctx.gp1 = gp1
        return loss

    @staticmethod
    def backward(ctx, gloss):
        p, t = ctx.saved_tensors
        unit = _units.get(p.device.index)
        if ctx.gp1 is not None and unit is not None and gloss.data_ptr() == unit.data_ptr():
            return ctx.gp1.view(ctx.shape), None  # upstream gradient is THE 1.0: forward wrote this already
        gp = torch.empty(p.numel(), dtype=torch.float32, device=p.device)
        g = gloss.contiguous()
        rc = _lib.load().ctr_bce_bwd(p.data_ptr(), p.stride(0) if p.numel() > 1 else 1, t.data_ptr(),
                                     t.stride(0) if t.numel() > 1 else 1, p.numel(), g.data_ptr(), gp.data_ptr(), 1,
                                     _lib.stream_ptr())
        _lib.check(rc, "ctr_bce_bwd")
        return gp.view(ctx.shape), None


# ---------------------------------------------------------------------------
# the loss deferred into the backward of the model that produced ``prob``
# ---------------------------------------------------------------------------
class _Deferral:
    """what a step that runs under ``deferred_bce`` knows: ``run`` is the forward (``ops.NcfProj``) whose backward can
    form the loss, ``prob`` the tensor it returned.  The model offers both (``offer_deferral``); nobody else does."""

    def __init__(self):
        self.run = self.prob = None


_deferral = None     # set only inside ``deferred_bce``


@contextlib.contextmanager
def deferred_bce():
    """Inside, ``BCELoss()(prob, target)`` on a ``prob`` that a model offered with ``offer_deferral`` launches nothing:
    it hands the model's backward the target and the loss tensor it returns.  The loss is valid only after
    ``loss.backward(unit_grad(device))`` has run -- which is why only a step that always runs the backward right behind
    the loss (``GraphedStep``) may enter here.  The state is gone when the block is left, by an exception too."""
    global _deferral
    if _deferral is not None:
        raise RuntimeError("deferred_bce does not nest")
    _deferral = _Deferral()
    try:
        yield _deferral
    finally:
        _deferral = None


def offer_deferral(run, prob: torch.Tensor) -> None:
    """a model's forward says: the backward of ``run`` (its ``backward`` takes ``target`` and ``loss``) can form the BCE
    loss of ``prob``.  Outside ``deferred_bce`` this is nothing."""
    if _deferral is not None:
        _deferral.run, _deferral.prob = run, prob


class _DeferredBCEFunction(torch.autograd.Function):
    """no launch: the gradient it passes back is a PLACEHOLDER that is never read -- ``run``'s backward recognises it by
    address (as this one recognises ``unit_grad``) and forms the real one itself"""

    @staticmethod
    def forward(ctx, prob, target, run):
        loss = torch.empty((), dtype=torch.float32, device=prob.device)
        placeholder = torch.empty(prob.numel(), dtype=torch.float32, device=prob.device)
        run.deferred = (target, loss, placeholder)
        ctx.shape, ctx.placeholder, ctx.device = prob.shape, placeholder, prob.device
        return loss

    @staticmethod
    def backward(ctx, gloss):
        unit = _units.get(ctx.device.index)
        if unit is None or gloss.data_ptr() != unit.data_ptr():
            raise RuntimeError("a deferred BCELoss takes loss.backward(unit_grad(device)) and nothing else: the model's "
                               "backward forms the gradient for an upstream of exactly 1")
        return ctx.placeholder.view(ctx.shape), None, None


def _deferrable(input: torch.Tensor, target: torch.Tensor):
    """the flat view of ``target`` the model's backward reads, if this call can be deferred; else None"""
    d = _deferral
    if d is None or d.run is None or not input.requires_grad or not torch.is_grad_enabled():
        return None
    # THE tensor the model returned (or a view of all of it: its gradient arrives at the model as a view of ours)
    if input.data_ptr() != d.prob.data_ptr() or input.numel() != d.prob.numel() or not input.is_contiguous():
        return None
    if not target.is_cuda or target.dtype != torch.float32 or target.numel() != input.numel() or target.requires_grad:
        return None
    flat = target.reshape(-1)
    if flat.numel() > 1 and flat.untyped_storage().data_ptr() != target.untyped_storage().data_ptr():
        return None      # reshape had to copy: a replay would read the copy's launch, not the caller's buffer -- today's path
    return flat


class BCELoss(torch.nn.Module):
    """``BCELoss()(prob, target)`` -> scalar mean loss, like ``torch.nn.BCELoss()``"""

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if _deferral is not None and type(self) is BCELoss:
            flat = _deferrable(input, target)
            if flat is not None:
                run, _deferral.run, _deferral.prob = _deferral.run, None, None
                return _DeferredBCEFunction.apply(input, flat, run)
        return _BCEFunction.apply(input, target)


class _GroupLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, negatives, kind, logq):
        _lib.require_device(prob, logq)
        p = prob.reshape(-1)
        if p.dtype != torch.float32 or p.numel() == 0 or p.numel() % (1 + negatives):
            raise ValueError(f"the group loss expects float32 input of whole groups of 1 + {negatives} samples")
        q = None if logq is None else logq.detach().reshape(-1)
        if q is not None and (q.dtype != torch.float32 or q.numel() != p.numel()):
            raise ValueError("the group loss expects a float32 log_q of one value per sample")
        groups = p.numel() // (1 + negatives)
        loss = torch.empty((), dtype=torch.float32, device=prob.device)
        ws = torch.empty(256, dtype=torch.float32, device=prob.device)
        # d loss / d prob for an upstream gradient of exactly 1, written by the same launch
        gp1 = torch.empty(p.numel(), dtype=torch.float32, device=prob.device) if ctx.needs_input_grad[0] else None
        if q is None:
            rc = _lib.load().ctr_group_loss_fwd(p.data_ptr(), p.stride(0) if p.numel() > 1 else 1, groups, negatives, kind,
                                                loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _ticket(prob.device).data_ptr(), _lib.ptr(gp1), _lib.stream_ptr())
            _lib.check(rc, "ctr_group_loss_fwd")
        else:
            rc = _lib.load().ctr_group_loss_logq_fwd(p.data_ptr(), p.stride(0) if p.numel() > 1 else 1, groups, negatives,
                                                     kind, loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                                     _ticket(prob.device).data_ptr(), _lib.ptr(gp1), q.data_ptr(),
                                                     q.stride(0) if q.numel() > 1 else 1, _lib.stream_ptr())
            _lib.check(rc, "ctr_group_loss_logq_fwd")
        ctx.save_for_backward(p)
        ctx.shape, ctx.negatives, ctx.kind, ctx.gp1, ctx.logq = prob.shape, negatives, kind, gp1, q
        return loss

    @staticmethod
    def backward(ctx, gloss):
        p, = ctx.saved_tensors
        unit = _units.get(p.device.index)
        if ctx.gp1 is not None and unit is not None and gloss.data_ptr() == unit.data_ptr():
            return ctx.gp1.view(ctx.shape), None, None, None  # upstream gradient is THE 1.0: forward wrote this already
        gp = torch.empty(p.numel(), dtype=torch.float32, device=p.device)
        g = gloss.contiguous()
        q = ctx.logq
        if q is None:
            rc = _lib.load().ctr_group_loss_bwd(p.data_ptr(), p.stride(0) if p.numel() > 1 else 1,
                                                p.numel() // (1 + ctx.negatives), ctx.negatives, ctx.kind, g.data_ptr(),
                                                gp.data_ptr(), 1, _lib.stream_ptr())
            _lib.check(rc, "ctr_group_loss_bwd")
        else:
            rc = _lib.load().ctr_group_loss_logq_bwd(p.data_ptr(), p.stride(0) if p.numel() > 1 else 1,
                                                     p.numel() // (1 + ctx.negatives), ctx.negatives, ctx.kind,
                                                     g.data_ptr(), gp.data_ptr(), 1, q.data_ptr(),
                                                     q.stride(0) if q.numel() > 1 else 1, _lib.stream_ptr())
            _lib.check(rc, "ctr_group_loss_logq_bwd")
        return gp.view(ctx.shape), None, None, None


class _GroupLoss(torch.nn.Module):
    """``loss_fn(input, target)`` over groups of ``group_size`` contiguous samples, slot 0 the positive; ``target`` is
    accepted, so that ``Trainer`` and ``GraphedStep`` drive the loss like ``BCELoss``, and not read: the position
    inside the group says which sample is the positive"""
    kind = None

    def __init__(self, negatives: int):
        super().__init__()
        self.negatives = int(negatives)
        if not 1 <= self.negatives <= _lib.CTR_GROUP_MAX_K:
            raise ValueError(f"negatives must be in [1, {_lib.CTR_GROUP_MAX_K}]")
        self.group_size = 1 + self.negatives

    def forward(self, input: torch.Tensor, target: torch.Tensor = None) -> torch.Tensor:
        return _GroupLossFunction.apply(input, self.negatives, self.kind, None)


class BPRLoss(_GroupLoss):
    """Bayesian personalised ranking: mean over the (positive, negative) pairs of ``softplus(z_neg - z_pos)``, i.e.
    ``-logsigmoid(z_pos - z_neg)``, z the logit of the model's probability"""
    kind = 0


class SampledSoftmaxLoss(_GroupLoss):
    """sampled softmax: mean over the groups of the cross entropy of the group's logits against slot 0.

    ``log_q``: the logQ correction for negatives that are not drawn uniformly (header comment of csrc/group_loss.hip):
    every sample's logit is lowered by ``log q(its item)`` before the softmax.  Either a ``data.DeviceLoader`` built with
    ``item_sampler`` -- the loss then reads ``loader.log_q_of(target)``, the static column the loader refills, so a
    captured step stays valid -- or a float32 device tensor of one value per sample.  With a loader, a ``target`` that is
    not one of its rating buffers is a ValueError; except under ``torch.no_grad()``, where it is an evaluation batch
    (``Trainer.rank_epoch`` on held-out candidates, which are drawn uniformly) and gets the uncorrected loss, the right
    form for a uniform q."""
    kind = 1

    def __init__(self, negatives: int, log_q=None):
        super().__init__(negatives)
        if log_q is not None and not torch.is_tensor(log_q) and not hasattr(log_q, "log_q_of"):
            raise ValueError("SampledSoftmaxLoss: log_q is a DeviceLoader built with item_sampler, or a float32 tensor")
        self.log_q = log_q

    def forward(self, input: torch.Tensor, target: torch.Tensor = None) -> torch.Tensor:
        log_q = self.log_q
        if log_q is not None and not torch.is_tensor(log_q):
            try:
                log_q = log_q.log_q_of(target)
            except ValueError:
                if torch.is_grad_enabled() or log_q._sampler is None:
                    raise
                log_q = None
        return _GroupLossFunction.apply(input, self.negatives, self.kind, log_q)
