"""Logistic regression -- counterpart of the reference's model/lr.py:11-37."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops
from ..ops import ACT_SIGMOID
from ._base import CatalogueScorer, FeatureModel, Params


class LogisticRegression(FeatureModel):
    """``LogisticRegression(num_users, num_items, num_feature)``; ``forward(x: (B,45)) -> (B,1)``:
    ``sigmoid(user(u) + item(i) + linear(x[:,2:]))`` (lr.py:24-25) -- the wide kernel of DeepFM
    (run on one all-zero vector, so that its FM term vanishes) followed by the sigmoid."""

    def __init__(self, num_users, num_items, num_feature: int):
        super().__init__()
        self.user = nn.Embedding(num_users, 1)
        self.item = nn.Embedding(num_items, 1)
        self.linear = nn.Linear(num_feature, 1, True)
        xavier_normal_(self.user.weight.data)
        xavier_normal_(self.item.weight.data)

    def _params(self):
        return Params(user1=self.user.weight, item1=self.item.weight, w=self.linear.weight, b=self.linear.bias)

    def forward(self, feature_vector):
        return self._run_model(feature_vector, self._params())

    @staticmethod
    def _unit(device):
        return torch.ones((1, 1), dtype=torch.float32, device=device)

    def run_forward(self, inputs, p):
        (x,) = inputs
        batch, dev = x.shape[0], x.device
        none = torch.zeros((batch, 4), dtype=torch.float32, device=dev)   # the "FM vectors": one zero vector
        logit = torch.empty((batch, 1), dtype=torch.float32, device=dev)
        ops.fm_wide_fwd(none, 1, 4, x, p.user1, p.item1, p.w, p.b, logit, self._flag)
        prob = ops.linear_fwd(logit, self._unit(dev), None, ACT_SIGMOID)   # sigmoid(1 * logit)
        return prob, (none, logit, prob)

    def run_backward(self, state, inputs, p, gprob, zeros):
        (x,) = inputs
        none, logit, prob = state
        glogit = torch.empty_like(logit)
        ops.linear_bwd(logit, self._unit(x.device), prob, gprob, ACT_SIGMOID, glogit, None, None)
        ops.fm_wide_bwd(none, 1, 4, x, p.user1, p.item1, p.w, p.b, glogit, zeros[id(p.user1)], zeros[id(p.item1)],
                        zeros[id(p.w)], zeros[id(p.b)], None, accumulate=False)

    def recommendation(self, num_users, user_item, k):
        return self._rank_users(num_users, user_item, k)

    def catalogue_scorer(self, assembler):
        """as ``FeatureModel.catalogue_scorer``; the scores come from the rank-0 arm of ``ctr_lowrank_grid_scores`` over
        one bias per user and one per item, made once per call, not from the per-sample forward"""
        return _GridScorer(self, assembler)


def grid_path() -> str:
    """how a ``catalogue_scorer`` scores a LogisticRegression: always "grid" (the model has no shape to refuse)"""
    return "grid"


class _GridScorer(CatalogueScorer):
    """LogisticRegression on the user x item grid: ``sigmoid(a[u] + b[i])`` with
        a = user(u) + w[:24] . x_u + bias,   b = item(i) + w[24:] . x_i
    both made for the whole tables at every public call, so a table row's bits do not depend on the users asked for."""

    path = "grid"
    row_blocks = 0               # 0: the launch's own geometry (tests set 1, 2 to reach the tile loop at small shapes)

    def _shared(self):
        p, asm = self.model._params(), self.assembler
        self.model._need_device(p.user1, asm.user_features)
        w = p.w.detach().reshape(-1)
        a = p.user1.detach()[:, 0] + (asm.user_features * w[:24]).sum(1) + p.b.detach()
        b = p.item1.detach()[:, 0] + (asm.item_features * w[24:]).sum(1)
        return a, b

    def _scores(self, users, start, stop, shared=None):
        rows = users.numel() if users is not None else stop - start
        if rows == 0:
            return torch.empty((0, self.num_items), dtype=torch.float32, device=self.device)
        a, b = shared
        return ops.lowrank_grid_scores(None, None, a, b, users=users, user0=start, rows=rows,
                                       row_blocks=self.row_blocks)
