"""NFM -- counterpart of the reference's model/nfm.py:8-84."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops
from ..ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, Layer
from ._base import FeatureModel, Params
from .deepfm import six_field_specs


class NFM(FeatureModel):
    """``NFM(num_users, num_items, hidden_units, embedding_dim)``; ``forward(x: (B,45)) -> (B,1)``.

    The six vectors of DeepFM (one embedding-stage launch) -> bi-interaction pooling
    ``sum_{i<j} f_i * f_j`` (csrc/interact.hip) -> ``linear`` (no activation, nfm.py:62) -> Linear+ReLU
    per pair; wide part from the DeepFM wide kernel on a single vector (FM term identically
    zero); both write the columns of the (B, 1+H_last) operand of ``output``."""

    def __init__(self, num_users, num_items, hidden_units, embedding_dim):
        super().__init__()
        self.user_embedding = nn.Embedding(num_users, embedding_dim)
        self.item_embedding = nn.Embedding(num_items, embedding_dim)
        self.age_embedding = nn.Embedding(1, embedding_dim)
        self.gender_embedding = nn.Embedding(2, embedding_dim)
        self.occupation_embedding = nn.Embedding(21, embedding_dim)
        self.movie_embedding = nn.Embedding(19, embedding_dim)
        self.linear = nn.Linear(embedding_dim, hidden_units[0])
        self.dnn_network = nn.ModuleList([nn.Linear(a, b) for a, b in zip(hidden_units[:-1], hidden_units[1:])])
        self.relu = nn.ReLU()
        self.user = nn.Embedding(num_users, 1)
        self.item = nn.Embedding(num_items, 1)
        self.wide = nn.Linear(1 + 2 + 21 + 19, 1)
        self.output = nn.Linear(2, 1)
        for emb in (self.user_embedding, self.item_embedding, self.age_embedding, self.gender_embedding,
                    self.occupation_embedding, self.movie_embedding, self.user, self.item):
            xavier_normal_(emb.weight.data)

    def _params(self):
        """``deep``: ``linear`` without activation, then Linear+ReLU"""
        return Params(tables=[e.weight for e in (self.user_embedding, self.item_embedding, self.age_embedding,
                                                 self.gender_embedding, self.occupation_embedding,
                                                 self.movie_embedding)],
                      user1=self.user.weight, item1=self.item.weight, wide_w=self.wide.weight, wide_b=self.wide.bias,
                      out_w=self.output.weight, out_b=self.output.bias,
                      deep=[Layer(self.linear.weight, self.linear.bias, ACT_NONE)]
                      + [Layer(lin.weight, lin.bias, ACT_RELU) for lin in self.dnn_network])

    def forward(self, x):
        return self._run_model(x, self._params())

    def run_forward(self, inputs, p):
        (x,) = inputs
        batch, e, dev = x.shape[0], self.user_embedding.embedding_dim, x.device
        emb = torch.empty((batch, 6 * e), dtype=torch.float32, device=dev)
        ops.embed_fwd(six_field_specs(p.tables, e), x, batch, emb, self._flag)
        cross = self._padded_rows(batch, e, dev)
        ops.biinteract_fwd(emb, 6, e, cross)
        *_, last = p.deep
        comb = torch.empty((batch, 1 + last.weight.shape[0]), dtype=torch.float32, device=dev)
        hs = [cross]
        for k, layer in enumerate(p.deep):
            out = comb[:, 1:] if k == len(p.deep) - 1 else None
            w = self._aligned_weight(layer.weight) if k == 0 else layer.weight
            hs.append(ops.linear_fwd(hs[-1], w, layer.bias, layer.act, out=out))
        ops.fm_wide_fwd(emb[:, :e], 1, e, x, p.user1, p.item1, p.wide_w, p.wide_b, comb[:, 0:1], self._flag)
        prob = ops.linear_fwd(comb, p.out_w, p.out_b, ACT_SIGMOID)
        return prob, (emb, hs, comb, prob)

    def run_backward(self, state, inputs, p, gprob, zeros):
        (x,) = inputs
        emb, hs, comb, prob = state
        batch, e, dev = x.shape[0], self.user_embedding.embedding_dim, x.device
        gcomb = torch.empty_like(comb)
        ops.linear_bwd(comb, p.out_w, prob, gprob, ACT_SIGMOID, gcomb, zeros[id(p.out_w)], zeros[id(p.out_b)])
        gh = gcomb[:, 1:]
        for k, layer in reversed(list(enumerate(p.deep))):
            gin = self._padded_rows(batch, hs[k].shape[1], dev)
            w = self._aligned_weight(layer.weight, refresh=False) if k == 0 else layer.weight
            ops.linear_bwd(hs[k], w, hs[k + 1], gh, layer.act, gin, zeros[id(layer.weight)], zeros[id(layer.bias)])
            gh = gin
        gemb = torch.empty_like(emb)
        ops.biinteract_bwd(emb, 6, e, gh, gemb, accumulate=False)
        ops.fm_wide_bwd(emb[:, :e], 1, e, x, p.user1, p.item1, p.wide_w, p.wide_b, gcomb[:, 0:1], zeros[id(p.user1)],
                        zeros[id(p.item1)], zeros[id(p.wide_w)], zeros[id(p.wide_b)], None, accumulate=False)
        ops.embed_bwd(six_field_specs(p.tables, e), x, batch, gemb, zeros)

    def recommendation(self, num_users, user_item, k):
        return self._rank_users(num_users, user_item, k)
