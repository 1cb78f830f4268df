"""Deep & Cross (DCN) -- counterpart of the reference's model/deepcross.py:7-89."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops
from ..ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, Layer
from ._base import FeatureModel, Params
from .deepcrossing import DeepCrossing


class CrossNetwork(nn.Module):
    """parameter container of the cross layers ``x_{l+1} = x0 * (W_l x_l) + b_l + x_l``
    (reference model/deepcross.py:7-18)"""

    def __init__(self, input_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        self.cross_weights = nn.ModuleList([nn.Linear(input_dim, input_dim, bias=False) for _ in range(num_layers)])
        self.cross_biases = nn.ParameterList([nn.Parameter(torch.zeros(input_dim)) for _ in range(num_layers)])


class DeepNetwork(nn.Module):
    """parameter container of the deep tower: Linear + ReLU after EVERY layer
    (reference model/deepcross.py:21-31)"""

    def __init__(self, input_dim, hidden_units):
        super().__init__()
        layers = []
        for a, b in zip([input_dim] + hidden_units[:-1], hidden_units):
            layers += [nn.Linear(a, b), nn.ReLU()]
        self.network = nn.Sequential(*layers)


class DeepCross(FeatureModel):
    """``DeepCross(num_users, num_items, cross_layers, deep_hidden_units, embedding_dim)``;
    ``forward(x: (B,45)) -> (B,1)``.

    One embedding-stage launch builds the (B, 5E+1) stack; every cross layer is a d x d GEMM
    on the matrix cores plus one streaming combine kernel (csrc/cross.hip); the last cross
    output and the last deep activation are written side by side into the operand of the
    output layer (no torch.cat)."""

    def __init__(self, num_users, num_items, cross_layers, deep_hidden_units, embedding_dim):
        super().__init__()
        self.user_embedding = nn.Embedding(num_users, embedding_dim)
        self.item_embedding = nn.Embedding(num_items, embedding_dim)
        self.gender_embedding = nn.Embedding(2, embedding_dim)
        self.occupation_embedding = nn.Embedding(21, embedding_dim)
        self.movie_embedding = nn.Embedding(19, embedding_dim)
        d = embedding_dim * 5 + 1
        self.cross_network = CrossNetwork(d, cross_layers)
        self.deep_network = DeepNetwork(d, list(deep_hidden_units))
        self.output_layer = nn.Linear(d + deep_hidden_units[-1], 1)
        for emb in (self.user_embedding, self.item_embedding, self.gender_embedding, self.occupation_embedding,
                    self.movie_embedding):
            xavier_normal_(emb.weight.data)

    def _params(self):
        return Params(tables=[e.weight for e in (self.user_embedding, self.item_embedding, self.gender_embedding,
                                                 self.occupation_embedding, self.movie_embedding)],
                      cw=[lin.weight for lin in self.cross_network.cross_weights],
                      cb=list(self.cross_network.cross_biases),
                      deep=[Layer(m.weight, m.bias, ACT_RELU) for m in self.deep_network.network
                            if isinstance(m, nn.Linear)],
                      out_w=self.output_layer.weight, out_b=self.output_layer.bias)

    def forward(self, x):
        return self._run_model(x, self._params())

    def run_forward(self, inputs, p):
        (x,) = inputs
        batch, e = x.shape[0], self.user_embedding.embedding_dim
        d, dev = 5 * e + 1, x.device
        x0 = self._padded_rows(batch, d, dev)
        ops.embed_fwd(DeepCrossing._specs(p.tables, e), x, batch, x0, self._flag)
        *_, last = p.deep
        comb = self._padded_rows(batch, d + last.weight.shape[0], dev)   # [x_L | deep_out]: operand of the output layer
        xs, us = [x0], []
        for l, (w, b) in enumerate(zip(p.cw, p.cb)):
            u = ops.linear_fwd(xs[-1], self._aligned_weight(w), None, ACT_NONE, out=self._padded_rows(batch, d, dev))
            out = comb[:, :d] if l == len(p.cw) - 1 else self._padded_rows(batch, d, dev)
            ops.cross_fwd(x0, u, xs[-1], b, out)
            us.append(u)
            xs.append(out)
        if not p.cw:
            comb[:, :d].copy_(x0)
        hs = [x0]
        for k, layer in enumerate(p.deep):
            out = comb[:, d:] if k == len(p.deep) - 1 else None
            w = self._aligned_weight(layer.weight) if k == 0 else layer.weight
            hs.append(ops.linear_fwd(hs[-1], w, layer.bias, ACT_RELU, out=out))
        prob = ops.linear_fwd(comb, self._aligned_weight(p.out_w), p.out_b, ACT_SIGMOID)
        return prob, (xs, us, hs, comb, prob)

    def run_backward(self, state, inputs, p, gprob, zeros):
        (x,) = inputs
        xs, us, hs, comb, prob = state
        batch, e = x.shape[0], self.user_embedding.embedding_dim
        d, dev = 5 * e + 1, x.device
        gcomb = self._padded_rows(batch, comb.shape[1], dev)
        ops.linear_bwd(comb, self._aligned_weight(p.out_w, refresh=False), prob, gprob, ACT_SIGMOID, gcomb,
                       zeros[id(p.out_w)], zeros[id(p.out_b)])
        # deep tower: its input gradient starts the accumulator of d loss / d x0
        gh = gcomb[:, d:]
        for k, layer in reversed(list(enumerate(p.deep))):
            gin = self._padded_rows(batch, hs[k].shape[1], dev)
            w = self._aligned_weight(layer.weight, refresh=False) if k == 0 else layer.weight
            ops.linear_bwd(hs[k], w, hs[k + 1], gh, ACT_RELU, gin, zeros[id(layer.weight)], zeros[id(layer.bias)])
            gh = gin
        gx0 = gh
        # cross layers, last to first: gx holds d loss / d x_{l+1}, becomes d loss / d x_l in place
        gx = gcomb[:, :d]
        for l, (w, b) in reversed(list(enumerate(zip(p.cw, p.cb)))):
            gu = self._padded_rows(batch, d, dev)
            ops.cross_bwd(xs[0], us[l], gx, gu, gx0, zeros[id(b)])
            ops.linear_bwd(xs[l], self._aligned_weight(w, refresh=False), None, gu, ACT_NONE, gx, zeros[id(w)],
                           None, accumulate_gx=True)
        ops.act_bwd(gx, gx, ACT_NONE, gx0, accumulate=True)   # x_0 is x0 itself: gx0 += gx
        ops.embed_bwd(DeepCrossing._specs(p.tables, e), x, batch, gx0, zeros)

    def recommendation(self, num_users, user_item, k):
        return self._rank_users(num_users, user_item, k)
