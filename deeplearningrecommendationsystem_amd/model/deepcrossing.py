"""Deep Crossing -- counterpart of the reference's model/deepcrossing.py:8-92."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops
from ..ops import ACT_RELU, ACT_SIGMOID, FieldSpec, Layer
from .._lib import FIELD_BAG, FIELD_DENSE, FIELD_ID_F32
from ._base import FeatureModel, Params


class ResidualBlock(nn.Module):
    """parameter container of one residual unit ``relu(linear2(relu(linear1(x))) + x)``
    (reference model/deepcrossing.py:8-27)"""

    def __init__(self, hidden_unit, dim_stack):
        super().__init__()
        self.linear1 = nn.Linear(dim_stack, hidden_unit)
        self.linear2 = nn.Linear(hidden_unit, dim_stack)
        self.relu = nn.ReLU()


class DeepCrossing(FeatureModel):
    """``DeepCrossing(num_user, num_item, num_feature, hidden_units)``;
    ``forward(x: (B,45)) -> (B,1)``.  The stacking layer
    [user, item, age(1), gender, occupation, movie] is one embedding-stage launch
    into a (B, 5E+1) buffer whose rows are padded to a multiple of 4 floats; every
    residual add + ReLU is the epilogue of the block's second GEMM."""

    def __init__(self, num_user, num_item, num_feature, hidden_units):
        super().__init__()
        self.user_embedding = nn.Embedding(num_user, num_feature)
        self.item_embedding = nn.Embedding(num_item, num_feature)
        self.gender_embedding = nn.Embedding(2, num_feature)
        self.occupation_embedding = nn.Embedding(21, num_feature)
        self.movie_embedding = nn.Embedding(19, num_feature)
        for emb in (self.user_embedding, self.item_embedding, self.gender_embedding, self.occupation_embedding,
                    self.movie_embedding):
            xavier_normal_(emb.weight.data)
        dim_stack = num_feature * 5 + 1
        self.res_layers = nn.ModuleList([ResidualBlock(unit, dim_stack) for unit in hidden_units])
        self.linear = nn.Linear(dim_stack, 1)

    def _params(self):
        """``res``: one [linear1, linear2] pair per residual block"""
        return Params(tables=[e.weight for e in (self.user_embedding, self.item_embedding, self.gender_embedding,
                                                 self.occupation_embedding, self.movie_embedding)],
                      lin_w=self.linear.weight, lin_b=self.linear.bias,
                      res=[[Layer(lin.weight, lin.bias, ACT_RELU) for lin in (blk.linear1, blk.linear2)]
                           for blk in self.res_layers])

    def forward(self, feature_vector):
        return self._run_model(feature_vector, self._params())

    @staticmethod
    def _specs(tables, e):
        user, item, gender, occ, movie = tables
        return [
            FieldSpec(FIELD_ID_F32, e, 0, table=user, src_col=0),
            FieldSpec(FIELD_ID_F32, e, e, table=item, src_col=1),
            FieldSpec(FIELD_DENSE, 1, 2 * e, src_col=2),
            FieldSpec(FIELD_BAG, e, 2 * e + 1, table=gender, src_col=3, bag_size=2),
            FieldSpec(FIELD_BAG, e, 3 * e + 1, table=occ, src_col=5, bag_size=21),
            FieldSpec(FIELD_BAG, e, 4 * e + 1, table=movie, src_col=26, bag_size=19),
        ]

    @staticmethod
    def _stack_buffer(batch, width, device):
        padded = (width + 3) // 4 * 4
        return torch.empty((batch, padded), dtype=torch.float32, device=device)[:, :width]

    def run_forward(self, inputs, p):
        (x,) = inputs
        batch, e = x.shape[0], self.user_embedding.embedding_dim
        width = 5 * e + 1
        r = self._stack_buffer(batch, width, x.device)
        ops.embed_fwd(self._specs(p.tables, e), x, batch, r, self._flag)
        rs, hs = [r], []
        for lin1, lin2 in p.res:
            h = ops.linear_fwd(rs[-1], self._aligned_weight(lin1.weight), lin1.bias, ACT_RELU)
            out = self._stack_buffer(batch, width, x.device)
            ops.linear_fwd(h, lin2.weight, lin2.bias, ACT_RELU, out=out, residual=rs[-1])
            hs.append(h)
            rs.append(out)
        prob = ops.linear_fwd(rs[-1], self._aligned_weight(p.lin_w), p.lin_b, ACT_SIGMOID)
        return prob, (rs, hs, prob)

    def run_backward(self, state, inputs, p, gprob, zeros):
        (x,) = inputs
        rs, hs, prob = state
        batch, e = x.shape[0], self.user_embedding.embedding_dim
        width = 5 * e + 1
        gr = self._stack_buffer(batch, width, x.device)
        ops.linear_bwd(rs[-1], self._aligned_weight(p.lin_w, refresh=False), prob, gprob, ACT_SIGMOID, gr,
                       zeros[id(p.lin_w)], zeros[id(p.lin_b)])
        for k, (lin1, lin2) in reversed(list(enumerate(p.res))):
            r_in, r_out, h = rs[k], rs[k + 1], hs[k]
            gh = torch.empty_like(h)
            ops.linear_bwd(h, lin2.weight, r_out, gr, ACT_RELU, gh, zeros[id(lin2.weight)],
                           zeros[id(lin2.bias)])                                # through relu(linear2(h)+r)
            gr_in = self._stack_buffer(batch, width, x.device)
            ops.linear_bwd(r_in, self._aligned_weight(lin1.weight, refresh=False), h, gh, ACT_RELU, gr_in,
                           zeros[id(lin1.weight)], zeros[id(lin1.bias)])        # relu(linear1(r))
            ops.act_bwd(r_out, gr, ACT_RELU, gr_in, accumulate=True)            # the skip connection
            gr = gr_in
        ops.embed_bwd(self._specs(p.tables, e), x, batch, gr, zeros)

    def recommendation(self, num_users, user_item, k):
        return self._rank_users(num_users, user_item, k)
