"""Wide & Deep -- counterpart of the reference's model/widedeep.py:8-79."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops
from ..ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, Layer
from ._base import CatalogueScorer, FeatureModel, Params, SixFieldGridScorer
from .deepcrossing import DeepCrossing


class WideDeep(FeatureModel):
    """``WideDeep(num_users, num_items, hidden_units, embedding_dim)``; ``forward(x: (B,45)) -> (B,1)``.

    Deep part: the (B, 5E+1) stack of Deep Crossing -> ``linear`` (no activation,
    widedeep.py:55) -> Linear+ReLU per pair.  Wide part: ``user(u) + item(i) + wide(x[:,2:])``
    from the DeepFM wide kernel run with a single vector, whose FM term ``(v)^2 - v^2`` is
    identically zero.  Both write the columns of the (B, 1+H_last) operand of ``output``."""

    def __init__(self, num_users, num_items, hidden_units, embedding_dim):
        super().__init__()
        self.user_embedding = nn.Embedding(num_users, embedding_dim)
        self.item_embedding = nn.Embedding(num_items, embedding_dim)
        self.gender_embedding = nn.Embedding(2, embedding_dim)
        self.occupation_embedding = nn.Embedding(21, embedding_dim)
        self.movie_embedding = nn.Embedding(19, embedding_dim)
        self.linear = nn.Linear(embedding_dim * 5 + 1, hidden_units[0])
        self.dnn_network = nn.ModuleList([nn.Linear(a, b) for a, b in zip(hidden_units[:-1], hidden_units[1:])])
        self.relu = nn.ReLU()
        self.user = nn.Embedding(num_users, 1)
        self.item = nn.Embedding(num_items, 1)
        self.wide = nn.Linear(1 + 2 + 21 + 19, 1)
        self.output = nn.Linear(2, 1)
        for emb in (self.user_embedding, self.item_embedding, self.gender_embedding, self.occupation_embedding,
                    self.movie_embedding, self.user, self.item):
            xavier_normal_(emb.weight.data)

    def _params(self):
        """``deep``: ``linear`` without activation, then Linear+ReLU"""
        return Params(tables=[e.weight for e in (self.user_embedding, self.item_embedding, self.gender_embedding,
                                                 self.occupation_embedding, self.movie_embedding)],
                      user1=self.user.weight, item1=self.item.weight, wide_w=self.wide.weight, wide_b=self.wide.bias,
                      out_w=self.output.weight, out_b=self.output.bias,
                      deep=[Layer(self.linear.weight, self.linear.bias, ACT_NONE)]
                      + [Layer(lin.weight, lin.bias, ACT_RELU) for lin in self.dnn_network])

    def forward(self, x):
        return self._run_model(x, self._params())

    def run_forward(self, inputs, p):
        (x,) = inputs
        batch, e = x.shape[0], self.user_embedding.embedding_dim
        d, dev = 5 * e + 1, x.device
        stack = self._padded_rows(batch, d, dev)
        ops.embed_fwd(DeepCrossing._specs(p.tables, e), x, batch, stack, self._flag)
        *_, last = p.deep
        comb = torch.empty((batch, 1 + last.weight.shape[0]), dtype=torch.float32, device=dev)
        hs = [stack]
        for k, layer in enumerate(p.deep):
            out = comb[:, 1:] if k == len(p.deep) - 1 else None
            w = self._aligned_weight(layer.weight) if k == 0 else layer.weight
            hs.append(ops.linear_fwd(hs[-1], w, layer.bias, layer.act, out=out))
        ops.fm_wide_fwd(stack[:, :e], 1, e, x, p.user1, p.item1, p.wide_w, p.wide_b, comb[:, 0:1], self._flag)
        prob = ops.linear_fwd(comb, p.out_w, p.out_b, ACT_SIGMOID)
        return prob, (hs, comb, prob)

    def run_backward(self, state, inputs, p, gprob, zeros):
        (x,) = inputs
        hs, comb, prob = state
        batch, e = x.shape[0], self.user_embedding.embedding_dim
        dev = x.device
        gcomb = torch.empty_like(comb)
        ops.linear_bwd(comb, p.out_w, prob, gprob, ACT_SIGMOID, gcomb, zeros[id(p.out_w)], zeros[id(p.out_b)])
        gh = gcomb[:, 1:]
        for k, layer in reversed(list(enumerate(p.deep))):
            gin = self._padded_rows(batch, hs[k].shape[1], dev)
            w = self._aligned_weight(layer.weight, refresh=False) if k == 0 else layer.weight
            ops.linear_bwd(hs[k], w, hs[k + 1], gh, layer.act, gin, zeros[id(layer.weight)], zeros[id(layer.bias)])
            gh = gin
        ops.fm_wide_bwd(hs[0][:, :e], 1, e, x, p.user1, p.item1, p.wide_w, p.wide_b, gcomb[:, 0:1], zeros[id(p.user1)],
                        zeros[id(p.item1)], zeros[id(p.wide_w)], zeros[id(p.wide_b)], None, accumulate=False)
        ops.embed_bwd(DeepCrossing._specs(p.tables, e), x, batch, gh, zeros)

    def recommendation(self, num_users, user_item, k):
        return self._rank_users(num_users, user_item, k)

    def catalogue_scorer(self, assembler):
        """as ``FeatureModel.catalogue_scorer``; where ``grid_path`` says "grid" the scores come from
        ``ctr_widedeep_grid_scores`` over table rows made once per call, not from the per-sample forward"""
        hidden = [self.linear.out_features] + [lin.out_features for lin in self.dnn_network]
        return (_GridScorer if grid_path(hidden) == "grid" else CatalogueScorer)(self, assembler)


def grid_path(hidden_units) -> str:
    """how a ``catalogue_scorer`` scores a Wide & Deep of these ``hidden_units`` (any embedding width): "grid" --
    user-side and item-side table rows, then ``ctr_widedeep_grid_scores`` -- where the library has that kernel, else
    "forward": the per-sample forward over feature rows assembled chunk by chunk.  A function of the shape alone."""
    return "grid" if ops.widedeep_grid_supported(hidden_units) else "forward"


class _GridScorer(SixFieldGridScorer):
    """Wide & Deep on the user x item grid.  Every column of the (5E + 1) stack belongs to the user (user, age, gender,
    occupation) or to the item (item, movie) and ``linear`` has no activation, so
        h1 = relu(ZU[u] + ZI[i]),   ZU / ZI = W1 (W0 . a side's columns of the stack),   wide = a[u] + b[i]
    with every bias on the item side; the rest of the model runs per pair inside the kernel."""

    def _field_specs(self, p, dim, dev):
        return DeepCrossing._specs([t.detach() for t in p.tables], dim)

    def _stage(self, rows, dim, dev):
        return FeatureModel._padded_rows(rows, 5 * dim + 1, dev), None

    def _zero_other(self, stack, user_side):
        e = (stack.shape[1] - 1) // 5                              # [user | item | age | gender | occupation | movie]
        if user_side:
            stack[:, e:2 * e] = 0.0
            stack[:, 4 * e + 1:] = 0.0
        else:
            stack[:, :e] = 0.0
            stack[:, 2 * e:4 * e + 1] = 0.0

    def _side_prepare(self, p):
        # the first layer's rows are 5E + 1 floats long: the GEMM reads a copy padded to 16-byte rows, as the forward
        # does (made here, at every public call: the model's own copy belongs to its training step)
        w0 = p.deep[0].weight.detach()
        self._w0 = FeatureModel._padded_rows(w0.shape[0], w0.shape[1], w0.device)
        self._w0.copy_(w0)

    def _side_buffers(self, p, rows, dim, user_side, dev):
        """(Z (R, 256), first-order + wide term (R,)) of every row of one side's table"""
        return (torch.empty((rows, p.deep[1].weight.shape[0]), dtype=torch.float32, device=dev),
                torch.empty(rows, dtype=torch.float32, device=dev))

    def _side_rows(self, p, x, stack, vec, lo, hi, user_side, buffers):
        z, c = buffers
        w0, w1 = p.deep[0], p.deep[1]
        wide = p.wide_w.detach().reshape(-1)
        if user_side:
            c[lo:hi] = p.user1.detach()[lo:hi, 0] + (x[:, 2:26] * wide[:24]).sum(1)
        else:
            c[lo:hi] = p.item1.detach()[lo:hi, 0] + (x[:, 26:45] * wide[24:]).sum(1) + p.wide_b.detach()
        self._zero_other(stack, user_side)
        t = ops.linear_fwd(stack, self._w0, None if user_side else w0.bias.detach())
        ops.linear_fwd(t, w1.weight.detach(), None if user_side else w1.bias.detach(), out=z[lo:hi])

    def _grid_scores(self, shared, users, user0, rows):
        p, (zu, a), (zi, b) = shared
        w2, w3 = p.deep[2], p.deep[3]
        return ops.widedeep_grid_scores(zu, zi, a, b, w2.weight.detach(), w2.bias, w3.weight, w3.bias, p.out_w, p.out_b,
                                        users=users, user0=user0, rows=rows, row_blocks=self.row_blocks)
