"""PNN -- counterpart of the reference's model/pnn.py:8-143 (DNN, ProductLayers, PNN)."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops
from ..ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, Layer
from ._base import _USER_FIELDS, CatalogueScorer, FeatureModel, Params, SixFieldGridScorer, six_field_specs
from .deepfm import FieldsInput, field_vocabs
from .._lib import FIELD_ID_I64


class DNN(nn.Module):
    """parameter container for ``Linear+ReLU`` per consecutive pair of
    ``hidden_units`` (reference model/pnn.py:8-23); the math runs in PNN's
    fused forward/backward."""

    def __init__(self, hidden_units):
        super().__init__()
        self.dnn_network = nn.ModuleList([nn.Linear(a, b) for a, b in zip(hidden_units[:-1], hidden_units[1:])])
        self.relu = nn.ReLU()


class ProductLayers(nn.Module):
    """parameter container of the product layer (reference model/pnn.py:27-79)"""

    def __init__(self, num_feature, embed_dim, hidden_units, model="in"):
        super().__init__()
        self.model = model
        self.linear1 = nn.Linear(num_feature * embed_dim, hidden_units[0])
        if model == "in":
            self.linear2 = nn.Linear(int(num_feature * (num_feature - 1) / 2), hidden_units[0])
        elif model == "out":
            self.linear2 = nn.Linear(embed_dim, hidden_units[0])


class PNN(FeatureModel):
    """``PNN(embed_dim, hidden_units, model="in")``; ``forward(x: (B,45)) -> (B,1)``.

    inner mode: h0 = linear1(emb) + linear2(allpairs(emb)); the second GEMM takes
    the first one's output as its fused residual.  outer mode (reference
    pnn.py:67-72) reduces over the batch and only broadcasts when B == embed_dim;
    it is built from the same GEMM kernels (p = S^T S is the dW form)."""

    def __init__(self, embed_dim, hidden_units, model="in", *, num_users=943, num_items=1682, num_fields=None,
                 vocab=None):
        """keyword-only generalisation (BASELINE configs[2], "26 fields x 1e6 vocab"; the reference hard-codes six
        fields, pnn.py:87-92): ``num_fields=F, vocab=V`` builds F single-id fields ``embeddings.f`` (V, E) and
        ``forward(x: (B,F) ids)``; the product layer then has F(F-1)/2 inner products (325 at F = 26).  Inner
        mode only.  Defaults leave the reference model unchanged."""
        super().__init__()
        self.num_fields = num_fields
        if num_fields is not None:
            if model != "in":
                raise ValueError("the N-field generalisation implements the inner-product mode")
            self.vocabs = field_vocabs(num_fields, vocab)
            self.embeddings = nn.ModuleList([nn.Embedding(v, embed_dim) for v in self.vocabs])
            for emb in self.embeddings:
                xavier_normal_(emb.weight.data)
            self.product = ProductLayers(num_fields, embed_dim, hidden_units, model)
            self.dnn = DNN(hidden_units)
            self.output = nn.Linear(hidden_units[-1], 1)
            return
        self.user_embed = nn.Embedding(num_users, embed_dim)
        self.item_embed = nn.Embedding(num_items, embed_dim)
        self.age_embed = nn.Embedding(1, embed_dim)
        self.gender_embed = nn.Embedding(2, embed_dim)
        self.occupation_embed = nn.Embedding(21, embed_dim)
        self.movie_embed = nn.Embedding(19, embed_dim)
        for emb in (self.user_embed, self.item_embed, self.age_embed, self.gender_embed, self.occupation_embed,
                    self.movie_embed):
            xavier_normal_(emb.weight.data)
        self.product = ProductLayers(6, embed_dim, hidden_units, model)
        self.dnn = DNN(hidden_units)
        self.output = nn.Linear(hidden_units[-1], 1)
        if model == "out":
            # constant selector: S = sum_f v_f as one exact GEMM (products with 0/1)
            self.register_buffer("_sum_selector", torch.eye(embed_dim).repeat(1, 6), persistent=False)

    def _params(self):
        """``dnn`` then ``out`` is the stack on top of the product layer"""
        if self.num_fields is not None:
            tables = [e.weight for e in self.embeddings]
        else:
            tables = [e.weight for e in (self.user_embed, self.item_embed, self.age_embed, self.gender_embed,
                                         self.occupation_embed, self.movie_embed)]
        return Params(tables=tables, w1=self.product.linear1.weight, b1=self.product.linear1.bias,
                      w2=self.product.linear2.weight, b2=self.product.linear2.bias,
                      out=Layer(self.output.weight, self.output.bias, ACT_SIGMOID),
                      dnn=[Layer(lin.weight, lin.bias, ACT_RELU) for lin in self.dnn.dnn_network])

    def sparse_ids(self, inputs, p):
        """sparse mode: every table of the N-field form, the user and item tables of the six-field one"""
        ids = len(p.tables) if self.num_fields is not None else 2
        return [(t, [] if inputs is None else [inputs[0][:, c]]) for c, t in zip(range(ids), p.tables)]

    def forward(self, x):
        if self.num_fields is not None:
            return self._run([FieldsInput.ids(x, self.num_fields)], self._params())
        return self._run_model(x, self._params())

    def _specs(self, x, tables, dim):
        """the embedding stage's field list: the reference's six fields out of the (B,45) matrix, or F id columns"""
        if self.num_fields is None:
            return six_field_specs(tables, dim), x
        return [ops.FieldSpec(FIELD_ID_I64, dim, f * dim, table=table, idx=x[:, f], idx_stride=x.stride(0))
                for f, table in enumerate(tables)], None

    def run_forward(self, inputs, p):
        (x,) = inputs
        n = len(p.tables)
        npairs = n * (n - 1) // 2
        batch, dim = x.shape[0], self.product.linear1.in_features // n
        emb = torch.empty((batch, n * dim), dtype=torch.float32, device=x.device)
        specs, xin = self._specs(x, p.tables, dim)
        ops.embed_fwd(specs, xin, batch, emb, self._flag)
        if self.product.model == "in":
            prod = ops.allpairs_fwd(emb, n, dim, out=self._padded_rows(batch, npairs, x.device))
            lz = ops.linear_fwd(emb, p.w1, p.b1)
            h0 = ops.linear_fwd(prod, self._aligned_weight(p.w2), p.b2, residual=lz)
            extra = (prod,)
        else:
            if batch != dim:
                raise RuntimeError(f"PNN outer product: lz (1,{batch},H) and lp ({dim},H) only broadcast when "
                                   f"batch == embed_dim (reference model/pnn.py:75-77)")
            s = ops.linear_fwd(emb, self._sum_selector, None)                       # (B,E) = sum_f v_f
            prod = torch.zeros((dim, dim), dtype=torch.float32, device=x.device)
            ops.linear_bwd(s, prod, None, s, ACT_NONE, None, prod, None)           # p = S^T S
            lp = ops.linear_fwd(prod, p.w2, p.b2)                                   # (E,H0)
            h0 = ops.linear_fwd(emb, p.w1, p.b1, residual=lp)
            extra = (prod, s)
        acts = ops.mlp_fwd(h0, p.dnn + [p.out])
        return acts[-1].view(-1, 1), (emb, acts, extra)

    def run_backward(self, state, inputs, p, gprob, zeros):
        (x,) = inputs
        emb, acts, extra = state
        n = len(p.tables)
        npairs = n * (n - 1) // 2
        batch, dim = x.shape[0], emb.shape[1] // n
        _, gh0 = ops.mlp_bwd(acts, p.dnn + [p.out], gprob.view(batch, 1), None, zeros=zeros)
        gw1, gb1, gw2, gb2 = (zeros[id(t)] for t in (p.w1, p.b1, p.w2, p.b2))
        gemb = torch.empty_like(emb)
        ops.linear_bwd(emb, p.w1, None, gh0, ACT_NONE, gemb, gw1, gb1)
        if self.product.model == "in":
            (prod,) = extra
            gprod = self._padded_rows(batch, npairs, x.device)
            ops.linear_bwd(prod, self._aligned_weight(p.w2, refresh=False), None, gh0, ACT_NONE, gprod, gw2, gb2)
            ops.allpairs_bwd(emb, n, dim, gprod, gemb, accumulate=True)
        else:
            prod, s = extra
            gprod = torch.empty_like(prod)
            ops.linear_bwd(prod, p.w2, None, gh0, ACT_NONE, gprod, gw2, gb2)        # glp = gh0 as (E,H0)
            gs = ops.linear_fwd(s, gprod, None)                                     # S gp^T
            ops.linear_bwd(s, gprod, None, s, ACT_NONE, gs, None, None, accumulate_gx=True)   # += S gp
            ops.linear_bwd(emb, self._sum_selector, None, gs, ACT_NONE, gemb, None, None, accumulate_gx=True)
        specs, xin = self._specs(x, p.tables, dim)
        ops.embed_bwd(specs, xin, batch, gemb, zeros)

    def recommendation(self, num_users, user_item, k):
        return self._rank_users(num_users, user_item, k)

    def catalogue_scorer(self, assembler):
        """as ``FeatureModel.catalogue_scorer``; where ``grid_path`` says "grid" the scores come from
        ``ctr_pnn_grid_scores`` over table rows made once per call, not from the per-sample forward"""
        self._table_sizes()                                   # (refuses the num_fields= model)
        hidden = [self.product.linear1.out_features] + [lin.out_features for lin in self.dnn.dnn_network]
        grid = grid_path(hidden, self.user_embed.embedding_dim, self.product.model) == "grid"
        return (_GridScorer if grid else CatalogueScorer)(self, assembler)


def grid_path(hidden_units, embed_dim, model="in") -> str:
    """how a ``catalogue_scorer`` scores a six-field PNN of these shapes: "grid" -- user-side and item-side table
    rows, then ``ctr_pnn_grid_scores`` -- where the library has that kernel, else "forward": the per-sample forward
    over feature rows assembled chunk by chunk.  A function of shapes alone."""
    return "grid" if ops.pnn_grid_supported(hidden_units, embed_dim, model) else "forward"


def _pair_columns():
    """columns of ``allpairs`` (i < j lexicographic over the six fields) by side: (user-only, item-only, cross)"""
    user, item, cross, col = [], [], [], 0
    for i in range(6):
        for j in range(i + 1, 6):
            sides = (i in _USER_FIELDS) + (j in _USER_FIELDS)
            (user if sides == 2 else item if sides == 0 else cross).append(col)
            col += 1
    return user, item, cross


_USER_PAIRS, _ITEM_PAIRS, _CROSS_PAIRS = _pair_columns()     # [1, 2, 3, 9, 10, 12], [8], [0, 4, 5, 6, 7, 11, 13, 14]


class _GridScorer(SixFieldGridScorer):
    """PNN (inner mode) on the user x item grid.  Every field vector belongs to the user or to the item and the
    product layer's output h0 has no activation in front of the first DNN layer D1, so
        z1 = D1 h0 + c1 = ZU[u] + ZI[i] + G d(u, i),   G = D1 W2[:, cross columns],   d: the eight cross products
    with ZU / ZI = D1 applied to a side's part of h0 (its columns of ``linear1``, its own products through ``linear2``;
    every bias on the item side), and the rest of the model runs per pair inside the kernel, which forms ``d`` from
    the sides' field vectors FU (U, 4E) / FI (I, 2E)."""

    side_chunk = 1 << 15         # the pass also holds (rows, 16) products and (rows, 256) twice

    def _side_prepare(self, p):
        self.model._aligned_weight(p.w2)                     # ``linear2``'s padded copy, refreshed for ``_side_rows``

    def _side_buffers(self, p, rows, dim, user_side, dev):
        """(Z (R, 128), F (R, 4E) or (R, 2E)) of every row of one side's table"""
        return (torch.empty((rows, p.dnn[0].weight.shape[0]), dtype=torch.float32, device=dev),
                torch.empty((rows, len(self._fields(user_side)) * dim), dtype=torch.float32, device=dev))

    def _side_rows(self, p, x, emb, vec, lo, hi, user_side, buffers):
        z, f = buffers
        d1, w2 = p.dnn[0], self.model._aligned_weight(p.w2, refresh=False)
        f[lo:hi] = vec[:, self._fields(user_side), :].reshape(hi - lo, -1)
        self._zero_other(vec, user_side)                     # (and with the columns the other side's products)
        prod = ops.allpairs_fwd(emb, 6, vec.shape[2], out=self.model._padded_rows(hi - lo, 15, emb.device))
        lz = ops.linear_fwd(emb, p.w1.detach(), None if user_side else p.b1.detach())
        h0 = ops.linear_fwd(prod, w2, None if user_side else p.b2.detach(), residual=lz)
        ops.linear_fwd(h0, d1.weight.detach(), None if user_side else d1.bias.detach(), out=z[lo:hi])

    def _operands(self, p):
        d1 = p.dnn[0].weight.detach()
        cross = p.w2.detach()[:, _CROSS_PAIRS].t().contiguous()              # (8, 256): a cross column of W2 per row
        return (ops.linear_fwd(cross, d1, None).t().contiguous(),)           # (128, 8) = D1 W2[:, cross]

    def _grid_scores(self, shared, users, user0, rows):
        p, (zu, fu), (zi, fi), g = shared
        d2, d3 = p.dnn[1], p.dnn[2]
        return ops.pnn_grid_scores(zu, zi, fu, fi, g, d2.weight, d2.bias, d3.weight, d3.bias, p.out.weight, p.out.bias,
                                   users=users, user0=user0, rows=rows, row_blocks=self.row_blocks)
