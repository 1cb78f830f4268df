"""AFM -- counterpart of the reference's model/afm.py:7-83."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops
from ..ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, FieldSpec
from .._lib import FIELD_BAG, FIELD_ID_F32
from ._base import CatalogueScorer, FeatureModel, Params, SixFieldGridScorer
from .pnn import _CROSS_PAIRS, _ITEM_PAIRS, _USER_PAIRS   # the 15 pair columns by side: AFM's pairs are PNN's

NVEC, NPAIRS = 6, 15


class AFM(FeatureModel):
    """``AFM(num_users, num_items, embedding_dim, attention_dim)``; ``forward(x: (B,45)) -> (B,1)``.

    Vectors [user, item, age broadcast to E, gender, occupation, movie] in one embedding-stage
    launch (the age broadcast is a 1-row bag over a constant table of ones) -> the 15 pair
    products as a (B*15, E) operand -> attention net ``relu(P W + b) h`` on the matrix cores ->
    softmax over the pairs and weighted sum (the DIN pooling kernel with L = 15) ->
    ``output_layer`` with the linear part as the residual of its sigmoid."""

    def __init__(self, num_users, num_items, embedding_dim, attention_dim):
        super().__init__()
        self.user_embedding = nn.Embedding(num_users, embedding_dim)
        self.item_embedding = nn.Embedding(num_items, embedding_dim)
        self.gender_embedding = nn.Embedding(2, embedding_dim)
        self.occupation_embedding = nn.Embedding(21, embedding_dim)
        self.movie_embedding = nn.Embedding(19, embedding_dim)
        self.attention_W = nn.Parameter(torch.randn(embedding_dim, attention_dim))
        self.attention_b = nn.Parameter(torch.randn(attention_dim))
        self.attention_h = nn.Parameter(torch.randn(attention_dim, 1))
        self.output_layer = nn.Linear(embedding_dim, 1)
        self.user = nn.Embedding(num_users, 1)
        self.item = nn.Embedding(num_items, 1)
        self.linear = nn.Linear(1 + 2 + 21 + 19, 1)
        for emb in (self.user_embedding, self.item_embedding, self.gender_embedding, self.occupation_embedding,
                    self.movie_embedding, self.user, self.item):
            xavier_normal_(emb.weight.data)

    def _params(self):
        return Params(tables=[e.weight for e in (self.user_embedding, self.item_embedding, self.gender_embedding,
                                                 self.occupation_embedding, self.movie_embedding)],
                      att_w=self.attention_W, att_b=self.attention_b, att_h=self.attention_h,
                      out_w=self.output_layer.weight, out_b=self.output_layer.bias, user1=self.user.weight,
                      item1=self.item.weight, lin_w=self.linear.weight, lin_b=self.linear.bias)

    def forward(self, x):
        return self._run_model(x, self._params())

    def _ones(self, e, device):
        ones = getattr(self, "_age_ones", None)
        if ones is None or ones.device != device or ones.shape[1] != e:
            ones = torch.ones((1, e), dtype=torch.float32, device=device)
            object.__setattr__(self, "_age_ones", ones)
        return ones

    def _specs(self, tables, e, device):
        user, item, gender, occ, movie = tables
        return [
            FieldSpec(FIELD_ID_F32, e, 0 * e, table=user, src_col=0),
            FieldSpec(FIELD_ID_F32, e, 1 * e, table=item, src_col=1),
            FieldSpec(FIELD_BAG, e, 2 * e, table=self._ones(e, device), src_col=2, bag_size=1),   # age * ones(E)
            FieldSpec(FIELD_BAG, e, 3 * e, table=gender, src_col=3, bag_size=2),
            FieldSpec(FIELD_BAG, e, 4 * e, table=occ, src_col=5, bag_size=21),
            FieldSpec(FIELD_BAG, e, 5 * e, table=movie, src_col=26, bag_size=19),
        ]

    def run_forward(self, inputs, p):
        (x,) = inputs
        batch, e, dev = x.shape[0], self.user_embedding.embedding_dim, x.device
        emb = torch.empty((batch, NVEC * e), dtype=torch.float32, device=dev)
        ops.embed_fwd(self._specs(p.tables, e, dev), x, batch, emb, self._flag)
        pairs = self._padded_rows(batch * NPAIRS, e, dev)
        ops.pairprod_fwd(emb, NVEC, e, pairs)
        wt = p.att_w.t().contiguous()                       # (A, E): nn.Linear layout of the attention map
        hidden = ops.linear_fwd(pairs, self._aligned_weight(wt), p.att_b, ACT_RELU)
        ht = p.att_h.t().contiguous()                       # (1, A)
        score = ops.linear_fwd(hidden, ht, None, ACT_NONE)
        attn = torch.empty((batch, NPAIRS), dtype=torch.float32, device=dev)
        pooled = self._padded_rows(batch, e, dev)
        ops.din_pool_fwd(score, pairs, batch, NPAIRS, e, attn, pooled, summed=True)
        wide = torch.empty((batch, 1), dtype=torch.float32, device=dev)
        ops.fm_wide_fwd(emb[:, :e], 1, e, x, p.user1, p.item1, p.lin_w, p.lin_b, wide, self._flag)
        prob = ops.linear_fwd(pooled, p.out_w, p.out_b, ACT_SIGMOID, residual=wide)
        return prob, (emb, pairs, wt, ht, hidden, attn, pooled, prob)

    def run_backward(self, state, inputs, p, gprob, zeros):
        (x,) = inputs
        emb, pairs, wt, ht, hidden, attn, pooled, prob = state
        batch, e, dev = x.shape[0], self.user_embedding.embedding_dim, x.device
        # sigmoid(wide + pooled W^T + b): the residual's gradient is gz itself
        gz = torch.empty_like(prob)
        ops.act_bwd(prob, gprob, ACT_SIGMOID, gz, accumulate=False)
        gpooled = self._padded_rows(batch, e, dev)
        ops.linear_bwd(pooled, p.out_w, None, gz, ACT_NONE, gpooled, zeros[id(p.out_w)], zeros[id(p.out_b)])
        ops.fm_wide_bwd(emb[:, :e], 1, e, x, p.user1, p.item1, p.lin_w, p.lin_b, gz, zeros[id(p.user1)],
                        zeros[id(p.item1)], zeros[id(p.lin_w)], zeros[id(p.lin_b)], None, accumulate=False)
        gscore = torch.empty((batch * NPAIRS, 1), dtype=torch.float32, device=dev)
        ops.din_pool_bwd(attn, pairs, batch, NPAIRS, e, gpooled, True, gscore)
        ghidden = torch.empty_like(hidden)
        ght = torch.zeros_like(ht)
        ops.linear_bwd(hidden, ht, None, gscore, ACT_NONE, ghidden, ght, None)
        gpairs = self._padded_rows(batch * NPAIRS, e, dev)
        gwt = torch.zeros_like(wt)
        ops.linear_bwd(pairs, self._aligned_weight(wt, refresh=False), hidden, ghidden, ACT_RELU, gpairs, gwt,
                       zeros[id(p.att_b)])
        zeros[id(p.att_w)].copy_(gwt.t())
        zeros[id(p.att_h)].copy_(ght.t())
        gemb = torch.empty_like(emb)
        ops.pairprod_bwd(emb, NVEC, e, gpairs, attn, gpooled, gemb, accumulate=False)
        ops.embed_bwd(self._specs(p.tables, e, dev), x, batch, gemb, zeros)

    def recommendation(self, num_users, user_item, k):
        return self._rank_users(num_users, user_item, k)

    def catalogue_scorer(self, assembler):
        """as ``FeatureModel.catalogue_scorer``; where ``grid_path`` says "grid" the scores come from
        ``ctr_afm_grid_scores`` over table rows made once per call, not from the per-sample forward"""
        grid = grid_path(self.user_embedding.embedding_dim, self.attention_W.shape[1]) == "grid"
        return (_GridScorer if grid else CatalogueScorer)(self, assembler)


def grid_path(embedding_dim, attention_dim) -> str:
    """how a ``catalogue_scorer`` scores an AFM of these shapes: "grid" -- user-side and item-side table rows, then
    ``ctr_afm_grid_scores`` -- where the library has that kernel, else "forward": the per-sample forward over feature
    rows assembled chunk by chunk.  A function of shapes alone."""
    return "grid" if ops.afm_grid_supported(embedding_dim, attention_dim) else "forward"


class _GridScorer(SixFieldGridScorer):
    """AFM on the user x item grid.  Per pair product p the model needs s(p) = h . relu(W^T p + b_att) and t(p) = o . p
    (``output_layer`` of the pooled vector is the pooled t), every field vector belongs to the user or to the item, and
    a softmax can be merged from summaries, so
        out = sigmoid(a[u] + b[i] + n / d),   (m, d, n) = the softmax sums over the user's six products (mU, dU, nU),
                                              the item's one (sI, tI) and the eight cross products FU_a[u] * FI_b[i]
    with the wide part split into a / b (every bias on the item side).  The kernel forms the cross products from the
    sides' field vectors FU (U, 4E) / FI (I, 2E); a side's own products go through the forward's kernels here."""

    side_chunk = 1 << 14         # the pass also holds the (rows * 15, E) products and a side's own with their hidden rows

    def _field_specs(self, p, dim, dev):
        return self.model._specs([t.detach() for t in p.tables], dim, dev)

    def _side_buffers(self, p, rows, dim, user_side, dev):
        """(S (R, 4): a, mU, dU, nU, or (R, 3): b, sI, tI; F (R, 4E) or (R, 2E)) of every row of one side's table"""
        return (torch.empty((rows, 4 if user_side else 3), dtype=torch.float32, device=dev),
                torch.empty((rows, len(self._fields(user_side)) * dim), dtype=torch.float32, device=dev))

    def _side_rows(self, p, x, emb, vec, lo, hi, user_side, buffers):
        s, f = buffers
        rows, dim = hi - lo, vec.shape[2]
        f[lo:hi] = vec[:, self._fields(user_side), :].reshape(rows, -1)
        self._zero_other(vec, user_side)
        pairs = self.model._padded_rows(rows * NPAIRS, dim, emb.device)
        ops.pairprod_fwd(emb, NVEC, dim, pairs)
        cols = _USER_PAIRS if user_side else _ITEM_PAIRS
        own = pairs.view(rows, NPAIRS, dim)[:, cols, :].reshape(rows * len(cols), dim)
        hidden = ops.linear_fwd(own, p.att_w.detach().t().contiguous(), p.att_b.detach(), ACT_RELU)
        logit = ops.linear_fwd(hidden, p.att_h.detach().t().contiguous(), None, ACT_NONE).view(rows, len(cols))
        t = ops.linear_fwd(own, p.out_w.detach(), None, ACT_NONE).view(rows, len(cols))
        lin_w = p.lin_w.detach()[0]
        split = 2 + self.assembler.user_features.shape[1]                     # feature columns [2, split) are the user's
        if user_side:
            m = logit.max(dim=1).values
            e = torch.exp(logit - m[:, None])
            s[lo:hi, 0] = p.user1.detach()[lo:hi, 0] + (x[:, 2:split] * lin_w[:split - 2]).sum(dim=1)
            s[lo:hi, 1], s[lo:hi, 2], s[lo:hi, 3] = m, e.sum(dim=1), (e * t).sum(dim=1)
        else:
            s[lo:hi, 0] = (p.item1.detach()[lo:hi, 0] + (x[:, split:] * lin_w[split - 2:]).sum(dim=1)
                           + p.lin_b.detach() + p.out_b.detach())
            s[lo:hi, 1], s[lo:hi, 2] = logit[:, 0], t[:, 0]

    def _grid_scores(self, shared, users, user0, rows):
        p, (su, fu), (si, fi) = shared
        return ops.afm_grid_scores(su, si, fu, fi, p.att_w, p.att_b, p.att_h, p.out_w, users=users, user0=user0,
                                   rows=rows, row_blocks=self.row_blocks)
