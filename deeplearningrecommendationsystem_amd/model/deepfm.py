"""DeepFM -- counterpart of the reference's model/deepfm.py:8-95."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops
from ..ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, Layer
from ._base import CatalogueScorer, FeatureModel, Params, SixFieldGridScorer, six_field_specs


def field_vocabs(num_fields, vocab):
    """keyword-only generalisation shared by DeepFM / PNN: ``num_fields`` single-id fields with ``vocab`` rows
    each (an int, or one int per field)"""
    if vocab is None:
        raise ValueError("num_fields=... needs vocab=... (rows per field: an int or one per field)")
    vocabs = [int(vocab)] * num_fields if isinstance(vocab, int) else [int(v) for v in vocab]
    if len(vocabs) != num_fields or num_fields < 2 or num_fields > 32 or min(vocabs) < 1:
        raise ValueError(f"expected 2..32 fields with one positive vocabulary size each, got {num_fields} / {vocab}")
    return vocabs


class FieldsInput:
    """input handling of the N-id-field models: ``x`` is (B, F) int64 ids, or float32 carrying ids as the
    reference's feature matrix does in its two id columns (converted like ``x[:, c].long()``)"""

    @staticmethod
    def ids(x, num_fields):
        if x.dim() != 2 or x.shape[1] != num_fields or x.dtype not in (torch.int64, torch.float32):
            raise ValueError(f"expected a (B,{num_fields}) int64 (or float32) id matrix, got {tuple(x.shape)} {x.dtype}")
        x = x if x.dtype == torch.int64 else x.long()
        return x if x.stride(1) == 1 else x.contiguous()


class DeepFM(FeatureModel):
    """``DeepFM(num_users, num_items, hidden_units, embedding_dim)``;
    ``forward(x: (B,45)) -> (B,1)``.

    Buffers: emb (B,6E) feeds both the deep MLP and the FM term; the last deep
    layer and the wide+FM kernel write the two columns of ``comb`` (B,1+H_last)
    that ``output`` consumes (reference's torch.cat at deepfm.py:80).

    Keyword-only generalisation (BASELINE configs[2], "26 fields x 1e6 vocab"; the reference hard-codes its
    six fields, deepfm.py:14-17): ``DeepFM(None, None, hidden_units, embedding_dim, num_fields=F, vocab=V)``
    builds F single-id fields -- ``embeddings.f`` (V, E) and first-order ``first_order.f`` (V, 1) per field,
    ``first_order_bias`` in place of the ``wide`` Linear (no dense columns) -- and ``forward(x: (B,F) ids)``
    runs the same deep / FM / output structure with the gather fused into the FM kernel
    (``ctr_fields_fm_fwd``).  Defaults leave the reference model unchanged."""

    def __init__(self, num_users, num_items, hidden_units, embedding_dim, *, num_fields=None, vocab=None):
        super().__init__()
        self.num_fields = num_fields
        if num_fields is not None:
            self.vocabs = field_vocabs(num_fields, vocab)
            self.embeddings = nn.ModuleList([nn.Embedding(v, embedding_dim) for v in self.vocabs])
            self.first_order = nn.ModuleList([nn.Embedding(v, 1) for v in self.vocabs])
            self.first_order_bias = nn.Parameter(torch.zeros(1))
            self.linear = nn.Linear(embedding_dim * num_fields, hidden_units[0])
            self.dnn_network = nn.ModuleList([nn.Linear(a, b) for a, b in zip(hidden_units[:-1], hidden_units[1:])])
            self.relu = nn.ReLU()
            self.output = nn.Linear(2, 1)
            for emb in list(self.embeddings) + list(self.first_order):
                xavier_normal_(emb.weight.data)
            return
        self.user_embedding = nn.Embedding(num_users, embedding_dim)
        self.item_embedding = nn.Embedding(num_items, embedding_dim)
        self.age_embedding = nn.Embedding(1, embedding_dim)
        self.gender_embedding = nn.Embedding(2, embedding_dim)
        self.occupation_embedding = nn.Embedding(21, embedding_dim)
        self.movie_embedding = nn.Embedding(19, embedding_dim)
        self.linear = nn.Linear(embedding_dim * 6, hidden_units[0])
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
        deep = [Layer(self.linear.weight, self.linear.bias, ACT_NONE)]
        deep += [Layer(lin.weight, lin.bias, ACT_RELU) for lin in self.dnn_network]
        if self.num_fields is not None:
            return Params(tables=[e.weight for e in self.embeddings], firsts=[e.weight for e in self.first_order],
                          bias=self.first_order_bias, out_w=self.output.weight, out_b=self.output.bias, deep=deep)
        return Params(tables=[e.weight for e in (self.user_embedding, self.item_embedding, self.age_embedding,
                                                 self.gender_embedding, self.occupation_embedding,
                                                 self.movie_embedding)],
                      user1=self.user.weight, item1=self.item.weight, wide_w=self.wide.weight, wide_b=self.wide.bias,
                      out_w=self.output.weight, out_b=self.output.bias, deep=deep)

    def sparse_ids(self, inputs, p):
        """sparse mode: the id tables and their first-order (V,1) companions"""
        if self.num_fields is not None:
            cols = [[] if inputs is None else [inputs[0][:, f]] for f in range(self.num_fields)]
            return list(zip(p.tables + p.firsts, cols + cols))
        cols = [[] if inputs is None else [inputs[0][:, c]] for c in (0, 1)]   # float id columns of the (B,45) matrix
        user, item, *_ = p.tables
        return list(zip((user, item, p.user1, p.item1), cols + cols))

    def forward(self, x):
        if self.num_fields is not None:
            return self._run([FieldsInput.ids(x, self.num_fields)], self._params())
        return self._run_model(x, self._params())

    # ---- N id fields: gather fused with the FM term (csrc/fields.hip)
    def _fields_forward(self, idx, p):
        batch, dim = idx.shape[0], self.linear.in_features // self.num_fields
        *_, last = p.deep
        emb = torch.empty((batch, self.num_fields * dim), dtype=torch.float32, device=idx.device)
        comb = torch.empty((batch, 1 + last.weight.shape[0]), dtype=torch.float32, device=idx.device)
        ops.fields_fm_fwd(idx, p.tables, p.firsts, p.bias, emb, comb[:, 0:1], self._flag)
        acts = ops.mlp_fwd(emb, p.deep, last_out=comb[:, 1:])
        prob = ops.linear_fwd(comb, p.out_w, p.out_b, ACT_SIGMOID)
        return prob, (emb, comb, acts, prob)

    def _fields_backward(self, state, idx, p, gprob, zeros):
        emb, comb, acts, prob = state
        gcomb = torch.empty_like(comb)
        ops.linear_bwd(comb, p.out_w, prob, gprob, ACT_SIGMOID, gcomb, zeros[id(p.out_w)], zeros[id(p.out_b)])
        gemb = torch.empty_like(emb)
        ops.mlp_bwd(acts, p.deep, gcomb[:, 1:], gemb, zeros=zeros)
        ops.fields_fm_bwd(idx, self.vocabs, emb.shape[1] // self.num_fields, emb, gemb, gcomb[:, 0:1],
                          [zeros[id(t)] for t in p.tables], [zeros[id(t)] for t in p.firsts], zeros[id(p.bias)])

    def run_forward(self, inputs, p):
        (x,) = inputs
        if self.num_fields is not None:
            return self._fields_forward(x, p)
        batch, dim = x.shape[0], self.user_embedding.embedding_dim
        *_, last = p.deep
        emb = torch.empty((batch, 6 * dim), dtype=torch.float32, device=x.device)
        ops.embed_fwd(six_field_specs(p.tables, dim), x, batch, emb, self._flag)
        comb = torch.empty((batch, 1 + last.weight.shape[0]), dtype=torch.float32, device=x.device)
        acts = ops.mlp_fwd(emb, p.deep, last_out=comb[:, 1:])
        ops.fm_wide_fwd(emb, 6, dim, x, p.user1, p.item1, p.wide_w, p.wide_b, comb[:, 0:1], self._flag)
        prob = ops.linear_fwd(comb, p.out_w, p.out_b, ACT_SIGMOID)
        return prob, (emb, comb, acts, prob)

    def run_backward(self, state, inputs, p, gprob, zeros):
        (x,) = inputs
        if self.num_fields is not None:
            self._fields_backward(state, x, p, gprob, zeros)
            return
        emb, comb, acts, prob = state
        batch, dim = x.shape[0], self.user_embedding.embedding_dim
        gcomb = torch.empty_like(comb)
        ops.linear_bwd(comb, p.out_w, prob, gprob, ACT_SIGMOID, gcomb, zeros[id(p.out_w)], zeros[id(p.out_b)])
        gemb = torch.empty_like(emb)
        ops.mlp_bwd(acts, p.deep, gcomb[:, 1:], gemb, zeros=zeros)
        ops.fm_wide_bwd(emb, 6, dim, x, p.user1, p.item1, p.wide_w, p.wide_b, gcomb[:, 0:1], zeros[id(p.user1)],
                        zeros[id(p.item1)], zeros[id(p.wide_w)], zeros[id(p.wide_b)], gemb, accumulate=True)
        ops.embed_bwd(six_field_specs(p.tables, dim), x, batch, gemb, zeros)

    def recommendation(self, num_users, user_item, k):
        return self._rank_users(num_users, user_item, k)

    def catalogue_scorer(self, assembler):
        """as ``FeatureModel.catalogue_scorer``; where ``grid_path`` says "grid" the scores come from
        ``ctr_deepfm_grid_scores`` over table rows made once per call, not from the per-sample forward"""
        self._table_sizes()                                   # (refuses the num_fields= model)
        hidden = [self.linear.out_features] + [lin.out_features for lin in self.dnn_network]
        grid = grid_path(hidden, self.user_embedding.embedding_dim) == "grid"
        return (_GridScorer if grid else CatalogueScorer)(self, assembler)


def grid_path(hidden_units, embedding_dim) -> str:
    """how a ``catalogue_scorer`` scores a six-field DeepFM of these shapes: "grid" -- user-side and item-side table
    rows, then ``ctr_deepfm_grid_scores`` -- where the library has that kernel, else "forward": the per-sample forward
    over feature rows assembled chunk by chunk.  A function of shapes alone."""
    return "grid" if ops.deepfm_grid_supported(hidden_units, embedding_dim) else "forward"


class _GridScorer(SixFieldGridScorer):
    """DeepFM on the user x item grid.  Every column of the feature row belongs to the user or to the item and
    ``linear`` has no activation, so with SU / SI the sums of a side's field vectors
        fm = a[u] + b[i] + <SU[u], SI[i]>,   h1 = relu(ZU[u] + ZI[i]),   ZU / ZI = W1 (W0 . a side's columns of emb)
    and the rest of the model runs per pair inside the kernel."""

    def _side_buffers(self, p, rows, dim, user_side, dev):
        """(Z (R, 256), S (R, E), first-order + wide + FM-square term (R,)) of every row of one side's table"""
        return (torch.empty((rows, p.deep[1].weight.shape[0]), dtype=torch.float32, device=dev),
                torch.empty((rows, dim), dtype=torch.float32, device=dev),
                torch.empty(rows, dtype=torch.float32, device=dev))

    def _side_rows(self, p, x, emb, vec, lo, hi, user_side, buffers):
        z, s, c = buffers
        w0, w1 = p.deep[0], p.deep[1]
        wide = p.wide_w.detach().reshape(-1)
        f = vec[:, self._fields(user_side), :]
        total = f.sum(1)
        s[lo:hi] = total
        if user_side:
            first = p.user1.detach()[lo:hi, 0] + (x[:, 2:26] * wide[:24]).sum(1) + p.wide_b.detach()
        else:
            first = p.item1.detach()[lo:hi, 0] + (x[:, 26:45] * wide[24:]).sum(1)
        c[lo:hi] = first + 0.5 * ((total * total).sum(1) - (f * f).sum((1, 2)))
        self._zero_other(vec, user_side)
        t = ops.linear_fwd(emb, w0.weight.detach(), None if user_side else w0.bias.detach())
        ops.linear_fwd(t, w1.weight.detach(), None if user_side else w1.bias.detach(), out=z[lo:hi])

    def _grid_scores(self, shared, users, user0, rows):
        p, (zu, su, a), (zi, si, b) = shared
        w2, w3 = p.deep[2], p.deep[3]
        return ops.deepfm_grid_scores(zu, zi, su, si, a, b, w2.weight.detach(), w2.bias, w3.weight, w3.bias, p.out_w,
                                      p.out_b, users=users, user0=user0, rows=rows, row_blocks=self.row_blocks)
