"""Matrix factorisation -- counterpart of the reference's model/mf.py:10-35."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import ops, topn
from .._lib import FIELD_ID_I64
from ._base import CtrModule
from ._grid import UserGridScorer


class _MFFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user_table, item_table, user_idx, item_idx, err_flag):
        prob = ops.mf_fwd(user_table, item_table, user_idx, item_idx, err_flag)
        ctx.save_for_backward(user_table, item_table, user_idx, item_idx, prob)
        return prob

    @staticmethod
    def backward(ctx, gprob):
        user_table, item_table, user_idx, item_idx, prob = ctx.saved_tensors
        zeros = ops.zero_grads([user_table, item_table])
        gu = zeros[id(user_table)] if ctx.needs_input_grad[0] else None
        gi = zeros[id(item_table)] if ctx.needs_input_grad[1] else None
        ops.mf_bwd(user_table, item_table, user_idx, item_idx, prob, gprob.contiguous(), gu, gi)
        return gu, gi, None, None, None


def _softmax_rows(user_table, item_table, user_idx, item_idx, err_flag, grad):
    """gather the users' rows (the embedding stage's id lookup: a bad id reads row 0 and raises the flag) and run the
    row pass of the full softmax: (x, nll, lse, gx_unit)"""
    batch, dim = user_idx.numel(), user_table.shape[1]
    x = torch.empty((batch, dim), dtype=torch.float32, device=user_table.device)
    if batch:
        spec = ops.FieldSpec(FIELD_ID_I64, dim, 0, table=user_table, idx=user_idx)
        ops.embed_fwd([spec], None, batch, x, err_flag)
    return (x,) + ops.softmax_full_rows(x, item_table, item_idx, grad=grad, err_flag=err_flag)


class _SoftmaxNLLFunction(torch.autograd.Function):
    """nll of the item against the whole catalogue (csrc/softmax_full.hip); the (B, I) logits are never written"""

    @staticmethod
    def forward(ctx, user_table, item_table, user_idx, item_idx, err_flag):
        need_u, need_i = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        x, nll, lse, gx = _softmax_rows(user_table, item_table, user_idx, item_idx, err_flag, grad=need_u)
        ctx.save_for_backward(user_table, item_table, user_idx, item_idx, x if need_i else None,
                              lse if need_i else None, gx, nll if need_i else None)
        return nll

    @staticmethod
    def backward(ctx, gnll):
        user_table, item_table, user_idx, item_idx, x, lse, gx, nll = ctx.saved_tensors
        gnll = gnll.contiguous()
        gu = gi = None
        if ctx.needs_input_grad[0]:
            # dX = gnll[b] dX_unit[b], added to the users' rows of the dense gradient; a bad id adds to no row
            rows = user_table.shape[0]
            ok = (user_idx >= 0) & (user_idx < rows)
            gu = ops.zero_grads([user_table])[id(user_table)]
            gu.index_add_(0, user_idx.clamp(0, rows - 1), gx * (gnll * ok).unsqueeze(1))
        if ctx.needs_input_grad[1]:
            gi = ops.softmax_full_cols(x, item_table, item_idx, lse, gnll, nll=nll)
        return gu, gi, None, None, None


class MatrixFactorization(CtrModule):
    """``MatrixFactorization(num_users, num_items, embedding_size)``;
    ``forward(user_indices, item_indices) -> (B,)`` probabilities
    (reference model/mf.py:12-26)."""

    def __init__(self, num_users: int, num_items: int, embedding_size: int):
        super().__init__()
        self.user_embeddings = nn.Embedding(num_users, embedding_size)
        self.item_embeddings = nn.Embedding(num_items, embedding_size)
        xavier_normal_(self.user_embeddings.weight.data)
        xavier_normal_(self.item_embeddings.weight.data)

    def forward(self, user_indices: torch.Tensor, item_indices: torch.Tensor) -> torch.Tensor:
        w_u, w_i = self.user_embeddings.weight, self.item_embeddings.weight
        self._need_device(w_u, user_indices, item_indices)
        out = _MFFunction.apply(w_u, w_i, user_indices.contiguous(), item_indices.contiguous(),
                                self._err_flag(w_u.device))
        self._raise_if_bad_index()
        return out

    def softmax_nll(self, user_indices: torch.Tensor, item_indices: torch.Tensor) -> torch.Tensor:
        """``(B,)`` float32: the cross entropy of each pair's item against EVERY item of the catalogue under the
        scores ``<user, item>`` (no sigmoid, no temperature, no bias, nothing excluded),
        ``log sum_i exp(<p_u, q_i>) - <p_u, q_t>``.  No sampler and no logit matrix: two fused matrix-core passes
        (DESIGN.md section 4r).  Under ``no_grad`` the same values bitwise: the held-out log-likelihood."""
        w_u, w_i = self.user_embeddings.weight, self.item_embeddings.weight
        self._need_device(w_u, user_indices, item_indices)
        user_indices, item_indices = user_indices.contiguous(), item_indices.contiguous()
        if user_indices.dim() != 1 or user_indices.shape != item_indices.shape or user_indices.dtype != torch.int64 \
                or item_indices.dtype != torch.int64:
            raise ValueError(f"softmax_nll: expected two (B,) int64 id tensors, got {tuple(user_indices.shape)} "
                             f"{user_indices.dtype} and {tuple(item_indices.shape)} {item_indices.dtype}")
        flag = self._err_flag(w_u.device)
        if torch.is_grad_enabled() and (w_u.requires_grad or w_i.requires_grad):
            out = _SoftmaxNLLFunction.apply(w_u, w_i, user_indices, item_indices, flag)
        else:
            out = _softmax_rows(w_u.detach(), w_i.detach(), user_indices, item_indices, flag, grad=False)[1]
        self._raise_if_bad_index()
        return out

    def recommendation(self, num_users, num_items):
        """full-catalogue ranking (reference model/mf.py:28-35)"""
        with torch.no_grad():
            dev = self.user_embeddings.weight.device
            users = self.user_embeddings.weight[:num_users]
            items = self.item_embeddings.weight[:num_items]
            scores = ops.linear_fwd(users.contiguous(), items.contiguous(), None)
            return ops.topk_rows(scores, num_items).cpu().numpy()

    # ---- the user x item grid: row scorers and a bounded-workspace ranker (no gradients, training paths untouched)
    def _table_sizes(self):
        return self.user_embeddings.weight.shape[0], self.item_embeddings.weight.shape[0]

    def score_rows(self, start: int, stop: int) -> torch.Tensor:
        """(stop - start, num_items) float32 device tensor, fresh and row-major: the probabilities of users
        [start, stop) against every item -- the ``scores(start, stop)`` callable ``ranking_metrics`` takes.  Not
        chunked: the caller chose the rows."""
        return _GridScorer(self).score_rows(start, stop)

    def score_grid(self, users=None) -> torch.Tensor:
        """(len(users), num_items) float32 probabilities for any 1-D list of user ids (repeats and any order allowed;
        an id outside the table raises IndexError); ``None``: every user.  Not chunked: the caller chose the rows."""
        return _GridScorer(self).score_grid(users)

    def recommend(self, users=None, n: int = 20, exclude=None) -> torch.Tensor:
        """(len(users), n) int64: the items with the highest probability, best first, ties by ascending item id.
        ``exclude``: an ``ObservedPairs`` whose pairs are left out (``ops.rank_mask``), or None; rows with fewer than
        ``n`` items left end in -1.  Users are scored in chunks, so the workspace stays bounded."""
        return _GridScorer(self).recommend(users, n, exclude)


def grid_path(embedding_size) -> str:
    """how ``score_rows`` / ``score_grid`` / ``recommend`` score a model of this embedding size: "grid" --
    ``ctr_lowrank_grid_scores`` over the two tables as they are -- where the library has that kernel, else "forward":
    the per-sample forward over ids generated chunk by chunk"""
    return "grid" if int(embedding_size) > 0 and ops.lowrank_grid_supported(embedding_size) else "forward"


_FORWARD_CHUNK = 1 << 20     # pairs per forward call of the "forward" path


class _GridScorer(UserGridScorer):
    """score rows of the user x item grid of one model.  The operands are the weight tables themselves: no copy is
    made, so a scorer is never stale."""

    row_blocks = 0               # 0: the launch's own geometry (tests set 1, 2 to reach the tile loop at small shapes)

    def __init__(self, model: MatrixFactorization):
        super().__init__(*model._table_sizes(), model.user_embeddings.weight.device)
        self.model = model
        self.path = grid_path(model.user_embeddings.weight.shape[1])

    def _shared(self):
        tables = self.model.user_embeddings.weight.detach(), self.model.item_embeddings.weight.detach()
        self.model._need_device(*tables)
        return tables

    def _scores(self, users, start, stop, shared) -> torch.Tensor:
        rows = users.numel() if users is not None else stop - start
        if self.path == "grid":
            return ops.lowrank_grid_scores(*shared, None, None, users=users, user0=start, rows=rows,
                                           row_blocks=self.row_blocks)
        out = torch.empty((rows, self.num_items), dtype=torch.float32, device=self.device)
        topn.forward_grid(out, _FORWARD_CHUNK,
                          lambda r, i: self.model.forward(users[r] if users is not None else r + start, i))
        return out
