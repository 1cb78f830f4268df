"""The host frame around a grid kernel: a model that scores rows (users, or history rows) against EVERY item brings its
kernel and a few hooks; the range checks, the chunk walks, the exclusion and the ranking are here, once.  Three pieces:
``rank_rows`` (the tail of every ``recommend()``), ``UserGridScorer`` (rows are users of an id table) and
``HistoryGridScorer`` (rows are histories of a (hist, target) model).  Depends on ``ops`` and ``topn`` and on no model."""
from __future__ import annotations

import torch

from .. import ops, topn
from ..ops import Layer


def rank_rows(score_chunk, rows, num_items, n, exclude, row_users, device, before_error=None) -> torch.Tensor:
    """(rows, n) int64: every row's ``n`` best items, best first, ties by ascending item id, -1 where fewer are left.
    ``score_chunk(s, e)``: the fresh (e - s, num_items) scores of rows [s, e); ``exclude``: an ``ObservedPairs`` whose
    pairs are left out (``ops.rank_mask``), or None; ``row_users``: the int64 tensor of the ``exclude`` user of every
    row (None without ``exclude``).  ``before_error()``, if given, runs after the ranking and before the error bits
    of ``exclude`` are read."""
    err = torch.zeros(1, dtype=torch.int32, device=device)

    def chunk_scores(s, e):
        scores = score_chunk(s, e)
        if exclude is None:
            return scores, None
        off, ids = topn.excluded_rows(exclude, row_users[s:e])
        ops.rank_mask(scores, off, ids, err)
        return scores, num_items - off.diff()
    out = topn.top_n(rows, num_items, n, chunk_scores, device)
    if before_error is not None:
        before_error()
    if exclude is not None and int(err.item()):
        raise ValueError(f"exclude: inconsistent id rows (error bits {int(err.item()):#x})")
    return out


class UserGridScorer:
    """Scores of users against every item.  A subclass supplies ``_scores`` and, where the chunks of one public call
    share operands (projected tables, a folded head), ``_shared``; it keeps no copy of a weight: ``_shared`` reads the
    model's parameters at every public call, so a scorer is never stale after an optimizer step."""

    def __init__(self, num_users: int, num_items: int, device):
        self.num_users, self.num_items, self.device = num_users, num_items, device

    def _shared(self):
        """what the chunks of one public call share: made once per call, after the arguments were checked"""
        return None

    def _scores(self, users, start, stop, shared) -> torch.Tensor:
        """(rows, num_items) float32, fresh: the rows of ``users`` (validated 1-D int64 device tensor) or of the users
        [start, stop).  ``shared``: what ``_shared()`` returned for this public call."""
        raise NotImplementedError

    @torch.no_grad()
    def score_rows(self, start: int, stop: int) -> torch.Tensor:
        """(stop - start, num_items) float32 device tensor, fresh and row-major: the probabilities of users
        [start, stop) against every item.  Not chunked: the caller chose the rows."""
        start, stop = int(start), int(stop)
        if not 0 <= start <= stop <= self.num_users:
            raise IndexError(f"users [{start}, {stop}) are outside [0, {self.num_users})")
        return self._scores(None, start, stop, self._shared())

    __call__ = score_rows       # the ``scores(start, stop)`` callable ``ranking_metrics`` takes

    @torch.no_grad()
    def score_grid(self, users=None) -> torch.Tensor:
        """(len(users), num_items) float32 probabilities for any 1-D list of user ids (repeats and any order allowed;
        an id outside the table raises IndexError); ``None``: every user.  Not chunked: the caller chose the rows."""
        if users is None:
            return self._scores(None, 0, self.num_users, self._shared())
        return self._scores(topn.users_tensor(users, self.num_users, self.device), 0, None, self._shared())

    @torch.no_grad()
    def recommend(self, users=None, n: int = 20, exclude=None) -> torch.Tensor:
        """(len(users), n) int64: the items with the highest probability, best first, ties by ascending item id.
        ``exclude``: an ``ObservedPairs`` whose pairs are left out (``ops.rank_mask``), or None; rows with fewer than
        ``n`` items left end in -1.  Users are scored in chunks, so the workspace stays bounded."""
        if n < 1:
            raise ValueError("n must be at least 1")
        if exclude is not None and (exclude.num_users, exclude.num_items) != (self.num_users, self.num_items):
            raise ValueError(f"exclude was built for {exclude.num_users} x {exclude.num_items}, the model is "
                             f"{self.num_users} x {self.num_items}")
        u = topn.users_tensor(users, self.num_users, self.device)
        shared = self._shared()
        return rank_rows(lambda s, e: self._scores(u[s:e], 0, None, shared), u.numel(), self.num_items, n, exclude, u,
                         self.device)


# pairs per chunk of the history grid walk (at least one history row): beyond the scores a chunk holds the fc operand
# and the activations ``mlp_fwd`` keeps -- DIN 4 * (2E + 256 + 128) B = 2 KiB a pair at E = 64 (256 MiB), DIEN
# 4 * (2E + 128 + 64) B = 896 B a pair at E = 16 (112 MiB)
PAIR_CHUNK = 1 << 17


class HistoryGridScorer:
    """Score history rows against every item of one (hist, target) model whose fc stack reads [left | table row].
    What does not depend on the rows is made once, here, and not once per chunk: the item part AT of the split first
    attention layer, and the history part -- the table under ``w_hist`` -- where the table is the smaller row set.
    A subclass supplies ``_grid_path`` (which shapes take the grid path), ``_operands`` (what it makes once) and
    ``_fill`` (the one kernel call that writes the left half of the fc operand)."""

    def __init__(self, model):
        self.model = model
        p = model._params()
        self.table = p.table.detach()
        model._need_device(self.table)
        self.flag = model._err_flag(self.table.device)
        self.fc = [Layer(layer.weight.detach(), layer.bias.detach(), layer.act) for layer in p.fc]
        self.path = self._grid_path(self.table.shape[1], [tuple(layer.weight.shape) for layer in p.att])
        self.hist_table = None
        if self.path == "grid":
            att1, att2, att3 = p.att
            self.w_hist, w_item = self._operands(p, att1.weight.detach())
            self.at = ops.linear_fwd(self.table, w_item, att1.bias.detach())
            self.w2, self.b2 = att2.weight.detach().contiguous(), att2.bias.detach()
            self.w3 = att3.weight.detach().reshape(-1)

    def _grid_path(self, embed_size, attention_dims) -> str:
        """ "grid" or "forward" for a model of these shapes"""
        raise NotImplementedError

    def _operands(self, p, w1):
        """(the weight of the history part, the weight of the item part) out of the first attention layer's ``w1`` =
        [Wa | Wb | Wc]; whatever else ``_fill`` reads is set on ``self`` here"""
        raise NotImplementedError

    def _fill(self, hist, part, by_position: bool, out) -> None:
        """write the left half ``out`` (pairs, E) of the fc operand for the rows ``hist``: ``part`` is the history part
        by table row, or (``by_position``) by history position of ``hist``"""
        raise NotImplementedError

    def _history_part(self, hist, positions):
        """(history part, by position?) for the rows ``hist`` of a call over ``positions`` history positions: the
        projected table where it has no more rows than that (made once), else the projection of the gathered rows"""
        num_items, dim = self.table.shape
        if self.hist_table is None and num_items <= positions:
            self.hist_table = ops.linear_fwd(self.table, self.w_hist, None)
        if self.hist_table is not None:
            return self.hist_table, False
        hrows = torch.empty((hist.numel(), dim), dtype=torch.float32, device=hist.device)
        ops.din_concat_fwd(self.table, hist, torch.zeros(hist.shape[0], dtype=torch.int64, device=hist.device), hrows,
                           None, self.flag, h_only=True)
        return ops.linear_fwd(hrows, self.w_hist, None), True

    def __call__(self, hist) -> torch.Tensor:
        """(R, num_items) float32, fresh: the rows of ``hist`` (validated (R, L) int64 device tensor)"""
        hist = hist.contiguous()
        rows = hist.shape[0]
        num_items, dim = self.table.shape
        dev = self.table.device
        out = torch.empty((rows, num_items), dtype=torch.float32, device=dev)
        if rows == 0:
            return out
        if self.path != "grid":
            topn.forward_grid(out, PAIR_CHUNK, lambda r, i: self.model.forward(hist[r], i))
            return out
        per = max(1, PAIR_CHUNK // num_items)
        for s in range(0, rows, per):
            part = hist[s:s + per]
            fcin = torch.empty((part.shape[0] * num_items, 2 * dim), dtype=torch.float32, device=dev)
            fcin.view(part.shape[0], num_items, 2 * dim)[:, :, dim:] = self.table
            self._fill(part, *self._history_part(part, hist.numel()), fcin[:, :dim])
            # the stage a fused kernel would take over: the fc stack on the (pairs, 2E) operand
            ops.mlp_fwd(fcin, self.fc, last_out=out[s:s + per].view(-1, 1))
        return out
