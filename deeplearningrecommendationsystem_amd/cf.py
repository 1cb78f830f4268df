"""Neighbourhood collaborative filtering: the reference's UserCF_Final.py / ItemCF_Final.py as a library.

The reference builds a dense 0/1 user x item matrix with ``pivot``, takes ``cosine_similarity`` over all rows (UserCF)
or columns (ItemCF), and for every user loops in Python over the unrated items.  Here the similarity and the
neighbour lists come from one fused kernel (csrc/knn_cf.hip: i8 matrix cores, exact intersection counts, the n x n
similarity never written), the predictions from a second one, and the ranking from ``ctr_topk_rows``.

Semantics (the contract tests/cf_numpy.py restates):

* similarity ``float32(c / sqrt(a b))`` evaluated in float64, c the intersection count, a and b the two row counts;
  0 when a or b is 0 (sklearn's ``normalize`` of a zero row);
* neighbours: positions ``[1 : k+1]`` of the row sorted by similarity descending, index ascending -- position 0 is
  dropped as the reference drops it (``similarities[1:k + 1]``), which is not always the row itself;
* predictions as ``prediction_dating`` / ``prediction_item_based``, accumulated in float32 in neighbour order;
* recommendations: unrated items by prediction descending, item index ascending, padded with -1.

Deliberate deviation: matrix columns are item ids.  The reference's ``pivot`` drops items that never occur in
``ua.base``, after which its ``item_index + 1`` is not the item id.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops, topn

__all__ = ["ImplicitMatrix", "implicit_matrix", "UserCF", "ItemCF", "recall_precision_f1"]


def _pad64(n: int) -> int:
    return max(64, (n + 63) // 64 * 64)


class ImplicitMatrix:
    """the 0/1 user x item matrix as int8 (num_users, cols_pad) on the device, columns = item ids"""

    def __init__(self, data: torch.Tensor, num_users: int, num_items: int):
        self.data, self.num_users, self.num_items = data, num_users, num_items
        self._t = None

    @property
    def counts(self) -> torch.Tensor:
        """int32 interactions per user"""
        return self.data.sum(dim=1, dtype=torch.int32)

    def transposed(self) -> torch.Tensor:
        """int8 (num_items, pad64(num_users)): the item rows ItemCF compares"""
        if self._t is None:
            t = torch.zeros((self.num_items, _pad64(self.num_users)), dtype=torch.int8, device=self.data.device)
            t[:, :self.num_users] = self.data[:, :self.num_items].t()
            self._t = t
        return self._t

    def dense(self) -> np.ndarray:
        """host (num_users, num_items) uint8 copy"""
        return self.data[:, :self.num_items].cpu().numpy().astype(np.uint8)


def implicit_matrix(user_ids, item_ids, num_users: int, num_items: int, device="cuda") -> ImplicitMatrix:
    """implicit feedback from 0-based (user, item) pairs; a pair seen twice counts once (the reference's
    ``rating > 0 -> 1``)"""
    u = torch.as_tensor(user_ids, dtype=torch.int64).reshape(-1)
    i = torch.as_tensor(item_ids, dtype=torch.int64).reshape(-1)
    if u.shape != i.shape:
        raise ValueError("user_ids and item_ids differ in length")
    if num_users < 1 or num_items < 1:
        raise ValueError("num_users and num_items must be positive")
    if u.numel() and (int(u.min()) < 0 or int(u.max()) >= num_users or int(i.min()) < 0 or int(i.max()) >= num_items):
        raise IndexError("a user or item id is outside [0, num_users) x [0, num_items)")
    data = torch.zeros((num_users, _pad64(num_items)), dtype=torch.int8, device=device)
    data[u.to(device), i.to(device)] = 1
    return ImplicitMatrix(data, num_users, num_items)


def _knn(x: torch.Tensor, k: int):
    """positions [1 : k+1] of every row's ranking (index -1 / similarity 0 past the end of a short list)"""
    if k < 1:
        raise ValueError("k must be at least 1")
    if k + 1 > ops.CF_KNN_MAX_K:
        raise ValueError(f"k = {k}: the neighbour kernel keeps k + 1 <= {ops.CF_KNN_MAX_K} entries per row")
    idx, sim = ops.cf_knn(x, x.sum(dim=1, dtype=torch.int32), k + 1)
    return idx[:, 1:].contiguous(), sim[:, 1:].contiguous()


class _NeighbourCF:
    _scores = None   # ops.usercf_scores / ops.itemcf_scores

    def __init__(self, k: int = 10):
        if not 1 <= k <= ops.CF_KNN_MAX_K - 1:
            raise ValueError(f"k = {k}: the neighbour kernel keeps k + 1 <= {ops.CF_KNN_MAX_K} entries per row")
        self.k = k
        self.matrix: Optional[ImplicitMatrix] = None
        self.neighbors = self.neighbor_sims = self._unrated = None

    def _rows(self, matrix: ImplicitMatrix) -> torch.Tensor:
        raise NotImplementedError

    def fit(self, matrix: ImplicitMatrix):
        self.matrix = matrix
        self.neighbors, self.neighbor_sims = _knn(self._rows(matrix), self.k)
        self._unrated = matrix.num_items - matrix.counts.to(torch.int64)   # per user: the scores that are not -inf
        return self

    def _check_fitted(self):
        if self.matrix is None:
            raise RuntimeError("call fit() first")

    def predict(self, users=None) -> torch.Tensor:
        """(len(users), num_items) float32 predictions, -inf on the items a user has rated"""
        self._check_fitted()
        m = self.matrix
        u = topn.users_tensor(users, m.num_users, m.data.device)
        outs = [type(self)._scores(m.data, m.num_items, self.neighbors, self.neighbor_sims, u[s:s + topn.MAX_ROWS])
                for s in range(0, max(1, u.numel()), topn.MAX_ROWS)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def recommend(self, users=None, n: int = 20) -> torch.Tensor:
        """(len(users), n) int64: the n unrated items with the highest prediction, ties by ascending item id, -1 where
        a user has fewer than n unrated items.  Users are scored in chunks, so the workspace stays bounded."""
        self._check_fitted()
        if n < 1:
            raise ValueError("n must be at least 1")
        m = self.matrix
        u = topn.users_tensor(users, m.num_users, m.data.device)

        def chunk_scores(s, e):     # -inf on the rated items and on nothing else (csrc/knn_cf.hip)
            scores = type(self)._scores(m.data, m.num_items, self.neighbors, self.neighbor_sims, u[s:e])
            return scores, self._unrated[u[s:e]]
        return topn.top_n(u.numel(), m.num_items, n, chunk_scores, m.data.device)


class UserCF(_NeighbourCF):
    """UserCF_Final.py: neighbours are users, ``p[u, i] = sum_v s_uv R[v, i] / sum_v s_uv`` over u's k neighbours"""
    _scores = staticmethod(ops.usercf_scores)

    def _rows(self, matrix):
        return matrix.data


class ItemCF(_NeighbourCF):
    """ItemCF_Final.py: neighbours are items, ``p[u, i] = sum_j s_ij R[u, j] / sum_j s_ij`` over i's k neighbours"""
    _scores = staticmethod(ops.itemcf_scores)

    def _rows(self, matrix):
        return matrix.transposed()


def recall_precision_f1(recs, test_users, test_items, users=None, divisor=None):
    """the reference scripts' evaluation loop (UserCF_Final.py:67-91): per evaluated user, recall = |rec & test| /
    |test| (0 without test items), precision = |rec & test| / |set(rec)| (0 for an empty list, where the reference
    divides by zero); each summed and divided by ``divisor``; F1 = 2RP / (R + P).  ``recs`` has one row per user id
    (-1 = no item).  Defaults: every row, divided by their number.  ItemCF_Final.py:58 evaluates users 1..n-1 and
    divides by n -- pass ``users=range(n - 1), divisor=n`` to reproduce it."""
    recs = recs.cpu().numpy() if isinstance(recs, torch.Tensor) else np.asarray(recs)
    tu = np.asarray(test_users.cpu() if isinstance(test_users, torch.Tensor) else test_users).reshape(-1)
    ti = np.asarray(test_items.cpu() if isinstance(test_items, torch.Tensor) else test_items).reshape(-1)
    users = range(recs.shape[0]) if users is None else users
    divisor = recs.shape[0] if divisor is None else divisor
    order = np.argsort(tu, kind="stable")
    tu, ti = tu[order], ti[order]
    recall = precision = 0.0
    for u in users:
        lo, hi = np.searchsorted(tu, u, "left"), np.searchsorted(tu, u, "right")
        test = set(ti[lo:hi].tolist())
        rec = set(int(r) for r in recs[u] if r >= 0)
        same = len(rec & test)
        recall += same / len(test) if test else 0.0
        precision += same / len(rec) if rec else 0.0
    recall /= divisor
    precision /= divisor
    f1 = 2 * recall * precision / (recall + precision) if recall + precision > 0 else 0.0
    return recall, precision, f1
