"""Top-k ranking evaluation on the device: the reference's ``evaluator/ranking.py`` (``Ranking``) and
``data/reader.py``'s ``itemid_matrix`` / ``remove_itemid``, with the reference's numbers.

Semantics (the contract tests/ranking_numpy.py restates).  Rows pair up as ``zip(actual, predicted)``; ``a`` is the
actual row as given (a padded matrix row includes its ``-1`` pads, a ragged row has its true length), ``p`` the
predicted row, ``pk = p[:k]``, and ``-1`` is an ordinary id everywhere:

* precision / recall: ``sum |set(a) & set(pk)|`` over ``sum |set(pk)|`` and over ``sum |set(a)|``; f1 = 2PR / (P + R);
* MAP: ``AP = sum_{i<k, pk[i] in a} hits_i / (i + 1) / len(a)``, averaged;
* NDCG: ``r_j = [p[j] in a]`` over the whole ``p``; dcg over ``j < k``; idcg over ``min(k, sum r)`` leading ones; 0 when
  idcg is 0; averaged;
* MRR: ``1 / (j + 1)`` for the first ``p[j] in a`` over the whole ``p``, else 0; averaged.

Every per-user quantity comes from csrc/rank_eval.hip as a float64 partial; the aggregate is a fixed-order numpy
reduction of those partials, so two runs are bitwise equal.  ``ranking_metrics`` evaluates score rows directly: the
full ranking and the filtered lists are never built.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import ops, topn

__all__ = ["Ranking", "remove_itemid", "itemid_matrix", "ranking_metrics", "ranking_partials", "RankingMetrics",
           "PARTIALS_COLUMNS"]

RankingMetrics = namedtuple("RankingMetrics", "precision recall f1 map ndcg mrr")
PARTIALS_COLUMNS = ("same", "rec", "real", "ap", "dcg", "idcg", "rr")   # the columns of ranking_partials()

_I64_MAX = torch.iinfo(torch.int64).max
_I64_MIN = torch.iinfo(torch.int64).min


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("ranking evaluation runs on the HIP device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------ row containers
class _Rows:
    """id rows on the device: ``vals`` (rows, width) int64, ``lens`` (rows,) int64 (ragged rows: their length)"""

    def __init__(self, vals: torch.Tensor, lens: torch.Tensor):
        self.vals, self.lens = vals, lens

    @property
    def rows(self):
        return self.vals.shape[0]

    def head(self, rows):
        return _Rows(self.vals[:rows], self.lens[:rows])

    def csr(self, keep=None):
        """(offsets, ids): each row's valid entries (``keep``: a further mask) sorted ascending"""
        valid = torch.arange(self.vals.shape[1], device=self.vals.device) < self.lens[:, None]
        if keep is not None:
            valid &= keep
        srt = torch.where(valid, self.vals, _I64_MAX).sort(dim=1).values
        cnt = valid.sum(1)
        ids = srt[torch.arange(srt.shape[1], device=srt.device) < cnt[:, None]]
        off = torch.zeros(self.rows + 1, dtype=torch.int64, device=srt.device)
        torch.cumsum(cnt, 0, out=off[1:])
        return off, ids.contiguous()


def _is_pairs(x):
    return isinstance(x, tuple) and len(x) == 2 and all(np.ndim(t) == 1 or (isinstance(t, torch.Tensor) and t.dim() == 1)
                                                        for t in x)


def _rows_of(x, device, num_rows=None) -> _Rows:
    """a padded 2-D matrix (numpy / tensor), ragged rows (lists), or ``(users, items)`` pairs (row u = user u's items in
    order of appearance, ``num_rows`` rows)"""
    if _is_pairs(x):
        u = np.asarray(x[0].cpu() if isinstance(x[0], torch.Tensor) else x[0], dtype=np.int64)
        i = np.asarray(x[1].cpu() if isinstance(x[1], torch.Tensor) else x[1], dtype=np.int64)
        if u.shape != i.shape:
            raise ValueError("users and items differ in length")
        rows = int(u.max()) + 1 if num_rows is None and u.size else (num_rows or 0)
        if u.size and (int(u.min()) < 0 or int(u.max()) >= rows):
            raise IndexError(f"a user id of the pairs is outside [0, {rows})")
        order = np.argsort(u, kind="stable")
        lens = np.bincount(u, minlength=rows).astype(np.int64)
        start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        pos = np.arange(u.size, dtype=np.int64) - np.repeat(start, lens)
        vals = np.zeros((rows, int(lens.max()) if rows else 0), dtype=np.int64)
        vals[u[order], pos] = i[order]
        return _Rows(torch.from_numpy(vals).to(device), torch.from_numpy(lens).to(device))
    if isinstance(x, torch.Tensor):
        if x.dim() != 2:
            raise ValueError("expected a 2-D id matrix")
        vals = x.to(device=device, dtype=torch.int64).contiguous()
        return _Rows(vals, torch.full((vals.shape[0],), vals.shape[1], dtype=torch.int64, device=device))
    if isinstance(x, np.ndarray) and x.ndim == 2 and x.dtype != object:
        vals = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(device)
        return _Rows(vals, torch.full((vals.shape[0],), vals.shape[1], dtype=torch.int64, device=device))
    rows = [np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r, dtype=np.int64).reshape(-1) for r in x]
    lens = np.array([r.size for r in rows], dtype=np.int64)
    vals = np.zeros((len(rows), int(lens.max()) if rows else 0), dtype=np.int64)
    if rows:
        vals[np.arange(vals.shape[1]) < lens[:, None]] = np.concatenate(rows)
    return _Rows(torch.from_numpy(vals).to(device), torch.from_numpy(lens).to(device))


def _check_err(err: torch.Tensor) -> None:
    e = int(err.item())
    if e & ops.RANK_ERR_SURVIVOR:
        raise ValueError("a score that survives the exclusions is NaN or -inf: it cannot be ranked against the "
                         "excluded items (exclude the items it belongs to, or give it a finite score)")
    if e & ops.RANK_ERR_COUNT:
        raise ValueError("a row's survivor count differs from n_real: a surviving score has the excluded-item bit "
                         "pattern 0xffffffff, or the counts were not made for these exclusions")
    if e:
        raise ValueError(f"inconsistent id rows (error bits {e:#x})")


# ------------------------------------------------------------------------------------------------ reader helpers
def itemid_matrix(data) -> np.ndarray:
    """``MovieLens100K.itemid_matrix`` (data/reader.py:116-133): each user's items in order of appearance (duplicates
    kept), one row per distinct user in ascending user order, padded with -1.  ``data``: a frame with ``user_id`` /
    ``item_id`` columns, or ``(users, items)``."""
    if hasattr(data, "columns"):
        users, items = data["user_id"].to_numpy(), data["item_id"].to_numpy()
    else:
        users, items = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in data)
    users, items = users.reshape(-1), items.reshape(-1)
    uniq, inv, counts = np.unique(users, return_inverse=True, return_counts=True)
    if uniq.size == 0:
        raise ValueError("no interactions")
    order = np.argsort(inv, kind="stable")
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    pos = np.arange(users.size) - np.repeat(start, counts)
    out = np.full((uniq.size, int(counts.max())), -1, dtype=np.result_type(items.dtype, np.int64))
    out[inv[order], pos] = items[order]
    return out


def remove_itemid(recommendation_matrix, other_matrix):
    """``MovieLens100K.remove_itemid`` (data/reader.py:137-159) on the device: drop from row u of the ranking every id
    in ``set(other[u][other[u] >= 0])``, keep the order, pad every row with -1 to the longest one.  -1 entries of the
    ranking survive.  ``other`` with fewer rows than the ranking raises IndexError, as the reference does; when every
    row ends up empty the result is a (rows, 0) float64 array, as the reference's.  The dtype is the reference's too:
    the ranking's own integer dtype when no row is padded, int64 (numpy's promotion with the -1 pads) when one is.  A
    device tensor in gives a device tensor out, anything else a numpy array."""
    dev = _device()
    on_device = isinstance(recommendation_matrix, torch.Tensor) and recommendation_matrix.is_cuda
    given = recommendation_matrix if isinstance(recommendation_matrix, torch.Tensor) else np.asarray(recommendation_matrix)
    rec = torch.as_tensor(given.astype(np.int64) if isinstance(given, np.ndarray) else given)
    if rec.dim() != 2:
        raise ValueError(f"expected a 2-D ranking, got {rec.dim()} dimensions")
    rec = rec.to(device=dev, dtype=torch.int64).contiguous()
    rows = rec.shape[0]
    other = _rows_of(other_matrix, dev)
    if other.rows < rows:
        raise IndexError(f"index {other.rows} is out of bounds for axis 0 with size {other.rows}")
    if rows == 0:
        raise ValueError("max() arg is an empty sequence")
    other = other.head(rows)
    off, ids = other.csr(keep=other.vals >= 0)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    out, out_len = ops.rank_filter(rec, off, ids, err)
    _check_err(err)
    width = int(out_len.max())
    if width == 0:
        res = torch.empty((rows, 0), dtype=torch.float64, device=dev)
    else:
        res = out[:, :width].masked_fill(torch.arange(width, device=dev) >= out_len[:, None], -1)
        if bool((out_len == width).all()):    # no pad: the reference's array keeps the ranking's elements' dtype
            if on_device:
                res = res.to(given.dtype)
            else:
                return res.cpu().numpy().astype(given.dtype)
        elif not on_device:
            return res.cpu().numpy().astype(np.result_type(given.dtype, np.int64))
    return res if on_device else res.cpu().numpy()


# ------------------------------------------------------------------------------------------------ aggregation
def _ratios(parts: np.ndarray, strict: bool):
    same, rec, real = (int(parts[:, c].astype(np.int64).sum()) for c in range(3))
    if strict:
        precision = same / (rec * 1.0)
        recall = same / (real * 1.0)
        return precision, recall, 2 * (precision * recall) / (precision + recall)
    precision = same / rec if rec else float("nan")
    recall = same / real if real else float("nan")
    f1 = 2 * (precision * recall) / (precision + recall) if precision + recall > 0 else float("nan")
    return precision, recall, f1


def _ndcg(parts: np.ndarray) -> np.ndarray:
    dcg, idcg = parts[:, 4], parts[:, 5]
    return np.where(idcg > 0, dcg / np.where(idcg > 0, idcg, 1.0), 0.0)


class Ranking:
    """drop-in for the reference's ``evaluator.ranking.Ranking``: the same methods, numbers and printout, the per-user
    work in csrc/rank_eval.hip (``ctr_rank_metrics_lists``).  ``real_list`` / ``rec_list``: 2-D numpy arrays or
    tensors, or ragged lists of lists.  Raises ZeroDivisionError where the reference does: an empty actual row in
    ``mapk``, no recommended or no actual items, or P + R = 0, in ``precision_recall_f1``."""

    def __init__(self, real_list, rec_list, k):
        self.actual = real_list
        self.predicted = rec_list
        self.k = k
        self._parts = self._alen = None

    def _partials(self):
        if self._parts is None:
            dev = _device()
            if int(self.k) < 1:
                raise ValueError(f"k = {self.k}: the evaluation needs k >= 1")
            act, pred = _rows_of(self.actual, dev), _rows_of(self.predicted, dev)
            rows = min(act.rows, pred.rows)
            act, pred = act.head(rows), pred.head(rows)
            if rows and (bool((pred.vals == _I64_MIN).any()) or bool((act.vals == _I64_MIN).any())):
                raise ValueError("ids must be above INT64_MIN")
            off, ids = act.csr()
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            parts = torch.empty((0, 7), dtype=torch.float64, device=dev)
            if rows:
                parts = ops.rank_metrics_lists(pred.vals, pred.lens.contiguous(), off, ids, act.lens.contiguous(),
                                               int(self.k), err)
            _check_err(err)
            self._parts, self._alen = parts.cpu().numpy(), act.lens.cpu().numpy()
        return self._parts

    def precision_recall_f1(self):
        return _ratios(self._partials(), strict=True)

    @staticmethod
    def apk(actual, predicted, k):
        """average precision of one user: hits over positions < k, divided by len(actual)"""
        hits, score = 0, 0.0
        for i, x in enumerate(list(predicted)[:k]):
            if x in actual:
                hits += 1
                score += hits / (i + 1.0)
        return score / len(actual)

    def mapk(self):
        parts = self._partials()
        if (self._alen == 0).any():
            raise ZeroDivisionError("float division by zero")
        return np.mean(parts[:, 3])

    @staticmethod
    def dcg(relevance_scores, k):
        """sum over the first k relevances r of (2^r - 1) / log2(position + 1), positions from 1"""
        r = np.asarray(relevance_scores)[:k]
        return np.sum((2 ** r - 1) / np.log2(np.arange(2, len(r) + 2)))

    def ndcg(self, actual, predicted, k):
        """dcg of the relevances of the whole predicted row over the dcg of the same relevances sorted; 0 if that is 0"""
        r = [1 if x in actual else 0 for x in predicted]
        ideal = self.dcg(sorted(r, reverse=True), k)
        return self.dcg(r, k) / ideal if ideal > 0 else 0

    def mean_ndcg(self):
        return np.mean(_ndcg(self._partials()))

    @staticmethod
    def rr(actual, predicted):
        """reciprocal rank of the first predicted id in actual, 0 without one"""
        for i, x in enumerate(predicted):
            if x in actual:
                return 1.0 / (i + 1)
        return 0.0

    def mrr(self):
        return np.mean(self._partials()[:, 6])

    def ranking_eval(self):
        precision, recall, f1 = self.precision_recall_f1()
        map_score = self.mapk()
        mean_ndcg_score = self.mean_ndcg()
        mrr_score = self.mrr()
        print(f"""
                - Precision@{self.k}:  {precision}
                - Recall@{self.k}:  {recall}
                - F1 Score@{self.k}:  {f1}
                - MAP@{self.k}: {map_score}
                - Mean NDCG@{self.k}: {mean_ndcg_score}
                - MRR: {mrr_score}
                """)


# ------------------------------------------------------------------------------------------------ scores path
def _exclusions(stages, rows: int, n: int, device):
    """the union of the exclusion stages as a CSR over ``rows`` users (ids in [0, n), distinct, ascending) and the pad
    arithmetic of remove_itemid applied stage by stage: (off, ids, n_real, pad)"""
    m = len(stages)
    keys, tags = [], []
    for t, st in enumerate(stages):
        r = _rows_of(st, device, num_rows=rows)
        if r.rows < rows:
            raise IndexError(f"index {r.rows} is out of bounds for axis 0 with size {r.rows}")
        r = r.head(rows)
        valid = (torch.arange(r.vals.shape[1], device=device) < r.lens[:, None]) & (r.vals >= 0) & (r.vals < n)
        u = torch.arange(rows, device=device)[:, None].expand_as(r.vals)
        keys.append(u[valid] * n + r.vals[valid])
        tags.append(torch.full_like(keys[-1], t))
    n_real = torch.full((rows,), n, dtype=torch.int64, device=device)
    if not keys:
        return (torch.zeros(rows + 1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.int64, device=device),
                n_real, torch.zeros(rows, dtype=torch.int64, device=device))
    comp = torch.sort(torch.cat(keys) * m + torch.cat(tags)).values
    key = comp // m
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    key, stage = key[first], comp[first] % m       # each excluded (user, item) once, with the stage that drops it
    user = key // n
    d = torch.bincount(user * m + stage, minlength=rows * m).view(rows, m)
    width = n
    for t in range(m):
        n_real -= d[:, t]
        width = int((width - d[:, t]).max())      # the longest row after stage t: what remove_itemid pads to
    off = torch.zeros(rows + 1, dtype=torch.int64, device=device)
    torch.cumsum(torch.bincount(user, minlength=rows), 0, out=off[1:])
    return off, (key % n).contiguous(), n_real, width - n_real


def ranking_metrics(scores, real, k: int, exclude=(), chunk=None, num_users=None) -> RankingMetrics:
    """the aggregate of ``ranking_partials`` (same arguments): precision = sum same / sum rec, recall = sum same /
    sum real, f1 = 2PR / (P + R), and the means of AP, NDCG (dcg / idcg, 0 where idcg is 0) and RR, each reduced in a
    fixed order, so two runs are bitwise equal.  Where the reference divides by zero -- no recommended items, no
    actual items, P + R = 0 -- the ratio is nan instead."""
    p = ranking_partials(scores, real, k, exclude=exclude, chunk=chunk, num_users=num_users)
    precision, recall, f1 = _ratios(p, strict=False)
    return RankingMetrics(precision, recall, f1, np.mean(p[:, 3]), np.mean(_ndcg(p)), np.mean(p[:, 6]))


def ranking_partials(scores, real, k: int, exclude=(), chunk=None, num_users=None) -> np.ndarray:
    """``Ranking(real, remove_itemid(..remove_itemid(topk_rows(scores, N), exclude[0]).., exclude[-1]), k)`` without
    the full ranking, per user: each user chunk of scores is masked with the union of the exclusions, ranked by
    ``ctr_topk_rows`` to depth min(k, N), and evaluated by ``ctr_rank_metrics_scores``.  Returns the (users, 7) float64
    partials, columns PARTIALS_COLUMNS: |set(a) & set(p[:k])|, |set(p[:k])|, |set(a)|, AP, dcg, idcg, RR.

    ``scores``: a (U, N) float32 device tensor (left unchanged: each chunk is copied before it is masked), or a
    callable ``scores(start, stop)`` that returns a fresh row-major tensor of the rows of users [start, stop), which is
    masked in place (U = ``num_users``, by default the number of rows of ``real``).  ``real`` and every stage of
    ``exclude``: a padded id matrix (-1 pads are ids of the row, as the reference sees them), ragged rows, or
    ``(users, items)`` pairs (row u = user u's items).  The scores of items a user keeps must be finite or +inf: a
    NaN or -inf survivor raises ValueError (CF's ``predict()`` gives -inf only on rated items, which belong in an
    exclusion stage).  An empty actual row raises ZeroDivisionError, as its AP is undefined.  ``chunk`` users
    are scored at a time (default: ``topn.chunk_rows``, 512 MB of scores), so the workspace stays bounded."""
    dev = _device()
    if int(k) < 1:
        raise ValueError(f"k = {k}: the evaluation needs k >= 1")
    k = int(k)
    if isinstance(scores, torch.Tensor):
        if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_cuda:
            raise ValueError("scores must be a (U, N) float32 device tensor or a callable")
        table = scores
        fetch = lambda s, e: table[s:e]   # noqa: E731
        rows_all, n = scores.shape
    else:
        fetch, n, table = scores, None, None
        rows_all = num_users
    act = _rows_of(real, dev, num_rows=rows_all)
    rows_all = act.rows if rows_all is None else rows_all
    if rows_all < 1:
        raise ValueError("max() arg is an empty sequence")
    if n is None:
        probe = fetch(0, 1)
        n = probe.shape[1]
    rows = min(rows_all, act.rows)                 # zip(actual, predicted)
    act = act.head(rows)
    if rows and bool((act.lens == 0).any()):
        raise ZeroDivisionError("float division by zero (an empty actual row: its AP divides by len(a) = 0)")
    off_x, ids_x, n_real, pad = _exclusions(list(exclude), rows_all, n, dev)
    off_a, ids_a = act.csr()
    alen = act.lens.contiguous()
    kt = min(k, n)
    chunk = chunk or topn.chunk_rows(n)
    buf = torch.empty((min(chunk, max(rows, 1)), n), dtype=torch.float32, device=dev) if table is not None else None
    parts = torch.empty((rows, 7), dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    for s in range(0, rows, chunk):
        e = min(rows, s + chunk)
        sc = fetch(s, e)
        if not isinstance(sc, torch.Tensor) or sc.shape != (e - s, n) or sc.dtype != torch.float32 or not sc.is_cuda:
            raise ValueError(f"scores({s}, {e}) must return a ({e - s}, {n}) float32 device tensor")
        if table is not None or sc.stride(1) != 1:
            b = (buf if buf is not None else torch.empty_like(sc, memory_format=torch.contiguous_format))[:e - s]
            b.copy_(sc)            # the caller's own scores are never masked
        else:
            b = sc
        ops.rank_mask(b, off_x[s:e + 1], ids_x, err)
        top = ops.topk_rows(b, kt).contiguous()      # k > TOPK_MAX_K: a view of the sorted indices
        ops.rank_metrics_scores(b, top, k, off_a[s:e + 1], ids_a, alen[s:e], n_real[s:e], pad[s:e], parts[s:e], err)
    _check_err(err)
    return parts.cpu().numpy()
